"""Explicit central-difference (leapfrog) stepper on the lumped mass (include/cwf_hip.h "Explicit stepper").

State u_n and the half-step velocity v_(n-1/2) live in HBM; ``advance(n)`` queues n steps -- each one operator
product and one node pass, no solve -- and synchronises once. The step defaults to ``safety`` x the critical step
estimated by power iteration on M^-1 K (``lambda_max``, ``critical_dt``).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from .pcg import Expected, MatrixFreeSystem
from .physics import Curve, RayleighCoefficients, SolverSettings, TimeSettings
from .transient import TransientState


@dataclass
class ExplicitError:
    message: str
    context: list


@dataclass
class ExplicitTelemetry:
    time: float
    dt: float
    lambda_max: float
    critical_dt: float
    steps: int
    finite: bool

    @classmethod
    def from_c(cls, t: _lib.ExplicitTelemetryC):
        return cls(t.time, t.dt, t.lambda_max, t.critical_dt, int(t.steps), bool(t.finite))


def lambda_max(system: MatrixFreeSystem, iterations: int = 60):
    """-> (estimate of the largest eigenvalue of M^-1 K over the free DOFs, the last iteration's relative change)."""
    lam, change = C.c_double(), C.c_double()
    h = system.handle()
    rc = _lib.load().cwf_hip_lambda_max(h, int(iterations), C.byref(lam), C.byref(change))
    if rc:
        msg, ctx = _lib.last_error(h)
        raise RuntimeError(f"lambda_max failed: {msg} {ctx}")
    return lam.value, change.value


def critical_dt(lam: float, beta: float = 0.0) -> float:
    """The stability limit (2 / w)(sqrt(1 + xi^2) - xi), w = sqrt(lam), xi = beta w / 2 (host only)."""
    return float(_lib.load().cwf_explicit_critical_dt(float(lam), float(beta)))


def curve_value(curve, t: float) -> float:
    """evaluate_curve (cwf.physics) by the library (host only). curve: a Curve or a sequence of (time, value)."""
    pts = curve.points if isinstance(curve, Curve) else list(curve)
    times = np.ascontiguousarray([p[0] for p in pts], np.float64)
    values = np.ascontiguousarray([p[1] for p in pts], np.float64)
    return float(_lib.load().cwf_explicit_curve_value(_lib.ptr(times), _lib.ptr(values), len(pts), float(t)))


class ExplicitStepper(TransientState):
    """ExplicitStepper(packing, materials, rayleigh, solver_settings, time_settings, ...): the constructor shape of
    cwf.stepper.Stepper. solver_settings is unused (there is no solve) and time_settings.initial_dt is the
    implicit scheme's step, so neither sets the explicit step: ``dt`` does (0: safety x the estimated limit).
    State, external force, load pattern, times and close(): cwf.transient.TransientState."""

    DISPLACEMENT, VELOCITY, ACCELERATION, EXTERNAL_FORCE = 0, 1, 2, 4
    _PREFIX, _HANDLE = "cwf_hip_explicit", "_ex"

    def __init__(self, packing, materials, rayleigh: RayleighCoefficients,
                 solver_settings: SolverSettings | None = None, time_settings: TimeSettings | None = None,
                 dt: float = 0.0, safety: float = 0.9, power_iterations: int = 60, mode: int = _lib.MODE_PARITY,
                 device: int = 0, system: MatrixFreeSystem | None = None):
        self.packing = packing
        self.system = system or MatrixFreeSystem.from_packing(packing, materials, 1.0, 0.0, mode, device)
        h = self.system.handle()
        self._f = np.ascontiguousarray(packing.external_force, np.float32)
        self._bcv = np.ascontiguousarray(packing.bc_value, np.float32)
        d = _lib.ExplicitDescC(rayleigh.alpha, rayleigh.beta, float(dt), float(safety), int(power_iterations), 0,
                               _lib.ptr(self._f), _lib.ptr(self._bcv))
        ex = C.c_void_p()
        rc = _lib.load().cwf_hip_explicit_create(h, C.byref(d), C.byref(ex))
        if rc:
            msg, ctx = _lib.last_error(h)
            raise RuntimeError(f"explicit stepper create failed: {msg} {ctx}")
        self._ex = ex
        self.dof_count = packing.dof_count
        self.node_count = packing.node_count

    def advance(self, n_steps: int) -> Expected:
        t = _lib.ExplicitTelemetryC()
        rc = _lib.load().cwf_hip_explicit_advance(self._ex, int(n_steps), C.byref(t))
        if rc:
            msg, ctx = _lib.last_error(self.system._h)
            return Expected(error=ExplicitError(msg, ctx))
        return Expected(ExplicitTelemetry.from_c(t))

    def telemetry(self) -> ExplicitTelemetry:
        """The step, the estimate and the time so far (an advance of no steps)."""
        r = self.advance(0)
        if not r.has_value():
            raise RuntimeError(f"{r.error().message} {r.error().context}")
        return r.value()

    def get_state(self, which: int, out=None):
        if which == self.ACCELERATION:  # the scheme keeps none; the frame writers ask for the Newmark triple
            return np.zeros(self.dof_count, np.float32) if out is None else out
        return super().get_state(which, out)

    def set_load_curve(self, curve):
        """curve: a Curve, a sequence of (time, value), or None to remove it."""
        pts = [] if curve is None else (curve.points if isinstance(curve, Curve) else list(curve))
        times = np.ascontiguousarray([p[0] for p in pts], np.float64)
        values = np.ascontiguousarray([p[1] for p in pts], np.float64)
        self._check(_lib.load().cwf_hip_explicit_set_load_curve(self._ex, _lib.ptr(times), _lib.ptr(values), len(pts)))

    def set_dashpots(self, node_ids, C_n):
        """Absorbing-boundary dashpots (cwf.absorbing.dashpots): distinct node ids and their 3x3 matrices [n,3,3] or
        [9n]. Replaces the previous set; u, v, the step count and the loads are kept. Raises on a refused set, which
        leaves the previous one in force."""
        ids = np.ascontiguousarray(node_ids, np.uint32).reshape(-1)
        mats = np.ascontiguousarray(C_n, np.float64).reshape(-1)
        if mats.size != 9 * ids.size:
            raise ValueError("C must hold 9 values per dashpot node")
        self._check(_lib.load().cwf_hip_explicit_set_dashpots(self._ex, ids.size, _lib.ptr(ids), _lib.ptr(mats)))

    def get_dashpots(self):
        """-> (node_ids u32 [n], C f64 [n,3,3]) as they were set."""
        n = C.c_uint64()
        self._check(_lib.load().cwf_hip_explicit_get_dashpots(self._ex, C.byref(n), None, None))
        ids = np.zeros(n.value, np.uint32)
        mats = np.zeros(9 * n.value, np.float64)
        self._check(_lib.load().cwf_hip_explicit_get_dashpots(self._ex, C.byref(n), _lib.ptr(ids), _lib.ptr(mats)))
        return ids, mats.reshape(-1, 3, 3)

    def clear_dashpots(self):
        self._check(_lib.load().cwf_hip_explicit_set_dashpots(self._ex, 0, None, None))
