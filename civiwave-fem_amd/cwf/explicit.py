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


@dataclass
class MonitorInfo:
    receiver_count: int
    receiver_every: int
    receiver_capacity: int
    receiver_samples: int
    receiver_dropped: int
    energy_every: int
    energy_capacity: int
    energy_samples: int
    energy_dropped: int
    peaks: bool


@dataclass
class ReceiverTraces:
    """Rows of the receiver buffers: u_n and v_(n-1/2) at the step counts ``steps`` (time = steps x dt)."""
    steps: np.ndarray   # u64 [samples]
    time: np.ndarray    # f64 [samples]
    u: np.ndarray       # f32 [samples, receivers, 3]
    v: np.ndarray       # f32 [samples, receivers, 3]
    dt: float
    every: int

    def acceleration(self) -> np.ndarray:
        """The central acceleration (v_(n+1/2) - v_(n-1/2)) / dt at t_n of rows 0 .. samples - 2, f64
        [samples - 1, receivers, 3]; needs every step recorded (receiver_every == 1)."""
        if self.every != 1 or (self.steps.size > 1 and np.any(np.diff(self.steps.astype(np.int64)) != 1)):
            raise ValueError("acceleration() needs receiver_every == 1")
        return np.diff(self.v.astype(np.float64), axis=0) / self.dt


@dataclass
class EnergyLedger:
    """The ledger's rows (include/cwf_hip.h "Monitors"): work and dissipated are cumulative since set or reset."""
    steps: np.ndarray
    time: np.ndarray
    kinetic: np.ndarray
    potential: np.ndarray
    work: np.ndarray
    dissipated: np.ndarray

    def total(self) -> np.ndarray:
        return self.kinetic + self.potential

    def balance(self) -> np.ndarray:
        """total - work + dissipated: constant along a run up to rounding."""
        return self.total() - self.work + self.dissipated


@dataclass
class ElementMonitorInfo:
    gauge_count: int
    gauge_every: int
    gauge_capacity: int
    gauge_samples: int
    gauge_dropped: int
    envelope_every: int
    envelope_samples: int
    von_mises: bool
    shear_strain: bool
    stress_range: bool


@dataclass
class GaugeTraces:
    """Rows of the gauge buffer: {strain[6], stress[6], von_mises} of the gauge elements for u at the step counts
    ``steps`` (time = steps x dt), the rows cwf.post derives from the same u."""
    steps: np.ndarray   # u64 [samples]
    time: np.ndarray    # f64 [samples]
    rows: np.ndarray    # f32 [samples, gauges, 13]

    @property
    def strain(self) -> np.ndarray:
        return self.rows[:, :, 0:6]

    @property
    def stress(self) -> np.ndarray:
        return self.rows[:, :, 6:12]

    @property
    def von_mises(self) -> np.ndarray:
        return self.rows[:, :, 12]


@dataclass
class Envelopes:
    """The envelope maps that are set (the others None), the caller's element order (include/cwf_hip.h "Element
    monitors"): peak von Mises stress and peak effective shear strain f32 [E], the six stresses' minima and maxima
    f32 [E,6]."""
    von_mises: np.ndarray | None = None
    shear_strain: np.ndarray | None = None
    stress_min: np.ndarray | None = None
    stress_max: np.ndarray | None = None


def effective_shear_strain(strain) -> np.ndarray:
    """The envelope's effective shear strain of Voigt strains [..., 6] (engineering shears), float64, in the header's
    statement order: 2 sqrt(J2) of the strain deviator, |gamma| in pure shear (host only)."""
    e = np.asarray(strain, np.float64)
    d0, d1, d2 = e[..., 0] - e[..., 1], e[..., 1] - e[..., 2], e[..., 2] - e[..., 0]
    sd = d0 * d0 + d1 * d1 + d2 * d2
    sg = e[..., 3] * e[..., 3] + e[..., 4] * e[..., 4] + e[..., 5] * e[..., 5]
    return np.sqrt(sd * (2.0 / 3.0) + sg)


MAX_SOURCES = 8  # CWF_EXPLICIT_MAX_SOURCES


@dataclass
class LoadSource:
    """One load source (include/cwf_hip.h "Load sources"): the force A_e c(t - tau_e) on node_ids[e], c the
    piecewise-linear curve; node ids distinct, the caller's numbering."""
    curve: object          # a Curve or a sequence of (time, value)
    node_ids: np.ndarray   # u32 [n]
    amplitude: np.ndarray  # f64 [n,3]
    delay: np.ndarray      # f64 [n], seconds

    def points(self):
        return list(self.curve.points) if isinstance(self.curve, Curve) else [tuple(p) for p in self.curve]


@dataclass
class SourceInfo:
    source_count: int
    entry_count: int
    loaded_nodes: int
    curve_points: int
    device_bytes: int


@dataclass
class TieInfo:
    group_count: int
    member_count: int
    dashed_groups: int
    device_bytes: int


@dataclass
class PlasticityInfo:
    plastic_elements: int
    affected_nodes: int
    yielded_elements: int
    bytes: int


@dataclass
class PlasticState:
    """The plastic state in the caller's element order (include/cwf_hip.h "Plasticity"); elastic elements hold zeros."""
    plastic_strain: np.ndarray             # f64 [E,6], Voigt, engineering shears
    equivalent_plastic_strain: np.ndarray  # f64 [E]
    plastic_work: np.ndarray               # f64 [E], J
    stiffness: np.ndarray                  # f64 [E,6,6] each element's D

    def stress(self, strain, initial_stress=None) -> np.ndarray:
        """D (e - ep) of total strains [E,6] (float64, host): the stress the material carries; with initial_stress
        [E,6] (the soil set's stress at rest) sig0 + D (e - ep)."""
        ee = np.asarray(strain, np.float64) - self.plastic_strain
        st = np.einsum("eij,ej->ei", self.stiffness, ee)
        return st if initial_stress is None else np.asarray(initial_stress, np.float64).reshape(-1, 6) + st


def j2_update(D, yield_stress: float, hardening: float, volume: float, strain, state):
    """The element update of the plasticity scheme by the library (host only). D [6,6] isotropic, strain [6], state
    [8] = ep[6], abar, wp -> (yielded, the new state [8], sigma_p = D ep [6])."""
    Dm = np.ascontiguousarray(D, np.float64).reshape(36)
    e = np.ascontiguousarray(strain, np.float64).reshape(6)
    st = np.array(state, np.float64).reshape(8)
    sp = np.zeros(6, np.float64)
    y = _lib.load().cwf_explicit_j2_update(_lib.ptr(Dm), float(yield_stress), float(hardening), float(volume),
                                           _lib.ptr(e), _lib.ptr(st), _lib.ptr(sp))
    return bool(y), st, sp


def dp_update(D, alpha: float, kappa: float, beta: float, hardening: float, volume: float, strain, state,
              initial_stress=None):
    """The element update of the soil plasticity scheme by the library (host only). D [6,6] isotropic, strain [6],
    state [8] = ep[6], abar, wp, initial_stress [6] or None -> (0 elastic / 1 cone / 2 apex, the new state [8],
    sigma_p = D ep [6])."""
    Dm = np.ascontiguousarray(D, np.float64).reshape(36)
    par = np.array([alpha, kappa, beta, hardening], np.float64)
    e = np.ascontiguousarray(strain, np.float64).reshape(6)
    st = np.array(state, np.float64).reshape(8)
    sp = np.zeros(6, np.float64)
    s0 = None if initial_stress is None else np.ascontiguousarray(initial_stress, np.float64).reshape(6)
    b = _lib.load().cwf_explicit_dp_update(_lib.ptr(Dm), _lib.ptr(par), _lib.ptr(s0), float(volume), _lib.ptr(e),
                                           _lib.ptr(st), _lib.ptr(sp))
    return int(b), st, sp


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

    DISPLACEMENT, VELOCITY, ACCELERATION, EXTERNAL_FORCE, PLASTIC_FORCE = 0, 1, 2, 4, 5
    _PREFIX, _HANDLE = "cwf_hip_explicit", "_ex"

    def __init__(self, packing, materials, rayleigh: RayleighCoefficients,
                 solver_settings: SolverSettings | None = None, time_settings: TimeSettings | None = None,
                 dt: float = 0.0, safety: float = 0.9, power_iterations: int = 60, mode: int = _lib.MODE_PARITY,
                 device: int = 0, system: MatrixFreeSystem | None = None):
        self.packing = packing
        self.materials = materials
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
        self.element_count = packing.element_count

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

    # ---- tied boundaries (include/cwf_hip.h "Tied boundaries") ----
    def set_ties(self, offsets, node_ids):
        """Tie groups (cwf.ties.levels / periodic / merge): group g holds node_ids[offsets[g]:offsets[g + 1]], disjoint
        groups of at least two nodes with equal constraint masks, which then share one velocity. Replaces the previous
        set, which stays in force if this one is refused (RuntimeError); every member's v becomes its group's
        mass-weighted mean. u, the step count, loads, dashpots, monitors and plasticity are kept."""
        off = np.ascontiguousarray(offsets, np.uint64).reshape(-1)
        ids = np.ascontiguousarray(node_ids, np.uint32).reshape(-1)
        if off.size == 0 or int(off[-1]) != ids.size:
            raise ValueError("offsets must hold one entry more than there are groups and end at len(node_ids)")
        self._check(_lib.load().cwf_hip_explicit_set_ties(self._ex, off.size - 1, _lib.ptr(off), _lib.ptr(ids)))

    def get_ties(self):
        """-> (offsets u64 [groups + 1], node_ids u32 [members]) as they were set; ([0], []) without a set."""
        g, m = C.c_uint64(), C.c_uint64()
        self._check(_lib.load().cwf_hip_explicit_get_ties(self._ex, C.byref(g), C.byref(m), None, None))
        off, ids = np.zeros(g.value + 1, np.uint64), np.zeros(m.value, np.uint32)
        if g.value:
            self._check(_lib.load().cwf_hip_explicit_get_ties(self._ex, C.byref(g), C.byref(m), _lib.ptr(off),
                                                              _lib.ptr(ids)))
        return off, ids

    def clear_ties(self):
        self._check(_lib.load().cwf_hip_explicit_set_ties(self._ex, 0, None, None))

    def tie_info(self) -> TieInfo:
        i = _lib.ExplicitTieInfoC()
        self._check(_lib.load().cwf_hip_explicit_tie_info(self._ex, C.byref(i)))
        return TieInfo(int(i.group_count), int(i.member_count), int(i.dashed_groups), int(i.device_bytes))

    # ---- load sources (include/cwf_hip.h "Load sources") ----
    def set_sources(self, sources):
        """sources: LoadSource objects or (curve, node_ids, amplitude [n,3], delay [n]) tuples, at most MAX_SOURCES;
        an empty list removes the set. Replaces the previous set, which stays in force if this one is refused
        (RuntimeError). Sources and a load pattern exclude each other."""
        srcs = [s if isinstance(s, LoadSource) else LoadSource(*s) for s in (sources or [])]
        descs = (_lib.ExplicitSourceDescC * max(len(srcs), 1))()
        keep = []
        for d, s in zip(descs, srcs):
            pts = s.points()
            times = np.ascontiguousarray([p[0] for p in pts], np.float64)
            values = np.ascontiguousarray([p[1] for p in pts], np.float64)
            ids = np.ascontiguousarray(s.node_ids, np.uint32).reshape(-1)
            amp = np.ascontiguousarray(s.amplitude, np.float64).reshape(-1)
            tau = np.ascontiguousarray(s.delay, np.float64).reshape(-1)
            if amp.size != 3 * ids.size or tau.size != ids.size:
                raise ValueError("a source needs 3 amplitudes and 1 delay per node")
            keep.append((times, values, ids, amp, tau))
            d.curve_points, d.times, d.values = len(pts), times.ctypes.data, values.ctypes.data
            d.entry_count, d.node_ids, d.amplitude, d.delay = ids.size, ids.ctypes.data, amp.ctypes.data, tau.ctypes.data
        self._check(_lib.load().cwf_hip_explicit_set_sources(self._ex, descs if srcs else None, len(srcs)))

    def clear_sources(self):
        self._check(_lib.load().cwf_hip_explicit_set_sources(self._ex, None, 0))

    def get_sources(self):
        """-> [LoadSource] as they were set (curve: a list of (time, value))."""
        n = C.c_uint32()
        descs = (_lib.ExplicitSourceDescC * MAX_SOURCES)()
        self._check(_lib.load().cwf_hip_explicit_get_sources(self._ex, C.byref(n), descs))

        def arr(p, ctype, count, dtype):
            return np.ctypeslib.as_array(C.cast(p, C.POINTER(ctype)), shape=(count,)).astype(dtype) if count else \
                np.zeros(0, dtype)

        out = []
        for d in descs[:n.value]:
            m, k = int(d.entry_count), int(d.curve_points)
            t, v = arr(d.times, C.c_double, k, np.float64), arr(d.values, C.c_double, k, np.float64)
            out.append(LoadSource([(float(a), float(b)) for a, b in zip(t, v)], arr(d.node_ids, C.c_uint32, m, np.uint32),
                                  arr(d.amplitude, C.c_double, 3 * m, np.float64).reshape(m, 3),
                                  arr(d.delay, C.c_double, m, np.float64)))
        return out

    def source_info(self) -> SourceInfo:
        i = _lib.ExplicitSourceInfoC()
        self._check(_lib.load().cwf_hip_explicit_source_info(self._ex, C.byref(i)))
        return SourceInfo(int(i.source_count), int(i.entry_count), int(i.loaded_nodes), int(i.curve_points),
                          int(i.device_bytes))

    # ---- plasticity (include/cwf_hip.h "Plasticity") ----
    def set_plasticity(self, yield_stress, hardening=0.0):
        """J2 plasticity with linear isotropic hardening: a yield stress and a hardening modulus per material (scalars
        apply to every material); a yield stress of 0 or inf leaves that material elastic. The state starts at zero.
        Replaces the previous set, which stays in force if this one is refused (RuntimeError)."""
        sy = np.asarray(yield_stress, np.float64)
        sy = np.ascontiguousarray(np.broadcast_to(sy, (len(self.materials),)) if sy.ndim == 0 else sy.reshape(-1))
        H = np.asarray(hardening, np.float64)
        H = np.ascontiguousarray(np.broadcast_to(H, (sy.size,)) if H.ndim == 0 else H.reshape(-1))
        if H.size != sy.size:
            raise ValueError("one hardening modulus per yield stress")
        d = _lib.ExplicitPlasticityDescC(sy.ctypes.data, H.ctypes.data, sy.size)
        self._check(_lib.load().cwf_hip_explicit_set_plasticity(self._ex, C.byref(d)))

    def set_soil_plasticity(self, alpha, kappa, beta=0.0, hardening=0.0, initial_stress=None, node_pass: int = 0):
        """Drucker-Prager plasticity (include/cwf_hip.h "Soil plasticity"): friction alpha, cohesion kappa, dilation
        beta and hardening per material (scalars apply to every material; cwf.soil.from_mohr_coulomb gives them); a
        kappa of inf leaves that material elastic. initial_stress: the stress at rest [E,6] in the caller's element
        order (cwf.soil.geostatic_stress), or None for zeros. Replaces the previous set, J2 or soil, which stays in
        force if this one is refused (RuntimeError). node_pass: 0 leaves the choice of the node pass to the library;
        1 (plain), 2 (cooperative) and 3 (cooperative, short LDS rounds) are for tests and measurements, the results are
        the same bit for bit."""
        given = [np.asarray(x, np.float64) for x in (alpha, kappa, beta, hardening)]
        # scalars take the length of the arrays given with them, or the stepper's material count
        M = next((x.size for x in given if x.ndim), len(self.materials))
        al, ka, be, H = (np.ascontiguousarray(np.broadcast_to(x, (M,)) if x.ndim == 0 else x.reshape(-1))
                         for x in given)
        if not al.size == ka.size == be.size == H.size:
            raise ValueError("one alpha, kappa, beta and hardening per material")
        s0, rows = None, 0
        if initial_stress is not None:
            s0 = np.ascontiguousarray(initial_stress, np.float64)
            if s0.size % 6:
                raise ValueError("initial_stress is [E,6]")
            rows = s0.size // 6
        d = _lib.ExplicitSoilDescC(al.ctypes.data, ka.ctypes.data, be.ctypes.data, H.ctypes.data, al.size,
                                   s0.ctypes.data if s0 is not None else None, rows, int(node_pass), 0)
        self._check(_lib.load().cwf_hip_explicit_set_soil_plasticity(self._ex, C.byref(d)))

    def plasticity_model(self) -> int:
        """0: no plasticity set, 1: J2 (set_plasticity), 2: soil (set_soil_plasticity)."""
        m = C.c_int(0)
        self._check(_lib.load().cwf_hip_explicit_plasticity_model(self._ex, C.byref(m)))
        return int(m.value)

    def clear_plasticity(self):
        """Removes the set in force, J2 or soil."""
        self._check(_lib.load().cwf_hip_explicit_set_plasticity(self._ex, None))

    def reset_plasticity(self):
        """The same set: plastic strain, equivalent plastic strain, plastic work and the correction force zeroed."""
        self._check(_lib.load().cwf_hip_explicit_reset_plasticity(self._ex))

    def plasticity_info(self) -> PlasticityInfo:
        i = _lib.ExplicitPlasticityInfoC()
        self._check(_lib.load().cwf_hip_explicit_plasticity_info(self._ex, C.byref(i)))
        return PlasticityInfo(int(i.plastic_elements), int(i.affected_nodes), int(i.yielded_elements), int(i.bytes))

    def plasticity(self) -> PlasticState:
        E = self.element_count
        ep, abar, wp = np.zeros((E, 6), np.float64), np.zeros(E, np.float64), np.zeros(E, np.float64)
        self._check(_lib.load().cwf_hip_explicit_read_plasticity(self._ex, _lib.ptr(ep), _lib.ptr(abar), _lib.ptr(wp), E))
        D = np.stack([np.asarray(m.stiffness, np.float64).reshape(6, 6) for m in self.materials])
        return PlasticState(ep, abar, wp, D[np.asarray(self.packing.material_index, np.int64)])

    # ---- monitors (include/cwf_hip.h "Monitors") ----
    def set_monitors(self, receivers=None, receiver_every: int = 1, receiver_capacity: int = 0, peaks: bool = False,
                     energy_every: int = 0, energy_capacity: int = 0):
        """Receiver traces at the nodes ``receivers`` (distinct ids) every ``receiver_every`` steps, peak maps, and the
        energy ledger every ``energy_every`` steps (0: none); capacities in samples. Replaces the previous set, which
        stays in force if this one is refused (RuntimeError)."""
        nodes = np.zeros(0, np.uint32) if receivers is None else np.ascontiguousarray(receivers, np.uint32).reshape(-1)
        d = _lib.ExplicitMonitorDescC(nodes.size, _lib.ptr(nodes) if nodes.size else None,
                                      int(receiver_every) if nodes.size else 0,
                                      int(receiver_capacity) if nodes.size else 0, int(energy_every),
                                      int(energy_capacity) if energy_every else 0, 1 if peaks else 0, 0)
        self._check(_lib.load().cwf_hip_explicit_set_monitors(self._ex, C.byref(d)))

    def clear_monitors(self):
        self._check(_lib.load().cwf_hip_explicit_set_monitors(self._ex, None))

    def reset_monitors(self):
        """The same set: sample counts rewound, peaks and cumulative sums zeroed."""
        self._check(_lib.load().cwf_hip_explicit_reset_monitors(self._ex))

    def monitor_info(self) -> MonitorInfo:
        i = _lib.ExplicitMonitorInfoC()
        self._check(_lib.load().cwf_hip_explicit_monitor_info(self._ex, C.byref(i)))
        return MonitorInfo(*(int(getattr(i, n)) for n, _ in _lib.ExplicitMonitorInfoC._fields_[:9]), bool(i.peaks))

    def receiver_traces(self) -> ReceiverTraces:
        i = self.monitor_info()
        n, r = i.receiver_samples, i.receiver_count
        steps = np.zeros(n, np.uint64)
        u, v = np.zeros((n, r, 3), np.float32), np.zeros((n, r, 3), np.float32)
        self._check(_lib.load().cwf_hip_explicit_read_receivers(self._ex, 0, n, _lib.ptr(steps), _lib.ptr(u),
                                                                _lib.ptr(v)))
        dt = self.time_step()
        return ReceiverTraces(steps, steps.astype(np.float64) * dt, u, v, dt, i.receiver_every)

    def peaks(self):
        """-> (peak_u, peak_v, peak_a), f32 [N] each, the caller's node order."""
        out = [np.zeros(self.node_count, np.float32) for _ in range(3)]
        self._check(_lib.load().cwf_hip_explicit_read_peaks(self._ex, _lib.ptr(out[0]), _lib.ptr(out[1]),
                                                            _lib.ptr(out[2]), self.node_count, _lib.PTR_HOST))
        return tuple(out)

    def energy(self) -> EnergyLedger:
        n = self.monitor_info().energy_samples
        steps = np.zeros(n, np.uint64)
        rows = np.zeros((n, 4), np.float64)
        self._check(_lib.load().cwf_hip_explicit_read_energy(self._ex, 0, n, _lib.ptr(steps), _lib.ptr(rows)))
        return EnergyLedger(steps, steps.astype(np.float64) * self.time_step(), rows[:, 0].copy(), rows[:, 1].copy(),
                            rows[:, 2].copy(), rows[:, 3].copy())

    # ---- element monitors (include/cwf_hip.h "Element monitors") ----
    def set_element_monitors(self, gauges=None, gauge_every: int = 1, gauge_capacity: int = 0,
                             envelope_every: int = 0, von_mises: bool = False, shear_strain: bool = False,
                             stress_range: bool = False):
        """Gauge rows {strain, stress, von Mises} at the elements ``gauges`` (distinct ids) every ``gauge_every``
        steps, and every ``envelope_every`` steps (0: none) the envelope maps asked for: peak von Mises stress, peak
        effective shear strain, min / max of the six stresses. A set of its own next to set_monitors'. Replaces the
        previous set, which stays in force if this one is refused (RuntimeError)."""
        elems = np.zeros(0, np.uint32) if gauges is None else np.ascontiguousarray(gauges, np.uint32).reshape(-1)
        maps = (_lib.ENVELOPE_VON_MISES if von_mises else 0) | (_lib.ENVELOPE_SHEAR_STRAIN if shear_strain else 0) | \
            (_lib.ENVELOPE_STRESS_RANGE if stress_range else 0)
        d = _lib.ExplicitElementMonitorDescC(elems.size, _lib.ptr(elems) if elems.size else None,
                                             int(gauge_every) if elems.size else 0,
                                             int(gauge_capacity) if elems.size else 0, int(envelope_every), maps, 0)
        self._check(_lib.load().cwf_hip_explicit_set_element_monitors(self._ex, C.byref(d)))

    def clear_element_monitors(self):
        self._check(_lib.load().cwf_hip_explicit_set_element_monitors(self._ex, None))

    def reset_element_monitors(self):
        """The same set: sample counts rewound, the maps back at their start values."""
        self._check(_lib.load().cwf_hip_explicit_reset_element_monitors(self._ex))

    def element_monitor_info(self) -> ElementMonitorInfo:
        i = _lib.ExplicitElementMonitorInfoC()
        self._check(_lib.load().cwf_hip_explicit_element_monitor_info(self._ex, C.byref(i)))
        m = int(i.envelope_maps)
        return ElementMonitorInfo(*(int(getattr(i, n)) for n, _ in _lib.ExplicitElementMonitorInfoC._fields_[:7]),
                                  bool(m & _lib.ENVELOPE_VON_MISES), bool(m & _lib.ENVELOPE_SHEAR_STRAIN),
                                  bool(m & _lib.ENVELOPE_STRESS_RANGE))

    def gauge_traces(self) -> GaugeTraces:
        i = self.element_monitor_info()
        n, g = i.gauge_samples, i.gauge_count
        steps = np.zeros(n, np.uint64)
        rows = np.zeros((n, g, 13), np.float32)
        self._check(_lib.load().cwf_hip_explicit_read_gauges(self._ex, 0, n, _lib.ptr(steps), _lib.ptr(rows)))
        return GaugeTraces(steps, steps.astype(np.float64) * self.time_step(), rows)

    def envelopes(self) -> Envelopes:
        """The maps that are set; RuntimeError "envelope map is not set" when there is none."""
        i = self.element_monitor_info()
        E = self.element_count
        if not (i.von_mises or i.shear_strain or i.stress_range):
            self._check(_lib.load().cwf_hip_explicit_read_envelopes(self._ex, _lib.ptr(np.zeros(max(E, 1), np.float32)),
                                                                    None, None, None, E, _lib.PTR_HOST))
        out = Envelopes(np.zeros(E, np.float32) if i.von_mises else None,
                        np.zeros(E, np.float32) if i.shear_strain else None,
                        np.zeros((E, 6), np.float32) if i.stress_range else None,
                        np.zeros((E, 6), np.float32) if i.stress_range else None)
        self._check(_lib.load().cwf_hip_explicit_read_envelopes(
            self._ex, _lib.ptr(out.von_mises), _lib.ptr(out.shear_strain), _lib.ptr(out.stress_min),
            _lib.ptr(out.stress_max), E, _lib.PTR_HOST))
        return out
