"""Modal analysis over the HIP C-ABI: the lowest natural frequencies and mode shapes of a structure.

    python -m cwf.modal scenario.yaml --modes K [--mode fast|parity] [--shift S] [--xi X --pair I J]
                                      [--out DIR] [--device D]

``solve_modes`` runs ``cwf_hip_modal_solve`` (subspace iteration with Rayleigh-Ritz over the handle's own PCG;
include/cwf_hip.h) and returns the eigenvalues lambda of ``K phi = lambda M phi``, the circular frequencies
``omega = sqrt(lambda)``, the frequencies in Hz and the M-orthonormal modes. ``rayleigh_from_modes`` places the
scenario's damping ratio on two of those frequencies (``physics.compute_rayleigh``). ``block_gram`` and
``block_rotate`` are the device block operations the solver is built from. All arithmetic runs in libcwf_hip.so on
the GPU; there is no CPU path.

The command loads the scenario exactly as ``cwf.run`` does and prints one JSON line; with ``--out`` it writes
``DIR/modes/mode_%05u.vtu``: the mode scaled to a largest nodal displacement of 5 % of the mesh's bounding-box
diagonal, zero velocity and acceleration, the frequency in Hz in the time field.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import os
import sys
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from .pcg import Expected, MatrixFreeSystem, PcgError, PcgSettings
from .physics import Damping, RayleighCoefficients, compute_rayleigh

MAX_BLOCK = 32  # CWF_MODAL_MAX_BLOCK


def default_block(modes: int) -> int:
    """The block size cwf_hip_modal_solve takes for ``block = 0``: min(2 k, k + 8), at most MAX_BLOCK."""
    return min(2 * modes, modes + 8, max(modes, MAX_BLOCK))


@dataclass
class ModalSettings:
    modes: int = 6
    block: int = 0  # 0: default_block(modes)
    max_outer: int = 40
    tolerance: float = 1.0e-6  # largest relative change of the lowest Ritz values between outer iterations
    shift: float = 0.0  # sigma >= 0: the solves run on K + sigma M
    # inner solves (warm starts are the solver's own: Ritz-scaled previous vectors)
    pcg: PcgSettings = field(default_factory=lambda: PcgSettings(20000, 1.0e-6, False))
    kr_from_applies: bool = False  # evaluation only: Kr = Xbar^T (K Xbar) with q extra operator applies


@dataclass
class ModalTelemetry:
    outer_iterations: int = 0
    converged: bool = False
    block: int = 0
    pcg_iterations: int = 0
    max_change: float = 0.0
    solve_ms: float = 0.0
    block_ms: float = 0.0


@dataclass
class ModalResult:
    eigenvalues: np.ndarray  # lambda [k], fp64, ascending
    omega: np.ndarray  # sqrt(lambda), rad/s
    hz: np.ndarray  # omega / 2 pi
    modes: np.ndarray  # f32 [k, 3N], M-orthonormal, caller's node order
    telemetry: ModalTelemetry


def _settings_c(s: ModalSettings) -> "_lib.ModalSettingsC":
    p = _lib.PcgSettingsC(int(s.pcg.max_iterations), float(s.pcg.relative_tolerance), 0, 0)
    return _lib.ModalSettingsC(int(s.modes), int(s.block), int(s.max_outer), 1 if s.kr_from_applies else 0,
                               float(s.tolerance), float(s.shift), p)


def solve_modes(system: MatrixFreeSystem, settings: ModalSettings | None = None) -> Expected:
    """-> Expected[ModalResult]. The system's own scalars are untouched (the call runs on (1, shift))."""
    s = settings or ModalSettings()
    h = system.handle()
    k = max(int(s.modes), 0)
    lam = np.zeros(max(k, 1), np.float64)
    modes = np.zeros((max(k, 1), system.dof_count), np.float32)
    tel = _lib.ModalTelemetryC()
    cs = _settings_c(s)
    st = _lib.load().cwf_hip_modal_solve(h, C.byref(cs), _lib.ptr(lam), _lib.ptr(modes), _lib.PTR_HOST, C.byref(tel))
    if st:
        return Expected(error=system._err())
    lam, modes = lam[:k], modes[:k]
    omega = np.sqrt(np.maximum(lam, 0.0))
    t = ModalTelemetry(int(tel.outer_iterations), bool(tel.converged), int(tel.block), int(tel.pcg_iterations),
                       tel.max_change, tel.solve_ms, tel.block_ms)
    return Expected(ModalResult(lam, omega, omega / (2.0 * math.pi), modes, t))


def _block(a, dof_count: int):
    """A block as the C-ABI takes it: q contiguous f32 [3N] columns = a C-contiguous [q, 3N] array or tensor."""
    if isinstance(a, np.ndarray):
        a = np.ascontiguousarray(a, np.float32).reshape(-1, dof_count)
        return a, a.shape[0], _lib.PTR_HOST
    if a.dim() == 1:
        a = a.reshape(1, -1)
    assert a.is_contiguous() and a.shape[1] == dof_count
    return a, int(a.shape[0]), _lib.PTR_DEVICE


def block_gram(system: MatrixFreeSystem, A, B=None, mass_weighted: bool = False) -> Expected:
    """G [qa, qb] fp64 = A^T W B for blocks A [qa, 3N], B [qb, 3N] (rows = the block's columns; B None: A itself).
    W = I, or the lumped mass on free DOFs and 0 on constrained ones."""
    h = system.handle()
    a, qa, kind = _block(A, system.dof_count)
    b, qb, kind_b = (a, qa, kind) if B is None else _block(B, system.dof_count)
    if kind_b != kind:
        return Expected(error=PcgError("both blocks must be host arrays or both device tensors"))
    G = np.zeros((qa, qb), np.float64)
    st = _lib.load().cwf_hip_block_gram(h, _lib.ptr(a), qa, _lib.ptr(b), qb, int(mass_weighted), _lib.ptr(G), kind)
    return Expected(G) if st == 0 else Expected(error=system._err())


def block_rotate(system: MatrixFreeSystem, X, Q, X_out=None, MX_out=None, with_mass: bool = True) -> Expected:
    """(X', M X') with X' [q_out, 3N] = Q^T-combined columns of X [q_in, 3N]: X'[o] = sum_i Q[i, o] X[i]. Host
    arrays are allocated when X is one; device tensors must be passed in (out of place)."""
    h = system.handle()
    x, q_in, kind = _block(X, system.dof_count)
    Q = np.ascontiguousarray(Q, np.float64)
    if Q.ndim != 2 or Q.shape[0] != q_in:
        return Expected(error=PcgError("Q must be [q_in, q_out]", [f"q_in={q_in}", f"Q={Q.shape}"]))
    q_out = Q.shape[1]
    if kind == _lib.PTR_HOST:
        X_out = np.zeros((q_out, system.dof_count), np.float32)
        MX_out = np.zeros((q_out, system.dof_count), np.float32) if with_mass else None
    elif X_out is None:
        return Expected(error=PcgError("device blocks need X_out"))
    st = _lib.load().cwf_hip_block_rotate(h, _lib.ptr(x), q_in, _lib.ptr(Q), q_out, _lib.ptr(X_out),
                                          _lib.ptr(MX_out), kind)
    return Expected((X_out, MX_out)) if st == 0 else Expected(error=system._err())


def rayleigh_from_modes(xi: float, w_i: float, w_j: float) -> RayleighCoefficients:
    """Rayleigh alpha, beta giving the damping ratio xi at the circular frequencies w_i and w_j: the scenario's
    ``damping: {xi, w1, w2}`` with two computed frequencies in place of guessed ones."""
    return compute_rayleigh(Damping(float(xi), float(w_i), float(w_j)))


def mode_displacement(packing, phi) -> np.ndarray:
    """The mode scaled so that its largest nodal displacement is 5 % of the mesh's bounding-box diagonal (f32)."""
    pos = np.asarray(packing.position0, np.float64).reshape(-1, 3)
    diag = float(np.linalg.norm(pos.max(axis=0) - pos.min(axis=0)))
    peak = float(np.linalg.norm(np.asarray(phi, np.float64).reshape(-1, 3), axis=1).max())
    return (np.asarray(phi, np.float64) * (0.05 * diag / peak if peak > 0 else 0.0)).astype(np.float32)


def write_mode_vtus(out_dir: str, packing, result: ModalResult, system: MatrixFreeSystem) -> list:
    """DIR/modes/mode_%05u.vtu through cwf_write_vtu: displacement = mode_displacement, its strain / stress fields
    (cwf_hip_derived_fields on `system`), velocity = acceleration = 0, time field = the frequency in Hz."""
    from copy import copy

    from .post import compute_derived_fields, write_vtu

    zeros = np.zeros(3 * packing.node_count, np.float32)
    paths = []
    for i, phi in enumerate(result.modes):
        frame = copy(packing)
        frame.displacement = mode_displacement(packing, phi)
        frame.velocity = zeros
        frame.acceleration = zeros
        derived = compute_derived_fields(packing, system=system, displacement=frame.displacement)
        path = os.path.join(out_dir, "modes", f"mode_{i:05d}.vtu")
        rc = write_vtu(path, frame, derived, float(result.hz[i]), i)
        if not rc.has_value():
            raise RuntimeError(f"{rc.error().message} {rc.error().context}")
        paths.append(path)
    return paths


def main(argv=None) -> int:
    from .run import ScenarioError, load_scenario

    ap = argparse.ArgumentParser(prog="python -m cwf.modal", description=__doc__.split("\n\n")[1])
    ap.add_argument("scenario")
    ap.add_argument("--modes", type=int, required=True)
    ap.add_argument("--mode", choices=["parity", "fast"], default="fast")
    ap.add_argument("--shift", type=float, default=0.0)
    ap.add_argument("--xi", type=float, default=None, help="damping ratio to place on the --pair modes")
    ap.add_argument("--pair", type=int, nargs=2, default=(1, 2), metavar=("I", "J"), help="1-based mode numbers")
    ap.add_argument("--out", default=None, help="output root (modes/mode_%%05u.vtu); omitted: no files")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    mode = _lib.MODE_FAST if a.mode == "fast" else _lib.MODE_PARITY
    try:
        cfg, m, P, materials = load_scenario(a.scenario, allow_hex8=mode == _lib.MODE_FAST)
    except ScenarioError as e:
        print(f"error: {e}", file=sys.stderr)
        return 1
    if a.xi is not None and not all(1 <= p <= a.modes for p in a.pair):
        print(f"error: --pair {a.pair[0]} {a.pair[1]} is outside 1..{a.modes}", file=sys.stderr)
        return 1
    system = MatrixFreeSystem.from_packing(P, materials, 1.0, 0.0, mode=mode, device=a.device)
    try:
        r = solve_modes(system, ModalSettings(modes=a.modes, shift=a.shift))
        if not r.has_value():
            print(f"error: {r.error().message} {r.error().context}", file=sys.stderr)
            return 1
        res = r.value()
        t = res.telemetry
        line = dict(scenario=a.scenario, nodes=P.node_count, dofs=P.dof_count, mode=a.mode, modes=a.modes,
                    shift=a.shift, eigenvalues=[float(x) for x in res.eigenvalues],
                    omega=[float(x) for x in res.omega], hz=[float(x) for x in res.hz], block=t.block,
                    outer_iterations=t.outer_iterations, converged=t.converged, pcg_iterations=t.pcg_iterations,
                    max_change=t.max_change, solve_ms=t.solve_ms, block_ms=t.block_ms)
        if a.xi is not None:
            i, j = a.pair
            rc = rayleigh_from_modes(a.xi, res.omega[i - 1], res.omega[j - 1])
            line["rayleigh"] = dict(xi=a.xi, pair=[i, j], alpha=rc.alpha, beta=rc.beta)
        if a.out:
            line["vtu"] = write_mode_vtus(a.out, P, res, system)
        print(json.dumps(line))
        return 0
    finally:
        system.close()


if __name__ == "__main__":
    sys.exit(main())
