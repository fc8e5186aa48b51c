"""Shared by the absorbing-boundary tests: the 1-D soil column, the scheme of include/cwf_hip.h with dashpots in
all-float64 numpy with the dense K (the float32 restatement is explicit_common.scheme_steps), the update matrices by
the library, and the energy of a state."""
import functools
import math
from dataclasses import replace

import numpy as np

from cwf import _lib, absorbing, meshgen, pack, scenarios
from cwf.physics import Assignment, DirichletFix, compute_lame
from explicit_common import constrained, dashpot_rows  # this module's own uses
from helpers import dense_stiffness

SOIL = scenarios.LAYER_MATERIALS[1]  # m1: E 3 GPa, nu 0.3, rho 1800


def wave_speed(material, kind):
    l = compute_lame(material.youngs_modulus, material.poisson_ratio)
    return math.sqrt(((l.lambda_ + 2.0 * l.mu) if kind == "P" else l.mu) / material.density)


def update_matrices(Cn, mass32, alpha, dt):
    """P, Q [n,3,3] of cwf_explicit_dashpot_update for matrices Cn [n,3,3] at nodes of f32 mass mass32 [n]."""
    L = _lib.load()
    Cn = np.ascontiguousarray(Cn, np.float64).reshape(-1, 3, 3)
    P, Q = np.zeros_like(Cn), np.zeros_like(Cn)
    for i in range(len(Cn)):
        rc = L.cwf_explicit_dashpot_update(_lib.ptr(Cn[i]), float(np.float64(np.float32(mass32[i]))), float(alpha),
                                           float(dt), _lib.ptr(P[i]), _lib.ptr(Q[i]))
        assert rc == 0, (i, _lib.last_error(None))
    return P, Q


def scheme_f64(K, mass, fixed, dt, steps, force_at=None, dash=None, u0=None, v0=None, round_operator=False,
               alpha=0.0):
    """The scheme in float64 state and math with the dense K (homogeneous constraints). dash: (ids, C [n,3,3]) with
    P, Q formed here in float64 by numpy. round_operator: the operator's input and output and the force pass through
    float32 (what an f32 operator costs). Yields (n, u_n, v_(n-1/2)) for n = 0 .. steps."""
    D = mass.size
    u = np.zeros(D) if u0 is None else np.where(fixed, 0.0, u0)
    v = np.zeros(D) if v0 is None else np.where(fixed, 0.0, v0)
    h = alpha * dt / 2.0
    c1, c2 = (1.0 - h) / (1.0 + h), dt / (1.0 + h)
    if dash is not None:
        ids, Cn = dash
        I = np.eye(3)
        B = Cn * (dt / (2.0 * mass.reshape(-1, 3)[ids, 0]))[:, None, None]
        A = np.linalg.inv((1.0 + h) * I + B)
        P, Q = A @ ((1.0 - h) * I - B), dt * A
    yield 0, u.copy(), v.copy()
    for n in range(steps):
        w = u
        if round_operator:
            w = w.astype(np.float32).astype(np.float64)
        y = K @ w
        if round_operator:
            y = y.astype(np.float32).astype(np.float64)
        f = force_at(n) if force_at is not None else 0.0
        if round_operator and force_at is not None:
            f = f.astype(np.float32).astype(np.float64)
        g = (f - y) / mass
        vn = c1 * v + c2 * g
        if dash is not None:
            vn.reshape(-1, 3)[ids] = dashpot_rows(P, Q, v.reshape(-1, 3)[ids], g.reshape(-1, 3)[ids])
        v = np.where(fixed, 0.0, vn)
        u = np.where(fixed, 0.0, u + dt * v)
        yield n + 1, u.copy(), v.copy()


def energy(Ku, mass, u, v_minus, v_plus):
    """1/2 vbar^T M vbar + 1/2 u^T K u at step n: vbar = (v_(n-1/2) + v_(n+1/2)) / 2, Ku = K u_n; float64."""
    vb = 0.5 * (np.asarray(v_minus, np.float64) + np.asarray(v_plus, np.float64))
    u = np.asarray(u, np.float64)
    return 0.5 * float(vb @ (mass * vb)) + 0.5 * float(u @ np.asarray(Ku, np.float64))


def energies_f64(K, mass, states):
    """Energy at steps 0 .. len - 2 of a list of (n, u, v) from scheme_f64."""
    return np.array([energy(K @ states[i][1], mass, states[i][1], states[i][2], states[i + 1][2])
                     for i in range(len(states) - 1)])


# ---- the soil column ------------------------------------------------------------------------------------------------
COLUMN_H, COLUMN_NZ = 0.25, 24


@functools.lru_cache(maxsize=None)
def column_case(wave, fixed_base=False, nz=COLUMN_NZ, h=COLUMN_H):
    """kuhn_block(2, 2, nz, h) of the soil m1, every node held in the two axes the wave does not move: a 1-D P wave
    (free axis z) or S wave (free axis x) along z. Groups ALL, BASE (z = 0), TOP (z = max). No loads.
    fixed_base: the BASE nodes are held in every axis."""
    tm = meshgen.kuhn_block(2, 2, nz, h)
    n = np.arange(tm.node_count, dtype=np.uint32)
    tm.node_groups["ALL"] = n
    tm.node_groups["BASE"] = n[:9]
    tm.node_groups["TOP"] = n[-9:]
    mesh = pack.from_tetmesh(tm)
    hold = (True, True, False) if wave == "P" else (False, True, True)
    fixes = [DirichletFix("ALL", hold, tuple(0.0 if a else None for a in hold))]
    if fixed_base:
        fixes.append(DirichletFix("BASE", (True, True, True), (0.0, 0.0, 0.0)))
    cfg = scenarios.make_config(gravity=(0.0, 0.0, 0.0), point=(0.0, 0.0, 0.0), dirichlet=fixes)
    cfg = replace(cfg, materials=[SOIL], assignments=[Assignment("SOLID", SOIL.name)])
    return scenarios.Case(f"column-{wave}", mesh, cfg, pack.build_packed_buffers(mesh, cfg))


@functools.lru_cache(maxsize=None)
def column_dense(wave, fixed_base=False):
    """Dense K (float64 geometry), the f32 lumped mass per DOF as float64, the constrained DOFs, the largest
    eigenvalue of M^-1 K over the free DOFs; read-only, shared."""
    return dense_of(column_case(wave, fixed_base))


def dense_of(case):
    P = case.packing
    D = P.dof_count
    K = dense_stiffness(P, case.mesh.coords, case.mesh.tets, case.materials[0].stiffness).reshape(D, D)
    fixed = constrained(P)
    mass = np.repeat(P.lumped_mass.astype(np.float64), 3)
    s = 1.0 / np.sqrt(mass[~fixed])
    lam = np.linalg.eigvalsh(K[np.ix_(~fixed, ~fixed)] * s[:, None] * s[None, :])
    for a in (K, fixed, mass):
        a.setflags(write=False)
    return dict(K=K, fixed=fixed, mass=mass, lam_max=float(lam[-1]))


def column_axis(wave):
    return 2 if wave == "P" else 0


def column_dashpots(wave):
    """The BASE face's dashpots by cwf.absorbing -> (ids, C [n,3,3])."""
    case = column_case(wave)
    return absorbing.dashpots(case.mesh, case.cfg, absorbing.faces_of_group(case.mesh, "BASE"))


def incident_curve(wave, dt, h=COLUMN_H, nz=COLUMN_NZ, peak=1e-3):
    """The Gaussian incident velocity peak exp(-1/2 ((t - t0) c / sigma)^2), sigma = 6 h, t0 = 4 sigma / c, sampled
    at every step up to t0 + 2 H / c + 5 sigma / c -> (points [(t, value)], steps)."""
    c = wave_speed(SOIL, wave)
    sigma = 6.0 * h
    t0 = 4.0 * sigma / c
    steps = int(math.ceil((t0 + 2.0 * nz * h / c + 5.0 * sigma / c) / dt))
    pts = [(n * dt, peak * math.exp(-0.5 * ((n * dt - t0) * c / sigma) ** 2)) for n in range(steps + 1)]
    return pts, steps


def outgoing_pulse(wave, dt, h=COLUMN_H, nz=COLUMN_NZ, amplitude=1e-4):
    """u_0 = g(z), v_(-1/2) = c g'(z - c dt / 2), g a Gaussian (sigma = 6 h) centred at H / 2: the pulse g(z + c t)
    travelling towards the base -> (u0 [3N], v0 [3N] float64, steps to (H / 2 + 5 sigma) / c)."""
    case = column_case(wave)
    c = wave_speed(SOIL, wave)
    sigma, H = 6.0 * h, nz * h
    z = case.mesh.coords[:, 2]
    k = column_axis(wave)

    def g(x):
        return amplitude * np.exp(-0.5 * ((x - H / 2.0) / sigma) ** 2)

    u0, v0 = np.zeros((z.size, 3)), np.zeros((z.size, 3))
    u0[:, k] = g(z)
    zs = z - c * dt / 2.0
    v0[:, k] = c * (-(zs - H / 2.0) / sigma ** 2) * g(zs)
    return u0.reshape(-1), v0.reshape(-1), int(math.ceil((H / 2.0 + 5.0 * sigma) / c / dt))
