#!/usr/bin/env python3
"""CPU evidence for the explicit stepper's design (DESIGN.md section 3 "Explicit stepper"), in fp64 numpy on the
project's own dense stiffness (oracle.dense_assemble through the same fp64 gradients tests/helpers.py restates):

  1. what the state's precision buys: deviation from an all-fp64 run of (a) fp64 state, (b) f32 state with fp64 math
     rounded at the store, both with the operator's input and output rounded to f32;
  2. the damped stability limit dt <= (2 / w)(sqrt(1 + xi^2) - xi), xi = beta_R w / 2, for the lagged damping force:
     0.9 x it is stable, 1.02 x it and 0.9 x the undamped limit are not;
  3. how close power iteration on M^-1 K gets to lambda_max after 40 and 60 iterations from a hashed start.

    python tools/explicit_cpu_evidence.py [--steps 200 2000 20000]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("civiwave-fem_amd", "oracle"):
    sys.path.insert(0, os.path.join(ROOT, p))

import oracle as O  # noqa: E402
from cwf import scenarios  # noqa: E402


def dense_block(nx, ny, nz, h):
    case = scenarios.block_case(nx, ny, nz, h=h)
    P, coords, tets = case.packing, case.mesh.coords, np.asarray(case.mesh.tets)
    E = tets.shape[0]
    p = coords[tets]  # [E, 4, 3]
    e = p[:, 1:] - p[:, :1]
    v6 = np.einsum("ei,ei->e", e[:, 0], np.cross(e[:, 1], e[:, 2]))
    g = np.stack([np.cross(p[:, 2] - p[:, 1], p[:, 3] - p[:, 1]), np.cross(p[:, 3] - p[:, 0], p[:, 2] - p[:, 0]),
                  np.cross(p[:, 1] - p[:, 0], p[:, 3] - p[:, 0]), np.cross(p[:, 2] - p[:, 0], p[:, 1] - p[:, 0])],
                 axis=1) * (-1.0 / v6)[:, None, None]
    packed = O.Packed(P.node_count, E, P.connectivity, P.gradients, P.volume, P.material_index, P.lumped_mass64,
                      P.lumped_mass, P.offsets, P.element_indices, P.local_indices)
    D = P.dof_count
    K = O.dense_assemble(packed, tets, g.reshape(E, 12), np.abs(v6) / 6.0,
                         np.asarray(case.materials[0].stiffness)).reshape(D, D)
    fixed = (np.repeat(P.bc_mask, 3) & np.tile(np.array([1, 2, 4], np.uint32), P.node_count)) != 0
    m = np.repeat(P.lumped_mass.astype(np.float64), 3)
    f = P.external_force.astype(np.float64)
    s = 1.0 / np.sqrt(m[~fixed])
    lam = float(np.linalg.eigvalsh(K[np.ix_(~fixed, ~fixed)] * s[:, None] * s[None, :])[-1])
    return K, fixed, m, f, lam


def r32(x):
    return x.astype(np.float32).astype(np.float64)


def run(K, fixed, m, f, dt, steps, beta=0.0, op32=False, state32=False, checkpoints=()):
    u, v = np.zeros(m.size), np.zeros(m.size)
    out = {}
    for n in range(steps):
        w = np.where(fixed, 0.0, u + beta * v)
        y = K @ (r32(w) if op32 else w)
        if op32:
            y = r32(y)
        v = np.where(fixed, 0.0, v + dt * ((f - y) / m))
        if state32:
            v = r32(v)
        u = np.where(fixed, 0.0, u + dt * v)
        if state32:
            u = r32(u)
        if not np.isfinite(u).all() or np.abs(u).max() > 1e6:
            return None
        if n + 1 in checkpoints:
            out[n + 1] = (u.copy(), v.copy())
    return out if checkpoints else (u, v)


def dev(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def critical_dt(lam, beta):
    w = np.sqrt(lam)
    xi = beta * w / 2.0
    return (2.0 / w) * (np.sqrt(1.0 + xi * xi) - xi)


def power_iteration(K, fixed, m, iterations):
    i = np.arange(m.size, dtype=np.uint64)
    h = (i * np.uint64(2654435761) + np.uint64(0x9E3779B9)) % np.uint64(1 << 32)
    h ^= h >> np.uint64(15)
    x = np.where(fixed, 0.0, (h % np.uint64(1 << 24)).astype(np.float64) / float(1 << 23) - 1.0)
    lam = 0.0
    for _ in range(iterations):
        y = np.where(fixed, 0.0, K @ x)
        z = y / m
        lam = float(y @ z) / float(y @ x)
        x = z / lam
    return lam


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, nargs="+", default=[200, 2000, 20000])
    a = ap.parse_args()
    K, fixed, m, f, lam = dense_block(4, 3, 3, 0.25)
    dtc = critical_dt(lam, 0.0)
    dt = 0.9 * dtc
    print(f"4x3x3 h=0.25: lambda_max {lam:.6e}  critical dt {dtc:.6e}")
    cps = tuple(a.steps)
    A = run(K, fixed, m, f, dt, max(cps), checkpoints=cps)
    B = run(K, fixed, m, f, dt, max(cps), op32=True, checkpoints=cps)
    Cc = run(K, fixed, m, f, dt, max(cps), op32=True, state32=True, checkpoints=cps)
    for name, R in (("fp64 state", B), ("f32 state ", Cc)):
        print(f"  {name}, f32 operator i/o, deviation from all-fp64 at {cps} steps:  u " +
              " / ".join(f"{dev(R[c][0], A[c][0]):.1e}" for c in cps) + "   v " +
              " / ".join(f"{dev(R[c][1], A[c][1]):.1e}" for c in cps))
    beta = 0.2 * dtc
    dtd = critical_dt(lam, beta)
    for label, step in (("0.9 x damped limit", 0.9 * dtd), ("1.02 x damped limit", 1.02 * dtd),
                        ("0.9 x undamped limit", 0.9 * dtc)):
        ok = run(K, fixed, m, f, step, 4000, beta=beta) is not None
        print(f"  beta_R = 0.2 dt_crit, {label:22s} dt {step:.4e}: {'stable' if ok else 'blows up'}")
    for shape, h in (((4, 3, 3), 0.25), ((8, 5, 4), 0.1)):
        Kb, fb, mb, _, lb = (K, fixed, m, f, lam) if shape == (4, 3, 3) else dense_block(*shape, h)
        print(f"  power iteration {shape} h={h}: " +
              "  ".join(f"{it} it {power_iteration(Kb, fb, mb, it) / lb:.4f}" for it in (40, 60)))


if __name__ == "__main__":
    main()
