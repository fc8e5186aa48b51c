#!/usr/bin/env python3
"""Layered structured block: the per-plane stencil tables (k_keff_lattice_layered) against the fan groups the same
mesh ran before (CWF_LATTICE=0), same process, alternating.

The mesh is a Kuhn block of n^3 cells (default 149: C3's shape) in three horizontal strata of
scenarios.LAYER_MATERIALS. Both handles are created once; then rounds of fixed-length PCG solves (tolerance 1e-30,
so every iteration runs) alternate between them, after one warm-up solve each, until each path has run for at least
--seconds. Reported per path: PCG iterations per second over all measured rounds (and the spread of the rounds), and
the K_eff kernel's time per launch inside the loop (hipEvent brackets, sampled every 8th launch of separate rounds
so the markers do not sit in the timed rounds).

    python tools/layered_bench.py [--n 149] [--iters 500] [--seconds 1.0] [--element tet4|hex8]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "civiwave-fem_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (before libcwf_hip.so: one HIP runtime per process)

from cwf import _lib, pcg, scenarios  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=149)
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--element", default="tet4", choices=["tet4", "hex8"])
    a = ap.parse_args()
    n = a.n
    layers = [0] * (n // 3) + [1] * (n // 3) + [2] * (n - 2 * (n // 3))
    t0 = time.time()
    case = scenarios.layered_case(n, n, n, layers, h=0.1, element=a.element, xi=0.05, w=(10.0, 100.0), tol=3e-4)
    P = case.packing
    sK, sM = case.scalars()
    L = _lib.load()
    paths = {}
    for name, lattice in (("layered", None), ("other", "0")):
        if lattice is None:
            os.environ.pop("CWF_LATTICE", None)
        else:
            os.environ["CWF_LATTICE"] = lattice
        s = pcg.MatrixFreeSystem.from_packing(P, case.materials, sK, sM, mode=_lib.MODE_FAST)
        kern = (L.cwf_hip_system_keff_kernel(s.handle()) or b"").decode()
        paths[name] = dict(system=s, kernel=kern, rounds=[], keff_ms=0.0, keff_n=0)
    os.environ.pop("CWF_LATTICE", None)
    setup_s = time.time() - t0
    D = P.dof_count
    rhs = torch.from_numpy(case.static_rhs()).cuda()

    def solve(p, timing=0):
        s = p["system"]
        x = torch.zeros(D, device="cuda")
        r = torch.zeros(D, device="cuda")
        L.cwf_hip_system_set_timing(s.handle(), timing)
        torch.cuda.synchronize()
        t = time.perf_counter()
        tel = pcg.solve_pcg(s, rhs, pcg.PcgSettings(a.iters, 1e-30), pcg.PcgVectors(x, r)).value()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
        if timing:
            ms, cnt = C.c_double(), C.c_uint64()
            L.cwf_hip_system_timing(s.handle(), C.byref(ms), C.byref(cnt))
            p["keff_ms"] += ms.value
            p["keff_n"] += cnt.value
        L.cwf_hip_system_set_timing(s.handle(), 0)
        return tel.iterations, dt

    for p in paths.values():  # warm-up
        solve(p)
    spent = {k: 0.0 for k in paths}
    while min(spent.values()) < a.seconds:
        for k, p in paths.items():
            it, dt = solve(p)
            p["rounds"].append(it / dt)
            spent[k] += dt
    for _ in range(2):  # K_eff time per launch, in rounds of their own
        for p in paths.values():
            solve(p, timing=8)
    out = dict(tool="layered_bench", element=a.element, cells=[n, n, n], strata=[n // 3, n // 3, n - 2 * (n // 3)],
               nodes=P.node_count, elements=P.element_count, dofs=D, iters_per_solve=a.iters,
               setup_s=round(setup_s, 1))
    for k, p in paths.items():
        r = np.asarray(p["rounds"])
        out[k] = dict(kernel=p["kernel"], rounds=len(r), seconds=round(spent[k], 3),
                      pcg_it_per_s=round(float(len(r) * a.iters / spent[k]), 1),
                      pcg_it_per_s_min=round(float(r.min()), 1), pcg_it_per_s_max=round(float(r.max()), 1),
                      keff_us=round(p["keff_ms"] * 1e3 / max(1, p["keff_n"]), 2), keff_launches_timed=p["keff_n"])
    out["layered_over_other_pcg"] = round(out["layered"]["pcg_it_per_s"] / out["other"]["pcg_it_per_s"], 3)
    out["layered_over_other_keff_time"] = round(out["layered"]["keff_us"] / max(out["other"]["keff_us"], 1e-9), 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
