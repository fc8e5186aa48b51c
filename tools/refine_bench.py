#!/usr/bin/env python3
"""The refined static solve at benchmark size: one JSON line.

    python tools/refine_bench.py [--config c2] [--device 0] [--inner-sweep 1e-3 1e-4 1e-6] [--out FILE]

On a FAST handle of the config's block with scalars (1, 0) and its static right-hand side, in one process after a
warm-up solve: a plain f32 solve_pcg at tol 1e-6, then the refined solve at 1e-10. Reported: both wall times, the outer
and inner counts, the residual history (relative to |b|), residual_ms and solve_ms (hipEvent time in the fp64 kernels /
in the inner solves) and their ratio, the per-launch time of the fp64 residual tile kernel (cwf_hip_residual_f64_timed)
and, next to it, k_keff_parity_tile's on a PARITY twin of the same mesh in the same run (cwf_hip_keff_timed): the same
tile walk with f32 vectors. --inner-sweep repeats the refined solve at other inner tolerances.

The true residual at this size has no independent check: no dense reference fits, and the f32 PARITY operator cannot
resolve 1e-10. The history is the kernel's own fp64 evaluation, which tests/test_gpu_refine.py pins against dense
algebra at small sizes.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "civiwave-fem_amd"))

from cwf import _lib, pcg, scenarios  # noqa: E402


def refined(s, b, inner_tol):
    t0 = time.perf_counter()
    r = pcg.solve_refined(s, b, pcg.RefineSettings(inner=pcg.PcgSettings(20000, inner_tol, False)))
    wall = time.perf_counter() - t0
    if not r.has_value():
        return dict(inner_tolerance=inner_tol, error=r.error().message, context=r.error().context)
    t = r.value().telemetry
    return dict(inner_tolerance=inner_tol, wall_ms=wall * 1e3, outer_iterations=t.outer_iterations,
                inner_iterations=t.inner_iterations, converged=t.converged, stagnated=t.stagnated,
                history_rel=[float(v / t.rhs_norm) for v in t.history], residual_ms=t.residual_ms,
                solve_ms=t.solve_ms, residual_share=t.residual_ms / (t.residual_ms + t.solve_ms))


def run(key, device, sweep):
    import torch

    case = scenarios.config_case(key, max_iterations=20000)
    P = case.packing
    L = _lib.load()
    s = pcg.MatrixFreeSystem.from_packing(P, case.materials, 1.0, 0.0, mode=_lib.MODE_FAST, device=device)
    b32 = case.static_rhs()
    b = b32.astype(np.float64)
    x32, r32 = np.zeros_like(b32), np.zeros_like(b32)
    plain_set = pcg.PcgSettings(20000, 1e-6, False)
    pcg.solve_pcg(s, b32, plain_set, pcg.PcgVectors(x32, r32)).value()  # warm-up: plan, first launches
    t0 = time.perf_counter()
    tp = pcg.solve_pcg(s, b32, plain_set, pcg.PcgVectors(x32, r32)).value()
    plain_wall = time.perf_counter() - t0
    _, plain_true = pcg.residual_f64(s, b, x32.astype(np.float64)).value()  # also builds the tiles and the workspace
    out = dict(config=key, nodes=P.node_count, dofs=P.dof_count,
               kernel=(L.cwf_hip_system_keff_kernel(s.handle()) or b"").decode(),
               plain=dict(wall_ms=plain_wall * 1e3, iterations=tp.iterations, converged=tp.converged,
                          reported_rel=tp.residual_norm / tp.rhs_norm,
                          true_rel_fp64_kernel=plain_true / float(np.linalg.norm(b))),
               refined=refined(s, b, 1e-4), sweep=[refined(s, b, tol) for tol in sweep])
    ms = C.c_double()
    assert L.cwf_hip_residual_f64_timed(s.handle(), 20, C.byref(ms)) == 0
    out["residual_kernel_ms"] = ms.value
    s.close()
    twin = pcg.MatrixFreeSystem.from_packing(P, case.materials, 1.0, 0.0, mode=_lib.MODE_PARITY, device=device)
    xd = torch.rand(P.dof_count, device=f"cuda:{device}") - 0.5
    yd = torch.zeros_like(xd)
    assert L.cwf_hip_keff_timed(twin.handle(), _lib.ptr(xd), _lib.ptr(yd), 3, C.byref(ms)) == 0  # first launches
    assert L.cwf_hip_keff_timed(twin.handle(), _lib.ptr(xd), _lib.ptr(yd), 20, C.byref(ms)) == 0
    out["parity_kernel"] = (L.cwf_hip_system_keff_kernel(twin.handle()) or b"").decode()
    out["parity_kernel_ms"] = ms.value
    out["residual_over_parity"] = out["residual_kernel_ms"] / ms.value
    twin.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--config", default="c2")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--inner-sweep", type=float, nargs="*", default=[])
    ap.add_argument("--out", default=None, help="also write the line to this file")
    a = ap.parse_args()
    line = run(a.config, a.device, a.inner_sweep)
    print(json.dumps(line), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")
    return 1 if "error" in line["refined"] else 0


if __name__ == "__main__":
    sys.exit(main())
