#!/usr/bin/env python3
"""Record tests/golden/resident_handoff.json: what the resident solve (csrc/resident.hip) computes with the library in
use (CWF_LIB_PATH selects another build), for tests/test_gpu_resident_handoff.py to compare later builds with, bit for
bit. Per case: static solves from x = 0 after fixed iteration counts (tol 1e-30) and, where the case has one, the full
solve at tol 1e-6; of each the SHA-256 of the x bytes and of the r bytes, the iteration count and the fp64 residual
history as hex floats. The device's CU count goes with them: the box plan, and with it the grouping of the fp64 dot
sums, depends on it.

The file in the tree was recorded on a 256-CU MI355X with the library of the commit before the ring entries' r and p
stayed with the consumer (every published node then stored {r, tag} {Ap, tag} {p, tag}).

usage: python tools/record_resident_golden.py [OUT]   (CWF_VERBOSE=1 prints each plan's max_halo)"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "civiwave-fem_amd")]
GOLDEN = os.path.join(ROOT, "tests", "golden", "resident_handoff.json")

# name: (the case, fixed iteration counts, full solve at tol 1e-6 too). 55x55x55: 56^3 nodes, on 256 CUs 4 x 8 x 8 boxes
# of 14 x 7 x 7 nodes with up to 548 ring entries (CWF_VERBOSE: max_halo 548), so a thread's second ring slot is live
CASES = {
    "40x17x9": (lambda S: S.block_case(40, 17, 9, h=0.1, tol=1e-6, max_iterations=1500), (1, 2, 3, 20), True),
    "rollers-12x10x7": (lambda S: S.roller_case(12, 10, 7, tol=1e-6, max_iterations=1500), (1, 2, 3, 20), True),
    "hex8-33x9x5": (lambda S: S.block_case(33, 9, 5, h=0.1, element="hex8", tol=1e-6, max_iterations=800),
                    (1, 2, 3, 20), True),
    "55x55x55": (lambda S: S.block_case(55, 55, 55, h=0.1, tol=1e-30, max_iterations=20), (3, 20), False),
}


def cu_count():
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def solve(system, rhs, its, tol):
    """One static solve from x = 0: {iterations, converged, x, r (SHA-256), hist (hex floats)}."""
    import numpy as np

    from cwf import pcg

    x, r = np.zeros_like(rhs), np.zeros_like(rhs)
    t = pcg.solve_pcg(system, rhs, pcg.PcgSettings(its, tol), pcg.PcgVectors(x, r)).value()
    return {"iterations": int(t.iterations), "converged": bool(t.converged),
            "x": hashlib.sha256(x.tobytes()).hexdigest(), "r": hashlib.sha256(r.tobytes()).hexdigest(),
            "hist": [float(v).hex() for v in pcg.residual_history(system)]}


def run_case(name):
    """Every solve of one case on a fresh handle: {"kernel", "fixed": {its: solve}, "full": solve or None}."""
    from cwf import _lib, pcg, scenarios

    make, counts, full = CASES[name]
    case = make(scenarios)
    os.environ.pop("CWF_FUSED", None)
    s = pcg.MatrixFreeSystem.from_packing(case.packing, case.materials, *case.scalars(), mode=_lib.MODE_FAST)
    rhs = case.static_rhs()
    out = {"kernel": (_lib.load().cwf_hip_system_keff_kernel(s.handle()) or b"").decode(),
           "fixed": {str(n): solve(s, rhs, n, 1e-30) for n in counts},
           "full": solve(s, rhs, case.cfg.solver.max_iterations, 1e-6) if full else None}
    s.close()
    return out


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    rec = {"cus": cu_count(), "cases": {}}
    for name in CASES:
        rec["cases"][name] = run_case(name)
        c = rec["cases"][name]
        print(f"{name}: {c['kernel']}, full solve "
              f"{c['full']['iterations'] if c['full'] else '-'} iterations", flush=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {out} ({rec['cus']} CUs)")


if __name__ == "__main__":
    main()
