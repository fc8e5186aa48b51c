#!/usr/bin/env python3
"""Modal analysis at benchmark size: one JSON line per config.

    python tools/modal_bench.py [--configs c2 c2:hex8] [--modes 8] [--device 0] [--out FILE]

For each config (cwf.meshgen.CONFIGS key, ":hex8" for the native hex8 block) it runs cwf.modal.solve_modes on a
FAST handle and reports lambda / Hz, the outer and PCG iteration counts, solve_ms and block_ms (hipEvent time in the
inner solves / in the Gram, fold and rotation kernels) and block_ms's share of their sum, the Gram kernel's GB/s on a
block of the solve's size next to cwf_hip_bandwidth_probe on the same device, and the M-orthonormality defect of the
returned modes (max |Phi^T M Phi - I|, from cwf_hip_block_gram itself). The figures are what this run measured;
eigenvalue accuracy at this size has no dense reference to compare with.
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

from cwf import _lib, modal, pcg, scenarios  # noqa: E402


def gram_bandwidth(system, q, reps=5):
    """GB/s of G = A^T M A + A^T B on device blocks of q columns: bytes read / wall time of the synchronous calls
    (each includes the fold and the q x q copy to the host)."""
    import torch

    D = system.dof_count
    g = torch.Generator(device="cuda").manual_seed(1)
    A = torch.rand(q, D, device="cuda", generator=g) - 0.5
    B = torch.rand(q, D, device="cuda", generator=g) - 0.5
    modal.block_gram(system, A, B).value()  # workspace and first-launch costs
    modal.block_gram(system, A, None, True).value()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        modal.block_gram(system, A, B).value()
    t_ab = (time.perf_counter() - t0) / reps
    t0 = time.perf_counter()
    for _ in range(reps):
        modal.block_gram(system, A, None, True).value()
    t_aa = (time.perf_counter() - t0) / reps
    return dict(gram_ab_gbs=2 * q * D * 4 / t_ab / 1e9, gram_ab_ms=t_ab * 1e3,
                gram_ama_gbs=(q * D * 4 + D / 3 * 8) / t_aa / 1e9, gram_ama_ms=t_aa * 1e3)


def run(key, modes, device):
    name, _, element = key.partition(":")
    case = scenarios.config_case(name, element=element or "tet4")
    P = case.packing
    s = pcg.MatrixFreeSystem.from_packing(P, case.materials, 1.0, 0.0, mode=_lib.MODE_FAST, device=device)
    L = _lib.load()
    t0 = time.perf_counter()
    r = modal.solve_modes(s, modal.ModalSettings(modes=modes))
    wall = time.perf_counter() - t0
    if not r.has_value():
        return dict(config=key, error=r.error().message, context=r.error().context)
    res = r.value()
    t = res.telemetry
    G = modal.block_gram(s, res.modes, None, True).value()
    gbs = C.c_double()
    L.cwf_hip_bandwidth_probe(device, 1 << 30, 5, C.byref(gbs))
    out = dict(config=key, nodes=P.node_count, dofs=P.dof_count, kernel=(L.cwf_hip_system_keff_kernel(s.handle())
                                                                          or b"").decode(),
               modes=modes, block=t.block, eigenvalues=[float(x) for x in res.eigenvalues],
               hz=[float(x) for x in res.hz], outer_iterations=t.outer_iterations, converged=t.converged,
               max_change=t.max_change, pcg_iterations=t.pcg_iterations, solve_ms=t.solve_ms, block_ms=t.block_ms,
               block_share=t.block_ms / (t.solve_ms + t.block_ms), wall_s=wall,
               m_orthonormality_defect=float(np.abs(G - np.eye(modes)).max()), copy_probe_gbs=gbs.value)
    out.update(gram_bandwidth(s, t.block))
    s.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--configs", nargs="+", default=["c2", "c2:hex8"])
    ap.add_argument("--modes", type=int, default=8)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the lines (a JSON list) to this file")
    a = ap.parse_args()
    lines = []
    for key in a.configs:
        lines.append(run(key, a.modes, a.device))
        print(json.dumps(lines[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)
            f.write("\n")
    return 1 if any("error" in x for x in lines) else 0


if __name__ == "__main__":
    sys.exit(main())
