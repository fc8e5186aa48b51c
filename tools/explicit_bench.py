#!/usr/bin/env python3
"""Measure the explicit stepper: steps/s next to the operator's own time and to the Newmark stepper.

    python tools/explicit_bench.py [--configs c2 c3 c2:hex8] [--steps 2000] [--newmark-steps 3] [--out FILE]

Per config (a FAST handle of the block, created with scalars (1, 0)), in one process and one JSON line each, appended
to --out (default profiles/explicit_c2.json):
  - the explicit stepper at 0.9 x its estimated critical step: wall time of advance(steps) after a warm-up advance
    (one synchronisation per call), steps/s and us per step;
  - the same handle's cwf_hip_keff_timed operator time (the apply path: the tile launch and its finalize pass) and the
    ratio step / operator;
  - the bytes the update pass moves per node (80 on a structured block without a load pattern); the pass replaces
    the apply path's finalize pass (44 B per node), so step_us - keff_us is its cost over that pass;
  - simulated seconds per wall second, and the same for the Newmark stepper at the scenario's dt on the same handle
    (newmark-steps steps after one warm-up step).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "civiwave-fem_amd"))

import torch  # noqa: E402

from cwf import _lib, pcg, scenarios  # noqa: E402
from cwf.explicit import ExplicitStepper  # noqa: E402
from cwf.physics import RayleighCoefficients  # noqa: E402
from cwf.stepper import Stepper  # noqa: E402


def measure(key, steps, newmark_steps, device):
    name, _, element = key.partition(":")
    element = element or "tet4"
    L = _lib.load()
    t0 = time.perf_counter()
    case = scenarios.config_case(name, element=element)
    P = case.packing
    out = dict(config=key, name=case.name, nodes=P.node_count, dofs=P.dof_count, elements=P.element_count,
               build_s=time.perf_counter() - t0)
    sysm = pcg.MatrixFreeSystem.from_packing(P, case.materials, 1.0, 0.0, mode=_lib.MODE_FAST, device=device)
    h = sysm.handle()
    out["kernel"] = (L.cwf_hip_system_keff_kernel(h) or b"").decode()
    t0 = time.perf_counter()
    ex = ExplicitStepper(P, case.materials, RayleighCoefficients(0.0, 0.0), system=sysm)
    out["create_s"] = time.perf_counter() - t0  # the 60 power iterations are in here
    tel = ex.telemetry()
    out.update(dt=tel.dt, critical_dt=tel.critical_dt, lambda_max=tel.lambda_max)
    assert ex.advance(200).has_value()
    t0 = time.perf_counter()
    r = ex.advance(steps)
    wall = time.perf_counter() - t0
    assert r.has_value(), r.error()
    assert r.value().finite
    out.update(steps=steps, wall_s=wall, steps_per_s=steps / wall, step_us=1e6 * wall / steps,
               sim_s_per_wall_s=tel.dt * steps / wall)
    ex.close()
    xd = torch.rand(P.dof_count, device=f"cuda:{device}") - 0.5
    yd = torch.zeros_like(xd)
    ms = C.c_double()
    assert L.cwf_hip_keff_timed(h, _lib.ptr(xd), _lib.ptr(yd), 50, C.byref(ms)) == 0
    assert L.cwf_hip_keff_timed(h, _lib.ptr(xd), _lib.ptr(yd), 500, C.byref(ms)) == 0
    out["keff_us"] = 1e3 * ms.value
    out["step_over_keff"] = out["step_us"] / out["keff_us"]
    out["update_bytes_per_node"] = 80
    if newmark_steps > 0 and element == "tet4":
        nm = Stepper(P, case.materials, case.rayleigh, case.cfg.solver, case.cfg.time, system=sysm)
        t = 0.0
        rr = nm.step(t)
        assert rr.has_value(), rr.error()
        t = rr.value().simulation_time + rr.value().time_step
        t0 = time.perf_counter()
        iters = 0
        for _ in range(newmark_steps):
            rr = nm.step(t)
            assert rr.has_value(), rr.error()
            t = rr.value().simulation_time + rr.value().time_step
            iters += rr.value().pcg.iterations
        wall = time.perf_counter() - t0
        nm.close()
        out.update(newmark_dt=case.cfg.time.initial_dt, newmark_step_s=wall / newmark_steps,
                   newmark_iterations_per_step=iters / newmark_steps,
                   newmark_sim_s_per_wall_s=case.cfg.time.initial_dt * newmark_steps / wall)
    sysm.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["c2", "c3", "c2:hex8"])
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--newmark-steps", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "explicit_c2.json"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for key in a.configs:
        line = json.dumps(measure(key, a.steps, a.newmark_steps, a.device))
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
