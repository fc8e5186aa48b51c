#!/usr/bin/env python3
"""Measure the explicit stepper: steps/s next to the operator's own time and to the Newmark stepper.

    python tools/explicit_bench.py [--configs c2 c3 c2:hex8] [--steps 2000] [--newmark-steps 3] [--out FILE]
    python tools/explicit_bench.py --absorbing [--configs c3] [--steps 2000]
    python tools/explicit_bench.py --monitors [--configs c2 c3] [--steps 2000]
    python tools/explicit_bench.py --sources [--configs c2 c3] [--steps 2000]
    python tools/explicit_bench.py --envelopes [--configs c2 c3 c2:hex8] [--steps 2000]
    python tools/explicit_bench.py --ties [--configs c2 c3] [--steps 2000]
    python tools/explicit_bench.py --plasticity [--plain-only] [--repeats 5] [--configs c2 c3] [--steps 2000]
    python tools/explicit_bench.py --soil-plasticity [--repeats 5] [--configs c2 c3] [--steps 2000]

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

--absorbing: the cost of absorbing boundaries instead. Per config one line, appended to
profiles/explicit_absorbing.json: step_us of the stepper without dashpots, with viscous dashpots (cwf.absorbing) on the
five faces of the block other than z = max, and after clear_dashpots again, in one process on one handle; the share
of dashpot nodes and the bytes per node the update pass then moves (84 + 144 x share).

--monitors: the cost of the stepper's monitors. Per config one line, appended to profiles/explicit_monitors.json:
step_us of one stepper on one handle without monitors, with peak maps only, with the ledger only (energy_every 1 and
100), with 64 receivers (every 1 and 10), with everything together, and after clear_monitors again, next to the
estimate from bytes (the update pass's 80 B per node plus what the monitor moves, scaled from the plain step).

--sources: the cost of load sources (include/cwf_hip.h "Load sources"). Per config one line, appended to
profiles/explicit_sources.json, FAST handle, dashpots on the five faces other than z = max throughout: step_us with no
time-varying load, with the vertical incident pattern and curve (the update pass's PATTERN instantiation), with the same
wave as a source on the base, with an oblique plane-wave source on the five faces, with three sources on every node at
zero delay (a three-component record), and after the set is removed; next to the loaded nodes, the entries and the bytes
the source kernel moves by its layout (per loaded node 4 B node + 8 B offsets + 12 B f_ext + 12 B stored, per entry a
32-B record + 8 B curve directory; the curve's knots are shared and stay in L2).

--ties: the cost of tied lateral boundaries (include/cwf_hip.h "Tied boundaries"). Per config one line, appended to
profiles/explicit_ties_c2_c3.json, one stepper on one FAST handle of the unconstrained block: step_us of the plain step,
with the four lateral faces tied by level (one group per node plane), with the two face pairs tied periodically (pairs
and the vertical edges' groups of 4), and after clear_ties again; next to them the groups, members, the largest group,
the set's device bytes and the host time of building and of setting each set.

--envelopes: the cost of the element monitors (include/cwf_hip.h "Element monitors"). Per config one line, appended to
profiles/explicit_envelopes.json, one stepper on one FAST handle: step_us without element monitors, with each envelope
map alone and with all three at envelope_every 1, 10 and 100, with 64 gauges at every 1 and 10, and after
clear_element_monitors again; next to them the time of one element pass (the every-1 step minus the plain step) and
the estimate from bytes at the 6.25 TB/s copy ceiling: per element its record (tet4: 64 B + 4 B material; hex8: 32 B
of corner ids + 96 B of gradients + 4 B), the u gathers counted once per node (12 B x nodes / elements: the rest are
cache hits), and the maps read once and written at most once (4 to 56 B each way).

--plasticity: the cost of J2 plasticity (include/cwf_hip.h "Plasticity"). Per config three lines, appended to
profiles/explicit_plasticity.json, one stepper on one FAST handle: (a) "plain", no plasticity, the step timed
--repeats times (the median, and the spread (max - min) / median, which is what a comparison between two builds of the
library has to exceed); (b) "elastic", every material plastic with a yield stress nothing reaches; (c) "yielding", a
yield stress of 1 Pa, which the block's own weight passes almost everywhere. (b) and (c) carry the time the two
plasticity kernels and the update pass's read of p add over (a), next to the estimate from bytes at the 6.25 TB/s copy
ceiling: per slot the 64-B record, 4 B material, 4 B volume, 4 B slot element, 64 B of state and 16 B of corner positions
read, 48 B of corner forces read by the node pass; per node 12 B of u gathered once (the rest are cache hits), 8 B of
the compact CSR, 12 B of p stored and 12 B read by the update pass; per element that has yielded 48 B of corner forces
and (at most) 64 B of state written. --plain-only: line (a) alone, which a library without the feature can run
(CWF_LIB_PATH: the same-session comparison with the parent commit's build).

--soil-plasticity: the cost of the soil plasticity (include/cwf_hip.h "Soil plasticity"). Per config seven lines, appended
to profiles/explicit_soil_plasticity.json, one stepper on one FAST handle: "plain" as above; "j2_elastic", --plasticity's
(b); "soil_elastic", the soil set without a stress at rest and a cohesion nothing reaches; "soil_rest_elastic", the same
with a geostatic stress; "soil_rest_yielding", a geostatic stress with K0 = 0.2 that lies outside the cone and next to
no cohesion, so that every element yields; and the last two once more with node_pass = 1, the plain node pass in place
of the cooperative one the soil set launches ("..._plain_nodes"). The estimate is --plasticity's, plus 48 B of stress at
rest per slot where there is one.
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


def timed_steps(ex, steps):
    assert ex.advance(200).has_value()
    t0 = time.perf_counter()
    r = ex.advance(steps)
    wall = time.perf_counter() - t0
    assert r.has_value() and r.value().finite, r.error() if not r.has_value() else "non-finite"
    return 1e6 * wall / steps


def measure_absorbing(key, steps, device):
    import numpy as np

    from cwf import absorbing, meshgen

    name, _, element = key.partition(":")
    element = element or "tet4"
    case = scenarios.config_case(name, element=element)
    P, m = case.packing, case.mesh
    X = m.coords
    lo, hi = X.min(0), X.max(0)
    k = m.tets.shape[1]
    faces = []
    for axis, value in ((0, lo[0]), (0, hi[0]), (1, lo[1]), (1, hi[1]), (2, lo[2])):
        on = np.nonzero(X[:, axis] == value)[0]
        sel = np.zeros(P.node_count, bool)
        sel[on] = True
        t = m.tets[sel[m.tets].sum(1) >= (4 if k == 8 else 3)]  # only elements with a face on that plane
        faces.append(meshgen.boundary_faces(t, on))
    t0 = time.perf_counter()
    ids, Cn = absorbing.dashpots(m, case.cfg, np.concatenate(faces))
    out = dict(config=key, name=case.name, nodes=P.node_count, dashpot_nodes=int(ids.size),
               dashpot_share=ids.size / P.node_count, dashpots_s=time.perf_counter() - t0, steps=steps)
    sysm = pcg.MatrixFreeSystem.from_packing(P, case.materials, 1.0, 0.0, mode=_lib.MODE_FAST, device=device)
    out["kernel"] = (_lib.load().cwf_hip_system_keff_kernel(sysm.handle()) or b"").decode()
    ex = ExplicitStepper(P, case.materials, RayleighCoefficients(0.0, 0.0), system=sysm)
    out["dt"] = ex.telemetry().dt
    out["step_us"] = timed_steps(ex, steps)
    ex.set_dashpots(ids, Cn)
    out["step_us_absorbing"] = timed_steps(ex, steps)
    ex.clear_dashpots()
    out["step_us_cleared"] = timed_steps(ex, steps)
    out["absorbing_over_plain"] = out["step_us_absorbing"] / out["step_us"]
    out["update_bytes_per_node"] = 80
    out["update_bytes_per_node_absorbing"] = 84 + 144 * out["dashpot_share"]
    ex.close()
    sysm.close()
    return out


def measure_ties(key, steps, device):
    """--ties: the plain step, the step with the four lateral faces tied by level (a laminar box: one large group per
    node plane) and the step with the two face pairs tied periodically (pairs, and the vertical edges' groups of 4),
    all in one run on one handle. The block is run unconstrained, so that every group has one mask."""
    import dataclasses

    import numpy as np

    from cwf import ties

    name, _, element = key.partition(":")
    case = scenarios.config_case(name, element=element or "tet4")
    P = dataclasses.replace(case.packing, bc_mask=np.zeros_like(case.packing.bc_mask))
    X = case.mesh.coords
    lo, hi = X.min(0), X.max(0)
    face = {(a, e): np.nonzero(X[:, a] == (lo, hi)[e][a])[0] for a in (0, 1) for e in (0, 1)}
    side = np.unique(np.concatenate(list(face.values())))
    t0 = time.perf_counter()
    level = ties.levels(X, side, 2)
    pairs = ties.merge(P.node_count, ties.periodic(X, face[0, 0], face[0, 1], 0), ties.periodic(X, face[1, 0], face[1, 1], 1))
    out = dict(config=key, name=case.name, nodes=P.node_count, steps=steps, tie_sets_s=time.perf_counter() - t0)
    sysm = pcg.MatrixFreeSystem.from_packing(P, case.materials, 1.0, 0.0, mode=_lib.MODE_FAST, device=device)
    out["kernel"] = (_lib.load().cwf_hip_system_keff_kernel(sysm.handle()) or b"").decode()
    ex = ExplicitStepper(P, case.materials, RayleighCoefficients(0.0, 0.0), system=sysm)
    out["dt"] = ex.telemetry().dt
    out["step_us"] = timed_steps(ex, steps)
    for tag, (off, ids) in (("levels", level), ("periodic", pairs)):
        t0 = time.perf_counter()
        ex.set_ties(off, ids)
        out[f"set_ties_s_{tag}"] = time.perf_counter() - t0
        info = ex.tie_info()
        sizes = np.diff(off.astype(np.int64))
        out[f"groups_{tag}"], out[f"members_{tag}"] = info.group_count, info.member_count
        out[f"largest_group_{tag}"], out[f"device_bytes_{tag}"] = int(sizes.max()), info.device_bytes
        out[f"tied_share_{tag}"] = info.member_count / P.node_count
        out[f"step_us_{tag}"] = timed_steps(ex, steps)
        out[f"{tag}_over_plain"] = out[f"step_us_{tag}"] / out["step_us"]
    ex.clear_ties()
    out["step_us_cleared"] = timed_steps(ex, steps)
    ex.close()
    sysm.close()
    return out


def measure_monitors(key, steps, device):
    import numpy as np

    name, _, element = key.partition(":")
    case = scenarios.config_case(name, element=element or "tet4")
    P = case.packing
    N = P.node_count
    sysm = pcg.MatrixFreeSystem.from_packing(P, case.materials, 1.0, 0.0, mode=_lib.MODE_FAST, device=device)
    out = dict(config=key, name=case.name, nodes=N, steps=steps,
               kernel=(_lib.load().cwf_hip_system_keff_kernel(sysm.handle()) or b"").decode())
    ex = ExplicitStepper(P, case.materials, RayleighCoefficients(0.0, 0.0), system=sysm)
    out["dt"] = ex.telemetry().dt
    receivers = np.random.Generator(np.random.PCG64(5)).permutation(N)[:64]
    total = 200 + steps  # timed_steps warms up with 200 steps
    sets = [
        ("plain", None),
        ("peaks", dict(peaks=True)),
        ("ledger_every_1", dict(energy_every=1, energy_capacity=total)),
        ("ledger_every_100", dict(energy_every=100, energy_capacity=total // 100 + 1)),
        ("receivers64_every_1", dict(receivers=receivers, receiver_every=1, receiver_capacity=total)),
        ("receivers64_every_10", dict(receivers=receivers, receiver_every=10, receiver_capacity=total // 10 + 1)),
        ("all", dict(receivers=receivers, receiver_every=1, receiver_capacity=total, peaks=True, energy_every=1,
                     energy_capacity=total)),
        ("cleared", None),
    ]
    for label, kw in sets:
        if kw is None:
            ex.clear_monitors()
        else:
            ex.set_monitors(**kw)
        out["step_us_" + label] = timed_steps(ex, steps)
    # bytes per node of the update pass: 80 plain; peaks at most +24 (three 4-B loads, up to three 4-B stores);
    # the ledger +32 B per 256-node workgroup every step (its two accumulators read and written)
    out["update_bytes_per_node"] = dict(plain=80, peaks=104, ledger=80 + 32 / 256, all=104 + 32 / 256)
    ex.close()
    sysm.close()
    return out


def five_faces(case):
    """The boundary faces of the block other than z = max, and those of z = min alone."""
    import numpy as np

    from cwf import meshgen

    P, m = case.packing, case.mesh
    X = m.coords
    lo, hi = X.min(0), X.max(0)
    k = m.tets.shape[1]
    faces = []
    for axis, value in ((2, lo[2]), (0, lo[0]), (0, hi[0]), (1, lo[1]), (1, hi[1])):
        on = np.nonzero(X[:, axis] == value)[0]
        sel = np.zeros(P.node_count, bool)
        sel[on] = True
        t = m.tets[sel[m.tets].sum(1) >= (4 if k == 8 else 3)]  # only elements with a face on that plane
        faces.append(meshgen.boundary_faces(t, on))
    return np.concatenate(faces), faces[0]


def measure_sources(key, steps, device):
    import math

    import numpy as np

    from cwf import absorbing
    from cwf.explicit import LoadSource

    name, _, element = key.partition(":")
    case = scenarios.config_case(name, element=element or "tet4")
    P, m = case.packing, case.mesh
    N = P.node_count
    faces, base = five_faces(case)
    ids, Cn = absorbing.dashpots(m, case.cfg, faces)
    bid, bC = absorbing.dashpots(m, case.cfg, base)
    sysm = pcg.MatrixFreeSystem.from_packing(P, case.materials, 1.0, 0.0, mode=_lib.MODE_FAST, device=device)
    out = dict(config=key, name=case.name, nodes=N, steps=steps, dashpot_nodes=int(ids.size),
               kernel=(_lib.load().cwf_hip_system_keff_kernel(sysm.handle()) or b"").decode())
    ex = ExplicitStepper(P, case.materials, RayleighCoefficients(0.0, 0.0), system=sysm)
    dt = ex.telemetry().dt
    out["dt"] = dt
    ex.set_dashpots(ids, Cn)
    # a Gaussian velocity pulse over the whole run, 1024 points
    total = 2 * (200 + steps) * dt
    t = np.linspace(0.0, 6.0 * total, 1024)
    curve = list(zip(t, 1e-3 * np.exp(-0.5 * ((t - 0.5 * total) / (0.1 * total)) ** 2)))
    d = np.array([0.0, 0.0, 1.0])
    out["step_us_plain"] = timed_steps(ex, steps)
    pat = ExplicitStepper(P, case.materials, RayleighCoefficients(0.0, 0.0), system=sysm, dt=dt)
    pat.set_dashpots(ids, Cn)
    pat.set_load_pattern(np.zeros(P.dof_count), absorbing.incident_pattern(bid, bC, d, N))
    pat.set_load_curve(curve)
    out["step_us_pattern"] = timed_steps(pat, steps)
    pat.close()
    a = math.radians(30.0)
    khat = np.array([math.sin(a), 0.0, math.cos(a)])
    oid, oA, otau, _ = absorbing.incident_plane_wave(m, case.cfg, faces, khat, khat, m.coords.min(0))
    rec = [LoadSource(curve, np.arange(N, dtype=np.uint32), np.eye(3)[k][None, :] * np.ones((N, 1)), np.zeros(N))
           for k in range(3)]
    sets = [("source_vertical", [LoadSource(curve, bid, 2.0 * (bC @ d), np.zeros(bid.size))]),
            ("source_oblique", [LoadSource(curve, oid, oA, otau)]),
            ("dense_three", rec),
            ("removed", [])]
    for label, srcs in sets:
        ex.set_sources(srcs)
        i = ex.source_info()
        out["step_us_" + label] = timed_steps(ex, steps)
        if srcs:
            out[label] = dict(loaded_nodes=i.loaded_nodes, entries=i.entry_count, device_bytes=i.device_bytes,
                              kernel_bytes_per_step=36 * i.loaded_nodes + 40 * i.entry_count)
    ex.close()
    sysm.close()
    return out


def measure_envelopes(key, steps, device):
    import numpy as np

    name, _, element = key.partition(":")
    case = scenarios.config_case(name, element=element or "tet4")
    P = case.packing
    N, E = P.node_count, P.element_count
    hex8 = (element or "tet4") == "hex8"
    sysm = pcg.MatrixFreeSystem.from_packing(P, case.materials, 1.0, 0.0, mode=_lib.MODE_FAST, device=device)
    out = dict(config=key, name=case.name, nodes=N, elements=E, steps=steps,
               kernel=(_lib.load().cwf_hip_system_keff_kernel(sysm.handle()) or b"").decode())
    ex = ExplicitStepper(P, case.materials, RayleighCoefficients(0.0, 0.0), system=sysm)
    out["dt"] = ex.telemetry().dt
    gauges = np.random.Generator(np.random.PCG64(5)).permutation(E)[:64]
    total = 200 + steps  # timed_steps warms up with 200 steps
    maps = dict(von_mises=dict(von_mises=True), shear_strain=dict(shear_strain=True),
                stress_range=dict(stress_range=True),
                all=dict(von_mises=True, shear_strain=True, stress_range=True))
    out["step_us_plain"] = timed_steps(ex, steps)
    for label, kw in maps.items():
        for every in (1, 10, 100):
            ex.set_element_monitors(envelope_every=every, **kw)
            out[f"step_us_{label}_every_{every}"] = timed_steps(ex, steps)
    for every in (1, 10):
        ex.set_element_monitors(gauges=gauges, gauge_every=every, gauge_capacity=total // every + 1)
        out[f"step_us_gauges64_every_{every}"] = timed_steps(ex, steps)
    ex.clear_element_monitors()
    out["step_us_cleared"] = timed_steps(ex, steps)
    record = (32 + 96 + 4) if hex8 else (64 + 4)
    map_bytes = dict(von_mises=4, shear_strain=4, stress_range=48, all=56)
    ceiling = 6.25e12
    for label, b in map_bytes.items():
        lo, hi = E * (record + b) + 12 * N, E * (record + 2 * b) + 12 * N  # nothing stored .. every value stored
        out[f"pass_{label}"] = dict(measured_us=out[f"step_us_{label}_every_1"] - out["step_us_plain"],
                                    bytes_low=lo, bytes_high=hi, estimate_us_low=1e6 * lo / ceiling,
                                    estimate_us_high=1e6 * hi / ceiling)
    ex.close()
    sysm.close()
    return out


def measure_plasticity(key, steps, device, repeats, plain_only, only=None):
    import statistics

    name, _, element = key.partition(":")
    case = scenarios.config_case(name, element=element or "tet4")
    P = case.packing
    N, E = P.node_count, P.element_count
    sysm = pcg.MatrixFreeSystem.from_packing(P, case.materials, 1.0, 0.0, mode=_lib.MODE_FAST, device=device)
    base = dict(config=key, name=case.name, nodes=N, elements=E, steps=steps, library=_lib.LIB_PATH,
                kernel=(_lib.load().cwf_hip_system_keff_kernel(sysm.handle()) or b"").decode())
    ex = ExplicitStepper(P, case.materials, RayleighCoefficients(0.0, 0.0), system=sysm)
    base["dt"] = ex.telemetry().dt
    runs = [timed_steps(ex, steps) for _ in range(repeats)]
    plain = statistics.median(runs)
    lines = [dict(base, configuration="plain", step_us=plain, step_us_runs=runs,
                  spread=(max(runs) - min(runs)) / plain)]
    ceiling = 6.25e12
    for label, sy in (() if plain_only else (("elastic", 1e30), ("yielding", 1.0))):
        if only and label != only:
            continue
        ex.set_state(ExplicitStepper.DISPLACEMENT, torch.zeros(P.dof_count, device=f"cuda:{device}"))
        ex.set_state(ExplicitStepper.VELOCITY, torch.zeros(P.dof_count, device=f"cuda:{device}"))
        ex.set_plasticity(sy, 0.1 * case.cfg.materials[0].youngs_modulus)
        us = timed_steps(ex, steps)
        i = ex.plasticity_info()
        b = i.plastic_elements * (64 + 4 + 4 + 4 + 64 + 16 + 48) + N * (12 + 8 + 12 + 12)
        hi = b + (48 + 64) * i.yielded_elements  # every yielded element storing its forces and its state every step
        lines.append(dict(base, configuration=label, yield_stress=sy, step_us=us, plastic_elements=i.plastic_elements,
                          affected_nodes=i.affected_nodes, yielded_elements=i.yielded_elements, device_bytes=i.bytes,
                          added_us=us - plain, bytes_low=b, bytes_high=hi, estimate_us_low=1e6 * b / ceiling,
                          estimate_us_high=1e6 * hi / ceiling))
        ex.clear_plasticity()
    ex.close()
    sysm.close()
    return lines


def measure_soil_plasticity(key, steps, device, repeats):
    import statistics

    from cwf import soil

    name, _, element = key.partition(":")
    case = scenarios.config_case(name, element=element or "tet4")
    P = case.packing
    N, E = P.node_count, P.element_count
    sysm = pcg.MatrixFreeSystem.from_packing(P, case.materials, 1.0, 0.0, mode=_lib.MODE_FAST, device=device)
    base = dict(config=key, name=case.name, nodes=N, elements=E, steps=steps, library=_lib.LIB_PATH,
                kernel=(_lib.load().cwf_hip_system_keff_kernel(sysm.handle()) or b"").decode())
    ex = ExplicitStepper(P, case.materials, RayleighCoefficients(0.0, 0.0), system=sysm)
    base["dt"] = ex.telemetry().dt
    runs = [timed_steps(ex, steps) for _ in range(repeats)]
    plain = statistics.median(runs)
    lines = [dict(base, configuration="plain", step_us=plain, step_us_runs=runs,
                  spread=(max(runs) - min(runs)) / plain)]
    ceiling = 6.25e12
    H = 0.1 * case.cfg.materials[0].youngs_modulus
    rest = soil.geostatic_stress(P, case.cfg.materials, k0=0.2)  # K0 = 0.2 lies outside a cone of alpha = 0.05
    configurations = (("j2_elastic", lambda: ex.set_plasticity(1e30, H), False),
                      ("soil_elastic", lambda: ex.set_soil_plasticity(0.05, 1e30, 0.0, H), False),
                      ("soil_rest_elastic", lambda: ex.set_soil_plasticity(0.05, 1e30, 0.0, H, initial_stress=rest), True),
                      ("soil_rest_yielding", lambda: ex.set_soil_plasticity(0.05, 1e-3, 0.0, H, initial_stress=rest), True),
                      # the last two again with the plain node pass: what the choice of the cooperative one rests on
                      ("soil_rest_elastic_plain_nodes",
                       lambda: ex.set_soil_plasticity(0.05, 1e30, 0.0, H, initial_stress=rest, node_pass=1), True),
                      ("soil_rest_yielding_plain_nodes",
                       lambda: ex.set_soil_plasticity(0.05, 1e-3, 0.0, H, initial_stress=rest, node_pass=1), True))
    for label, setter, with_rest in configurations:
        ex.set_state(ExplicitStepper.DISPLACEMENT, torch.zeros(P.dof_count, device=f"cuda:{device}"))
        ex.set_state(ExplicitStepper.VELOCITY, torch.zeros(P.dof_count, device=f"cuda:{device}"))
        setter()
        us = timed_steps(ex, steps)
        i = ex.plasticity_info()
        b = i.plastic_elements * (64 + 4 + 4 + 4 + 64 + 16 + 48 + (48 if with_rest else 0)) + N * (12 + 8 + 12 + 12)
        hi = b + (48 + 64) * i.yielded_elements
        lines.append(dict(base, configuration=label, model=ex.plasticity_model(), step_us=us,
                          plastic_elements=i.plastic_elements, affected_nodes=i.affected_nodes,
                          yielded_elements=i.yielded_elements, device_bytes=i.bytes, added_us=us - plain, bytes_low=b,
                          bytes_high=hi, estimate_us_low=1e6 * b / ceiling, estimate_us_high=1e6 * hi / ceiling))
        ex.clear_plasticity()
    ex.close()
    sysm.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["c2", "c3", "c2:hex8"])
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--newmark-steps", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--absorbing", action="store_true", help="the cost of dashpots on five faces (see above)")
    ap.add_argument("--monitors", action="store_true", help="the cost of the monitors (see above)")
    ap.add_argument("--sources", action="store_true", help="the cost of load sources (see above)")
    ap.add_argument("--ties", action="store_true", help="the cost of tied lateral boundaries: by level and periodic")
    ap.add_argument("--envelopes", action="store_true", help="the cost of the element monitors (see above)")
    ap.add_argument("--plasticity", action="store_true", help="the cost of J2 plasticity (see above)")
    ap.add_argument("--soil-plasticity", action="store_true", help="the cost of the soil plasticity (see above)")
    ap.add_argument("--plain-only", action="store_true", help="--plasticity: the plain step alone")
    ap.add_argument("--repeats", type=int, default=5, help="--plasticity: timings of the plain step")
    ap.add_argument("--only", choices=["elastic", "yielding"], default=None,
                    help="--plasticity: that configuration alone after the plain step (profiler runs)")
    ap.add_argument("--out", default=None, help="default profiles/explicit_c2.json (--envelopes: "
                                                 "profiles/explicit_envelopes.json, --absorbing: "
                                                 "profiles/explicit_absorbing.json, --monitors: "
                                                 "profiles/explicit_monitors.json, --sources: "
                                                 "profiles/explicit_sources.json)")
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "explicit_soil_plasticity.json" if a.soil_plasticity else
                                  "explicit_plasticity.json" if a.plasticity else
                                  "explicit_envelopes.json" if a.envelopes else
                                  "explicit_sources.json" if a.sources else
                                  "explicit_ties_c2_c3.json" if a.ties else
                                  "explicit_monitors.json" if a.monitors else
                                  "explicit_absorbing.json" if a.absorbing else "explicit_c2.json")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if a.configs == ap.get_default("configs") and not a.envelopes:
        a.configs = ["c2", "c3"] if a.monitors or a.sources or a.plasticity or a.soil_plasticity or a.ties else \
            ["c3"] if a.absorbing else a.configs
    for key in a.configs if a.soil_plasticity else []:
        for d in measure_soil_plasticity(key, a.steps, a.device, a.repeats):
            print(json.dumps(d), flush=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(d) + "\n")
    if a.soil_plasticity:
        return
    for key in a.configs if a.plasticity else []:
        for d in measure_plasticity(key, a.steps, a.device, a.repeats, a.plain_only, a.only):
            print(json.dumps(d), flush=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(d) + "\n")
    for key in [] if a.plasticity else a.configs:
        line = json.dumps(measure_envelopes(key, a.steps, a.device) if a.envelopes else
                          measure_sources(key, a.steps, a.device) if a.sources else
                          measure_ties(key, a.steps, a.device) if a.ties else
                          measure_monitors(key, a.steps, a.device) if a.monitors else
                          measure_absorbing(key, a.steps, a.device) if a.absorbing else
                          measure(key, a.steps, a.newmark_steps, a.device))
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
