"""The explicit stepper's element monitors on the GPU (cwf_hip_explicit_set_element_monitors, include/cwf_hip.h
"Element monitors"). The oracle for everything but the shear strain is the project's own pinned cwf_hip_derived_fields:
a second stepper on a second handle of the same case is advanced step by step, and after every step its u goes through
the derived-fields element pass (reference()).

1. Gauge rows are those element records, bit for bit, with their step counts and times.
2. The von Mises and stress min / max envelopes are their running extrema by the stated rule, bit for bit.
3. The shear-strain envelope is the numpy fp64 restatement of the element strain and the header's formula.
4. Independence of the node monitors, reset, replace, capacity, refusals, clear.
5. Kernel names and launch counts, by the profiler on child processes.
6. python -m cwf.run's flags. 7. The soil column: peak shear strain = max |v_inc| / V_s where the pulses do not overlap.

Shapes: 432 tets (two workgroups with a ragged tail) as a PARITY handle, a FAST lattice and, jittered, FAST fan groups
with renumbered nodes; 288 hexes; 216 tets (one partial workgroup); 432 tets of two scattered materials, one of them a
rotated orthotropic one (the general D rows and mat[e]).
"""
import csv
import ctypes as C
import functools
import glob
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import element_monitors_common as ec
import explicit_common as xc
import materials_common as MC
from cwf import _lib, pcg, post, run, scenarios
from cwf.explicit import ExplicitStepper
from cwf.physics import RayleighCoefficients, compute_rayleigh
from explicit_common import ROOT, U, V, YAML, advance, block_scenario, run_cli
from helpers import assert_bitwise

pytestmark = pytest.mark.gpu

STEPS, EXTRA = 53, 5
KINDS = {  # the shared operator kinds on this file's blocks, and two more PARITY cases
    "parity": dict(xc.KINDS["parity"], block=(6, 3, 4)),
    "lattice": dict(xc.KINDS["lattice"], block=(6, 3, 4)),
    "groups": dict(xc.KINDS["groups"], block=(6, 3, 4)),
    "hex8": dict(xc.KINDS["hex8"], block=(8, 6, 6)),
    "small": dict(xc.KINDS["parity"], block=(4, 3, 3)),
    "mixed": dict(xc.KINDS["parity"], block=(6, 3, 4), materials=True),
}
CONFIGS = dict(xc.VARIANTS, curve_bc_state=dict(xc.VARIANTS["curve_bc_state"], state=True))
CASES = [(k, v) for k in ("parity", "lattice", "groups", "hex8") for v in CONFIGS] + \
    [("small", "undamped"), ("mixed", "undamped"), ("mixed", "curve_bc_state")]


@functools.lru_cache(maxsize=None)
def case_of(kind, curve):
    k = KINDS[kind]
    case = scenarios.block_case(*k["block"], h=0.1, jitter=k.get("jitter", False), element=k.get("element", "tet4"),
                                harmonic=5.0 if curve else None)
    if k.get("materials"):
        case = MC.MaterialCase(case, [MC.ISO, MC.ROT], MC.scattered(case, 2), name="mixed")
    return case


def new_system(case, kind):
    return xc.new_system(case, kind, kinds=KINDS)


class Reference:
    """One case's inputs and, for n = 0 .. STEPS + EXTRA, u_n, v_(n-1/2) and the derived-fields element records of u_n."""


@functools.lru_cache(maxsize=None)
def reference(kind, config):
    cfg = CONFIGS[config]
    case = case_of(kind, bool(cfg.get("curve")))
    P = case.packing
    E = P.element_count
    S = Reference()
    S.case, S.kind, S.cfg, S.E = case, kind, cfg, E
    S.alpha, S.beta = cfg["alpha"], cfg["beta"]
    rng = np.random.Generator(np.random.PCG64(5))
    S.bcv, S.u0, S.v0 = xc.seeded_state(P, xc.constrained(P), rng if cfg.get("state") else None)
    S.packing = xc.with_bc(P, S.bcv) if cfg.get("state") else P
    if cfg.get("curve"):
        S.base, S.pattern = case.load_pattern()
        _, S.curve = case.load_curve
    else:
        S.curve = None
    # gauges in a permuted order: the first and the last element and both sides of the workgroup boundary
    want = {0, 1, E - 1, E // 2, 17} | ({254, 255, 256, 257} if E > 257 else {E - 2})
    S.gauges = rng.permutation(np.array(sorted(want), np.int64))
    assert not np.array_equal(S.gauges, np.sort(S.gauges))
    system = new_system(case, kind)
    S.dt = 0.0
    st = stepper_of(S, system)
    try:
        S.dt = st.telemetry().dt
        S.U, S.V, S.F = [st.get_state(U)], [st.get_state(V)], [None]
        for n in range(1, STEPS + EXTRA + 1):
            assert advance(st, 1).steps == n
            S.U.append(st.get_state(U))
            S.V.append(st.get_state(V))
            S.F.append(post.compute_derived_fields(S.packing, system=system, displacement=S.U[-1]).elements)
        assert np.abs(S.F[STEPS][:, 12]).max() > 0.0
    finally:
        st.close()
        system.close()
    return S


def stepper_of(S, system):
    st = ExplicitStepper(S.packing, S.case.materials, RayleighCoefficients(S.alpha, S.beta), system=system, dt=S.dt)
    if S.dt:
        assert st.telemetry().dt == S.dt
    if S.curve is not None:
        st.set_load_pattern(S.base, S.pattern)
        st.set_load_curve(S.curve)
    if S.cfg.get("state"):
        st.set_state(U, S.u0)
        st.set_state(V, S.v0)
    return st


def shear32(S, n):
    """f32 of the header's formula on the fp64 restatement of u_n's element strain; the restatement's strain, stored
    as f32, is the derived-fields strain bit for bit (which checks the restatement, not the device)."""
    e = ec.element_strain64(S.packing, S.U[n])
    assert_bitwise(e.astype(np.float32).reshape(-1), S.F[n][:, 0:6].reshape(-1), f"restated strain of step {n}")
    return ec.effective_shear(e).astype(np.float32)


def envelope_reference(S, first, last, every=1, shear=False):
    """The maps after the updates that make the step counts first + 1 .. last, from the start values."""
    ref = ec.EnvelopeReference(S.E)
    for n in range(first + 1, last + 1):
        if n % every == 0:
            ref.add(S.F[n], shear32(S, n) if shear else None)
    return ref


def check_gauges(S, tr, want_steps, what, gauges=None):
    g = S.gauges if gauges is None else gauges
    assert np.array_equal(tr.steps, np.asarray(list(want_steps), np.uint64)), (what, tr.steps)
    assert np.array_equal(tr.time, tr.steps.astype(np.float64) * S.dt)
    assert tr.rows.shape == (len(tr.steps), g.size, 13)
    for i, n in enumerate(want_steps):
        assert_bitwise(tr.rows[i].reshape(-1), S.F[n][g].reshape(-1), f"{what}: gauge rows of step {n}")


def check_envelopes(env, ref, what, shear_ulp=False):
    """-> the number of shear-strain entries one ulp off (0 when the map is not compared)."""
    assert_bitwise(env.von_mises, ref.von_mises, f"{what}: von Mises")
    assert_bitwise(env.stress_min.reshape(-1), ref.stress_min.reshape(-1), f"{what}: stress min")
    assert_bitwise(env.stress_max.reshape(-1), ref.stress_max.reshape(-1), f"{what}: stress max")
    if not shear_ulp:
        return 0
    off = ec.ulps_apart(env.shear_strain, ref.shear_strain)
    assert off.max() <= 1, (what, np.argwhere(off > 1)[:5], off.max())
    return int(np.count_nonzero(off))


# ---- 1. gauges are the derived fields -------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,config", CASES)
def test_gauges_are_the_derived_fields_bit_for_bit(kind, config):
    S = reference(kind, config)
    system = new_system(S.case, kind)
    every1, every4 = stepper_of(S, system), stepper_of(S, system)
    try:
        every1.set_element_monitors(gauges=S.gauges, gauge_every=1, gauge_capacity=64)
        every4.set_element_monitors(gauges=S.gauges, gauge_every=4, gauge_capacity=64)
        assert advance(every1, STEPS).steps == STEPS
        advance(every4, STEPS)
        check_gauges(S, every1.gauge_traces(), range(1, STEPS + 1), f"{kind}/{config} every 1")
        check_gauges(S, every4.gauge_traces(), range(4, STEPS + 1, 4), f"{kind}/{config} every 4")
        i = every4.element_monitor_info()
        assert (i.gauge_count, i.gauge_every, i.gauge_capacity, i.gauge_samples, i.gauge_dropped) == \
            (S.gauges.size, 4, 64, 13, 0)
        assert (i.envelope_every, i.envelope_samples, i.von_mises, i.shear_strain, i.stress_range) == \
            (0, 0, False, False, False)
        tr = every1.gauge_traces()
        assert np.array_equal(tr.strain, tr.rows[:, :, :6]) and np.array_equal(tr.von_mises, tr.rows[:, :, 12])
        for st in (every1, every4):
            assert_bitwise(st.get_state(U), S.U[STEPS], "u after 53 steps")
            assert_bitwise(st.get_state(V), S.V[STEPS], "v after 53 steps")
    finally:
        every1.close()
        every4.close()
        system.close()


# ---- 2. and 3. envelopes are the running extrema --------------------------------------------------------------------
@pytest.mark.parametrize("kind,config", CASES)
def test_envelopes_are_the_running_extrema(kind, config):
    """von Mises and the stress range bit for bit; the shear strain bit for bit but for entries one f32 ulp off where
    the device's fp64 square root rounds the other way. Measured on an MI355X over all cases: 0 such entries."""
    S = reference(kind, config)
    system = new_system(S.case, kind)
    every1, every5 = stepper_of(S, system), stepper_of(S, system)
    try:
        every1.set_element_monitors(envelope_every=1, von_mises=True, shear_strain=True, stress_range=True)
        every5.set_element_monitors(envelope_every=5, von_mises=True, shear_strain=True, stress_range=True)
        start = ec.EnvelopeReference(S.E)
        check_envelopes(every1.envelopes(), start, "at set")
        assert_bitwise(every1.envelopes().shear_strain, start.shear_strain, "shear strain at set")
        advance(every1, 3)
        off = check_envelopes(every1.envelopes(), envelope_reference(S, 0, 3, shear=True), "after 3 steps", True)
        advance(every1, STEPS - 3)
        advance(every5, STEPS)
        env1 = every1.envelopes()
        off += check_envelopes(env1, envelope_reference(S, 0, STEPS, shear=True), f"{kind}/{config} every 1", True)
        off += check_envelopes(every5.envelopes(), envelope_reference(S, 0, STEPS, 5, shear=True),
                               f"{kind}/{config} every 5", True)
        print(f"{kind}/{config}: shear-strain entries one ulp off the restatement: {off} of {3 * S.E}")
        i = every5.element_monitor_info()
        assert (i.envelope_every, i.envelope_samples, i.von_mises, i.shear_strain, i.stress_range) == \
            (5, 10, True, True, True)
        assert env1.von_mises.max() > 0.0 and env1.shear_strain.max() > 0.0
        assert np.all(env1.stress_min <= env1.stress_max) and np.isfinite(env1.stress_min).all()
        if S.cfg.get("state"):  # both signs of stress occur, so the sign handling of min and max is exercised
            both = ((env1.stress_min < 0.0) & (env1.stress_max > 0.0)).any(1)
            assert both.sum() >= S.E / 10, both.sum()
        for st in (every1, every5):
            assert_bitwise(st.get_state(U), S.U[STEPS], "u with envelopes")
            assert_bitwise(st.get_state(V), S.V[STEPS], "v with envelopes")
    finally:
        every1.close()
        every5.close()
        system.close()


def test_single_maps_and_device_pointers():
    """Each map alone runs the same kernel with the other pointers NULL; the maps can be read into device memory."""
    import torch

    S = reference("parity", "curve_bc_state")
    system = new_system(S.case, "parity")
    sts = [stepper_of(S, system) for _ in range(3)]
    try:
        for st, kw in zip(sts, (dict(von_mises=True), dict(shear_strain=True), dict(stress_range=True))):
            st.set_element_monitors(envelope_every=2, **kw)
            advance(st, 10)
        ref = envelope_reference(S, 0, 10, 2, shear=True)
        vm, sh, rg = (st.envelopes() for st in sts)
        assert vm.shear_strain is None and vm.stress_min is None and sh.von_mises is None and rg.von_mises is None
        assert_bitwise(vm.von_mises, ref.von_mises, "von Mises alone")
        assert ec.ulps_apart(sh.shear_strain, ref.shear_strain).max() <= 1
        assert_bitwise(rg.stress_min.reshape(-1), ref.stress_min.reshape(-1), "stress min alone")
        assert_bitwise(rg.stress_max.reshape(-1), ref.stress_max.reshape(-1), "stress max alone")
        lo = torch.zeros((S.E, 6), dtype=torch.float32, device="cuda")
        hi = torch.zeros((S.E, 6), dtype=torch.float32, device="cuda")
        rc = _lib.load().cwf_hip_explicit_read_envelopes(sts[2]._ex, None, None, _lib.ptr(lo), _lib.ptr(hi), S.E,
                                                         _lib.PTR_DEVICE)
        assert rc == 0, _lib.last_error(system._h)
        assert_bitwise(lo.cpu().numpy().reshape(-1), ref.stress_min.reshape(-1), "stress min into device memory")
        assert_bitwise(hi.cpu().numpy().reshape(-1), ref.stress_max.reshape(-1), "stress max into device memory")
    finally:
        for st in sts:
            st.close()
        system.close()


# ---- 4. independence and lifecycle ----------------------------------------------------------------------------------
def memory_of(system):
    b = C.c_uint64()
    assert _lib.load().cwf_hip_system_memory(system.handle(), C.byref(b)) == 0
    return b.value


@pytest.mark.parametrize("kind", ["parity", "lattice"])
def test_node_and_element_monitors_do_not_touch_each_other(kind):
    S = reference(kind, "undamped")
    system = new_system(S.case, kind)
    plain, node, elem, both = (stepper_of(S, system) for _ in range(4))
    receivers = np.array([5, 0, S.case.packing.node_count - 1])
    node_kw = dict(receivers=receivers, receiver_every=2, receiver_capacity=32, peaks=True, energy_every=3,
                   energy_capacity=32)
    elem_kw = dict(gauges=S.gauges, gauge_every=3, gauge_capacity=32, envelope_every=2, von_mises=True,
                   shear_strain=True, stress_range=True)
    try:
        node.set_monitors(**node_kw)
        elem.set_element_monitors(**elem_kw)
        both.set_element_monitors(**elem_kw)
        both.set_monitors(**node_kw)
        for st in (plain, node, elem, both):
            advance(st, STEPS)
            assert_bitwise(st.get_state(U), S.U[STEPS], "u")
            assert_bitwise(st.get_state(V), S.V[STEPS], "v")
        a, b = node.receiver_traces(), both.receiver_traces()
        assert np.array_equal(a.steps, b.steps) and a.steps.size == 26
        assert_bitwise(a.u.reshape(-1), b.u.reshape(-1), "receiver u")
        assert_bitwise(a.v.reshape(-1), b.v.reshape(-1), "receiver v")
        for x, y in zip(node.peaks(), both.peaks()):
            assert_bitwise(x, y, "peak maps")
        ea, eb = node.energy(), both.energy()
        for name in ("kinetic", "potential", "work", "dissipated"):
            assert np.array_equal(getattr(ea, name).view(np.uint64), getattr(eb, name).view(np.uint64)), name
        ga, gb = elem.gauge_traces(), both.gauge_traces()
        check_gauges(S, ga, range(3, STEPS + 1, 3), f"{kind}: element monitors alone")
        check_gauges(S, gb, range(3, STEPS + 1, 3), f"{kind}: both sets")
        ref = envelope_reference(S, 0, STEPS, 2, shear=True)
        check_envelopes(elem.envelopes(), ref, f"{kind}: element monitors alone", True)
        check_envelopes(both.envelopes(), ref, f"{kind}: both sets", True)
        assert_bitwise(elem.envelopes().shear_strain, both.envelopes().shear_strain, "shear strain, with and without")
        # the node set's calls leave the element set alone, and the reverse
        both.reset_monitors()
        assert both.element_monitor_info().gauge_samples == 17 and both.monitor_info().receiver_samples == 0
        both.clear_monitors()
        check_envelopes(both.envelopes(), ref, f"{kind}: after clear_monitors", True)
        before = node.peaks()
        node.set_element_monitors(**elem_kw)
        node.reset_element_monitors()
        node.clear_element_monitors()
        assert node.monitor_info().receiver_samples == 26
        for x, y in zip(before, node.peaks()):
            assert_bitwise(x, y, "peak maps after the element set came and went")
    finally:
        for st in (plain, node, elem, both):
            st.close()
        system.close()


def refused(call, msg, ctx=()):
    with pytest.raises(RuntimeError) as e:
        call()
    assert msg in str(e.value) and all(f"'{c}'" in str(e.value) for c in ctx), str(e.value)


def raw_refused(system, rc, msg, ctx=()):
    got, lines = _lib.last_error(system._h)
    assert rc != 0 and got == msg and all(c in lines for c in ctx), (rc, got, lines)


@pytest.mark.parametrize("kind", ["parity", "lattice"])
def test_lifecycle_and_refusals(kind):
    S = reference(kind, "curve_bc_state")
    E = S.E
    L = _lib.load()
    system = new_system(S.case, kind)
    bytes0 = memory_of(system)
    st, short = stepper_of(S, system), stepper_of(S, system)
    try:
        assert memory_of(system) == bytes0
        i = st.element_monitor_info()
        assert (i.gauge_count, i.gauge_capacity, i.envelope_every, i.envelope_samples, i.von_mises) == (0, 0, 0, 0, False)
        refused(st.envelopes, "envelope map is not set")
        # capacity 3 with 10 due samples: 3 rows held, 7 dropped, stepping goes on
        short.set_element_monitors(gauges=S.gauges, gauge_every=1, gauge_capacity=3)
        assert advance(short, 10).steps == 10
        check_gauges(S, short.gauge_traces(), range(1, 4), f"{kind}: capacity 3")
        i = short.element_monitor_info()
        assert (i.gauge_samples, i.gauge_dropped) == (3, 7)
        assert_bitwise(short.get_state(U), S.U[10], "u past the full buffer")
        # every refusal, with its message and context; the set in force goes on recording across them
        st.set_element_monitors(gauges=S.gauges, gauge_every=1, gauge_capacity=64, envelope_every=1, von_mises=True,
                                stress_range=True)
        advance(st, 5)
        good = dict(gauges=[3, 4], gauge_every=1, gauge_capacity=8)
        for kw, msg, ctx in (
                (dict(gauges=[3, E]), "gauge element out of range", ["index=1", f"element={E}"]),
                (dict(gauges=[3, 9, 3]), "gauge element listed twice", ["index=2", "element=3"]),
                (dict(gauge_every=0), "gauge_every must be at least 1", []),
                (dict(gauge_capacity=0), "monitor capacity must not be zero", []),
                (dict(von_mises=True), "envelope_maps without envelope_every", []),
                (dict(envelope_every=2), "envelope_every without envelope_maps", [])):
            refused(lambda: st.set_element_monitors(**dict(good, **kw)), msg, ctx)
        ids = np.array([3, 4], np.uint32)
        d = _lib.ExplicitElementMonitorDescC(2, _lib.ptr(ids), 1, 8, 1, 8, 0)
        raw_refused(system, L.cwf_hip_explicit_set_element_monitors(st._ex, C.byref(d)), "unknown envelope map",
                    ["maps=8"])
        d = _lib.ExplicitElementMonitorDescC(2, None, 1, 8, 0, 0, 0)
        raw_refused(system, L.cwf_hip_explicit_set_element_monitors(st._ex, C.byref(d)), "null pointer")
        raw_refused(system, L.cwf_hip_explicit_element_monitor_info(st._ex, None), "null pointer")
        rows = np.zeros((6, S.gauges.size, 13), np.float32)
        raw_refused(system, L.cwf_hip_explicit_read_gauges(st._ex, 0, 6, None, _lib.ptr(rows)),
                    "monitor rows out of range", ["first=0", "count=6", "held=5"])
        raw_refused(system, L.cwf_hip_explicit_read_gauges(st._ex, 6, 0, None, None), "monitor rows out of range")
        buf = np.zeros(6 * (E + 1), np.float32)
        raw_refused(system, L.cwf_hip_explicit_read_envelopes(st._ex, _lib.ptr(buf), None, None, None, E + 1,
                                                              _lib.PTR_HOST),
                    "envelope map span size mismatch", [f"span={E + 1}", f"elements={E}"])
        raw_refused(system, L.cwf_hip_explicit_read_envelopes(st._ex, None, _lib.ptr(buf), None, None, E,
                                                              _lib.PTR_HOST), "envelope map is not set")
        advance(st, 5)
        check_gauges(S, st.gauge_traces(), range(1, 11), f"{kind}: across the refusals")
        env = st.envelopes()
        assert env.shear_strain is None
        check_envelopes(env, envelope_reference(S, 0, 10), f"{kind}: across the refusals")
        # reset: the same set from its start values; then 5 more steps are a fresh set's 5 steps
        advance(st, STEPS - 10)
        st.reset_element_monitors()
        i = st.element_monitor_info()
        assert (i.gauge_samples, i.gauge_dropped, i.envelope_samples, i.gauge_count) == (0, 0, 0, S.gauges.size)
        check_envelopes(st.envelopes(), ec.EnvelopeReference(E), f"{kind}: after the reset")
        advance(st, EXTRA)
        check_gauges(S, st.gauge_traces(), range(STEPS + 1, STEPS + EXTRA + 1), f"{kind}: refilled after the reset")
        check_envelopes(st.envelopes(), envelope_reference(S, STEPS, STEPS + EXTRA), f"{kind}: refilled after the reset")
        # a replacing set starts from the start values and keeps u, v and the step count
        st.set_element_monitors(gauges=S.gauges[:2], gauge_every=2, gauge_capacity=4, envelope_every=1,
                                shear_strain=True, stress_range=True)
        assert st.telemetry().steps == STEPS + EXTRA
        env = st.envelopes()
        assert env.von_mises is None
        start = ec.EnvelopeReference(E)
        assert_bitwise(env.shear_strain, start.shear_strain, "a new set's shear strain")
        assert_bitwise(env.stress_min.reshape(-1), start.stress_min.reshape(-1), "a new set's stress min")
        assert_bitwise(env.stress_max.reshape(-1), start.stress_max.reshape(-1), "a new set's stress max")
        assert st.element_monitor_info().gauge_samples == 0
        assert_bitwise(st.get_state(U), S.U[STEPS + EXTRA], "u after the new set")
        # clear: zeros, nothing readable, and the handle's own memory never moved (the stepper's arena is its own)
        st.clear_element_monitors()
        i = st.element_monitor_info()
        assert (i.gauge_count, i.gauge_every, i.gauge_capacity, i.gauge_samples, i.envelope_every, i.envelope_samples,
                i.von_mises, i.shear_strain, i.stress_range) == (0, 0, 0, 0, 0, 0, False, False, False)
        refused(st.envelopes, "envelope map is not set")
        assert st.gauge_traces().steps.size == 0
        assert memory_of(system) == bytes0
    finally:
        st.close()
        short.close()
        system.close()


# ---- 5. kernel names ------------------------------------------------------------------------------------------------
TRACE_SCRIPT = """
import sys
import numpy as np
from cwf import _lib, pcg, scenarios
from cwf.explicit import ExplicitStepper
from cwf.physics import RayleighCoefficients
case = scenarios.block_case(4, 3, 3, h=0.25)
system = pcg.MatrixFreeSystem.from_packing(case.packing, case.materials, 1.0, 0.0, mode=_lib.MODE_FAST)
st = ExplicitStepper(case.packing, case.materials, RayleighCoefficients(0.0, 0.0), system=system)
if sys.argv[1] == "node":
    st.set_monitors(receivers=[1, 2], receiver_every=1, receiver_capacity=8, peaks=True, energy_every=1,
                    energy_capacity=8)
if sys.argv[1] in ("element", "node"):
    st.set_element_monitors(gauges=[0, 7, 3], gauge_every=3, gauge_capacity=1, envelope_every=2, von_mises=True,
                            shear_strain=True, stress_range=True)
if sys.argv[1] == "node":  # a set that was removed before the steps launches nothing
    st.clear_element_monitors()
r = st.advance(7)
assert r.has_value(), r.error()
st.close()
system.close()
"""


def traced_kernels(tmp_path, which):
    """Kernel name -> launches of a seven-step run, by rocprofv3 --kernel-trace on a child process."""
    tool = shutil.which("rocprofv3") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "rocprofv3")
    out = tmp_path / which
    script = tmp_path / f"{which}.py"
    script.write_text(TRACE_SCRIPT)
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "civiwave-fem_amd"))
    p = subprocess.run([tool, "--kernel-trace", "--stats", "--output-format", "csv", "-d", str(out), "--",
                        sys.executable, str(script), which], capture_output=True, text=True, cwd=ROOT, env=env)
    assert p.returncode == 0, (p.stdout[-1000:], p.stderr[-2000:])
    files = glob.glob(str(out / "**" / "*kernel_trace.csv"), recursive=True)
    assert files, (p.stdout[-1000:], p.stderr[-2000:])
    counts = {}
    for f in files:
        with open(f, newline="") as fh:
            for row in csv.DictReader(fh):
                counts[row["Kernel_Name"]] = counts.get(row["Kernel_Name"], 0) + 1
    return counts


def test_kernel_names_and_launch_counts(tmp_path):
    """Three child processes under the profiler, seven steps each: a plain stepper, one with node monitors whose
    element monitors were set and cleared before its steps, and one with element monitors (envelopes every 2 steps:
    3 passes; gauges every 3 steps into one row: 1 recorded, 1 dropped)."""
    plain, node, element = (traced_kernels(tmp_path, w) for w in ("plain", "node", "element"))
    ours = ("k_explicit_envelope", "k_explicit_gauges")

    def new(counts):
        return {n: c for n, c in counts.items() if any(o in n for o in ours)}

    def updates(counts):
        return {n: c for n, c in counts.items() if "k_explicit_update" in n}

    assert sum(updates(plain).values()) == 7 and len(updates(plain)) == 1
    assert not new(plain) and not new(node), (new(plain), new(node))
    # the node-monitored stepper: its MON update pass, the receivers' gather and the ledger's fold, nothing else new
    theirs = ("k_explicit_update", "k_explicit_record", "k_explicit_energy_fold")
    assert {n for n in node if not any(t in n for t in theirs)} == {n for n in plain if "k_explicit_update" not in n}
    assert sum(updates(node).values()) == 7 and set(updates(node)) != set(updates(plain))
    assert [c for n, c in node.items() if "k_explicit_record" in n] == [7]
    got = new(element)
    print("element-monitored stepper, seven steps:", {n: c for n, c in element.items() if "explicit" in n})
    assert len(got) == 2, got
    assert [c for n, c in got.items() if "k_explicit_envelope" in n] == [3]
    assert [c for n, c in got.items() if "k_explicit_gauges" in n] == [1]
    assert {n for n in element if n not in got} == set(plain)
    assert updates(element) == updates(plain)


# ---- 6. the scenario run --------------------------------------------------------------------------------------------
def test_run_reports_a_gauge_the_mesh_does_not_have(capsys, tmp_path):
    assert run.main([YAML, "--integrator", "explicit", "--steps", "1", "--gauges", "0,5", "--out",
                     str(tmp_path / "refused")]) == 1
    err = capsys.readouterr().err
    assert "gauge element out of range" in err and "element=5" in err
    assert not os.path.exists(tmp_path / "refused" / "monitors")


def test_run_writes_envelopes_and_gauges(tmp_path):
    scenario = block_scenario(tmp_path)
    cfg, m, P, mats = run.load_scenario(scenario)
    E = P.element_count
    assert E == 216
    base = [scenario, "--integrator", "explicit", "--steps", "2", "--trace-every", "1", "--peaks"]
    with_flags, without = tmp_path / "element", tmp_path / "plain"
    p = run_cli([*base, "--out", str(with_flags), "--envelope-every", "2", "--gauges", "0,5", "--gauge-every", "1"])
    assert p.returncode == 0, p.stderr
    q = run_cli([*base, "--out", str(without)])
    assert q.returncode == 0, q.stderr
    summary = json.loads(p.stdout.strip().splitlines()[-1])["summary"]
    total = 2 * summary["steps_per_frame"]
    assert summary["explicit_steps"] == total
    assert summary["envelope_samples"] == total // 2 and summary["gauge_samples"] == total
    plain_summary = json.loads(q.stdout.strip().splitlines()[-1])["summary"]
    assert "envelope_samples" not in plain_summary and "gauge_samples" not in plain_summary
    mon = with_flags / "monitors"
    maps = {n: np.load(mon / f"envelope_{n}.npy") for n in ("von_mises", "shear_strain", "stress_min", "stress_max")}
    assert maps["von_mises"].shape == maps["shear_strain"].shape == (E,)
    assert maps["stress_min"].shape == maps["stress_max"].shape == (E, 6)
    assert all(a.dtype == np.float32 for a in maps.values()) and maps["von_mises"].max() > 0.0
    rows = open(mon / "gauges.csv").read().strip().splitlines()
    assert rows[0].startswith("step,time,element,strain_xx,") and rows[0].endswith(",stress_xz,von_mises")
    assert len(rows) == 1 + 2 * total and len(rows[1].split(",")) == 16
    assert [int(r.split(",")[2]) for r in rows[1:5]] == [0, 5, 0, 5]
    # an equal run through the Python interface: the same maps and the same last gauge rows
    st = ExplicitStepper(P, mats, compute_rayleigh(cfg.damping), cfg.solver, cfg.time)
    try:
        assert st.telemetry().dt == summary["dt"]
        st.set_element_monitors(gauges=[0, 5], gauge_every=1, gauge_capacity=total, envelope_every=2, von_mises=True,
                                shear_strain=True, stress_range=True)
        advance(st, total)
        env, tr = st.envelopes(), st.gauge_traces()
    finally:
        st.close()
        st.system.close()
    for name, a in maps.items():
        assert_bitwise(a.reshape(-1), getattr(env, name).reshape(-1), f"envelope_{name}.npy")
    for g, row in enumerate(rows[-2:]):
        cells = row.split(",")
        assert int(cells[0]) == total and float(cells[1]) == total * summary["dt"]
        assert_bitwise(np.array([float(x) for x in cells[3:]], np.float32), tr.rows[-1, g], f"last gauge row {g}")
    # every file of the run without the new flags is there, byte for byte
    files = sorted(os.path.relpath(os.path.join(d, f), without) for d, _, fs in os.walk(without) for f in fs)
    assert {"probes/probes.csv", "probes/traces.csv", "monitors/peaks.npy", "vtu/frame_00000.vtu"} <= set(files), files
    for rel in files:
        assert open(without / rel, "rb").read() == open(with_flags / rel, "rb").read(), rel
    assert sorted(os.listdir(with_flags / "monitors")) == [
        "envelope_shear_strain.npy", "envelope_stress_max.npy", "envelope_stress_min.npy", "envelope_von_mises.npy",
        "gauges.csv", "peaks.npy"]
    # the Newmark integrator refuses the flags
    r = run_cli([YAML, "--steps", "1", "--envelope-every", "2"])
    assert r.returncode == 1 and "belong to the explicit integrator" in r.stderr


# ---- 7. the soil column ---------------------------------------------------------------------------------------------
def test_soil_column_peak_shear_strain():
    """An S wave fed through the base dashpots of the 48-cell column (test_element_monitors_host decides on it): in
    the elements the reflected pulse reaches only after the up-going one has passed, the peak effective shear strain
    is max |v_inc| / V_s. The tolerance is twice the deviation of the all-float64 dense run's own envelope in those
    elements; the f32 state adds 1e-5. Measured on an MI355X (409 steps), relative to 1.2488e-06:
    fp64 run 4.979e-03, PARITY 4.976e-03, FAST lattice 4.982e-03."""
    case = ec.column_case()
    P = case.packing
    D = P.dof_count
    clear = ec.column_clear_elements(case, ec.COLUMN_NZ)
    assert clear.sum() == 576
    systems = {name: pcg.MatrixFreeSystem.from_packing(P, case.materials, 1.0, 0.0, mode=mode)
               for name, mode in (("PARITY", _lib.MODE_PARITY), ("FAST lattice", _lib.MODE_FAST))}
    try:
        probe = ExplicitStepper(P, case.materials, RayleighCoefficients(0.0, 0.0), system=systems["PARITY"])
        dt = probe.telemetry().dt
        probe.close()
        env64, R = ec.column_envelope_f64(dt)
        target = ec.column_target(R)
        dev64 = float(np.abs(env64[clear] - target).max())
        assert 0.0 < dev64 < 0.05 * target
        steps = R["steps"] + 1
        for name, system in systems.items():
            st = ExplicitStepper(P, case.materials, RayleighCoefficients(0.0, 0.0), system=system, dt=dt)
            try:
                st.set_load_pattern(np.zeros(D), R["pattern"])
                st.set_load_curve(R["pts"])
                st.set_dashpots(R["ids"], R["Cn"])
                st.set_element_monitors(envelope_every=1, shear_strain=True)
                advance(st, steps)
                env = st.envelopes().shear_strain.astype(np.float64)
            finally:
                st.close()
            dev = float(np.abs(env[clear] - target).max())
            print(f"S wave, {name}, {steps} steps: max |v_inc| / V_s = {target:.6e}; peak effective shear strain of "
                  f"the {int(clear.sum())} overlap-free elements, worst deviation: fp64 dense run "
                  f"{dev64 / target:.3e}, device {dev / target:.3e} (relative)")
            assert dev <= 2.0 * dev64, (dev, dev64)
            assert np.abs(env[~clear] - target).max() > 0.5 * target  # under the surface the pulses meet
    finally:
        for s in systems.values():
            s.close()
