"""J2 plasticity of the explicit stepper on the GPU (cwf_hip_explicit_set_plasticity, include/cwf_hip.h "Plasticity").

1. The stepper is the scheme: explicit_common.host_scheme with the plastic pass of plasticity_common as its p_at
   (numpy float64 in the header's statement order), each y from cwf_hip_apply_keff on a second handle -- u, v, the
   correction force p, ep, abar and wp bit for bit after 1, 2, 3 and 53 steps, on a PARITY handle, a FAST lattice and
   FAST fan groups (jittered, renumbered nodes), undamped and with Rayleigh damping. The yield stress is picked on the
   host so that at least a quarter of the elements have yielded by step 53 and at least one has not.
2. A yield stress nothing reaches gives the elastic stepper's u and v.
3. Uniform simple shear: the closed-form plastic strain, and no net correction force inside a constant stress field.
4. Permanent set: after a one-cycle pulse the damped plastic block keeps a displacement, its elastic twin returns.
5. Two materials, the upper one plastic: counts from the packing, zeros below, the layered lattice kernel still runs.
6. Refusals and lifecycle; dashpots, sources and peak maps alongside, against the restatement.
7. python -m cwf.run: a scenario with a yield_stress runs under the explicit integrator, writes the two cell arrays
   and the summary line, and is refused under Newmark.

Shapes: the 216-tet, 80-node block of tests/test_gpu_explicit.py (one partial workgroup of slots and of nodes); the
5 x 4 x 4 two-layer block (480 tets, 240 slots).
"""
import dataclasses
import json
import math
import os
import re

import numpy as np
import pytest

import absorbing_common as ac
import explicit_common as xc
import materials_common as MC
import plasticity_common as pc
import sources_common as sc
from cwf import _lib, explicit, pcg, scenarios
from cwf.explicit import ExplicitStepper
from cwf.physics import RayleighCoefficients
from explicit_common import (CHECKPOINTS, PF, U, V, YAML, advance, applier, case_of, mesh_case, new_system, refused,
                             run_cli)
from helpers import assert_bitwise
from plasticity_common import HARDENING, KINDS, VARIANTS

pytestmark = pytest.mark.gpu


def elastic_peaks(case, apply, V_, dt):
    """The elastic host scheme's per-element peak von Mises stress of D e over u_0 .. u_52 (float64)."""
    P = case.packing
    D = P.dof_count
    R = pc.Restatement(P, case.materials, 1.0, 0.0)  # every element a slot: its strain and D
    peak = np.zeros(P.element_count)
    u, v = np.zeros(D, np.float32), np.zeros(D, np.float32)
    for n in range(CHECKPOINTS[-1]):
        peak = np.maximum(peak, pc.von_mises(pc.iso_row_fold(R.D, R.strain(u))))
        u, v, _ = pc.plastic_scheme(P, apply, None, lambda n: P.external_force, V_["alpha"], V_["beta"], dt, u, v, n, 1)
    return peak


def restated_run(case, apply, V_, dt, sy, upto=CHECKPOINTS):
    """-> [(steps, u, v, p, (ep, abar, wp))] of the restatement at the checkpoints."""
    P = case.packing
    D = P.dof_count
    R = pc.Restatement(P, case.materials, sy, HARDENING)
    u, v, done, out = np.zeros(D, np.float32), np.zeros(D, np.float32), 0, []
    for n in upto:
        u, v, p = pc.plastic_scheme(P, apply, R, lambda n: P.external_force, V_["alpha"], V_["beta"], dt, u, v, done,
                                    n - done)
        done = n
        out.append((n, u, v, p, R.full()))
    return out


# ---- 1. the stepper is the scheme -----------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("kind", list(KINDS))
def test_stepper_is_the_scheme_bit_for_bit(kind, variant):
    V_ = VARIANTS[variant]
    case = case_of(kind)
    P = case.packing
    E = P.element_count
    sys_a, sys_b = new_system(case, kind), new_system(case, kind)
    st = ExplicitStepper(P, case.materials, RayleighCoefficients(V_["alpha"], V_["beta"]), system=sys_a)
    try:
        dt = st.telemetry().dt
        apply = applier(sys_b, P.dof_count)
        # the yield stress: a quantile of the elastic run's per-element peak von Mises stress, the first candidate for
        # which the restatement has yielded at least a quarter of the elements by step 53 and left at least one elastic
        peaks = elastic_peaks(case, apply, V_, dt)
        ref = None
        for quantile in (0.5, 0.35, 0.65, 0.2):
            sy = float(np.quantile(peaks, quantile))
            run = restated_run(case, apply, V_, dt, sy)
            yielded = np.count_nonzero(run[-1][4][1] > 0.0)
            if sy > 0.0 and 4 * yielded >= E and yielded < E:
                ref = run
                break
        assert ref is not None, "no candidate yield stress yields a quarter of the elements and leaves one elastic"
        st.set_plasticity(sy, HARDENING)
        info = st.plasticity_info()
        assert (info.plastic_elements, info.affected_nodes, info.yielded_elements) == (E, P.node_count, 0)
        assert info.bytes >= E * (4 + 64 + 48) + 12 * P.node_count
        done = 0
        for upto, u, v, p, state in ref:
            assert advance(st, upto - done).steps == upto
            done = upto
            what = f"{kind}/{variant} after {upto} steps"
            assert_bitwise(st.get_state(U), u, what + ": u")
            assert_bitwise(st.get_state(V), v, what + ": v")
            assert_bitwise(st.get_state(PF), p, what + ": p")
            pc.assert_state(st, state, what)
        assert st.plasticity_info().yielded_elements == yielded
        assert np.abs(ref[-1][3]).max() > 0.0
    finally:
        st.close()
        sys_a.close()
        sys_b.close()


# ---- 2. never yielding is the elastic stepper -----------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_a_yield_stress_nothing_reaches_is_the_elastic_stepper(kind):
    case = case_of(kind)
    P = case.packing
    sys_a, sys_b = new_system(case, kind), new_system(case, kind)
    ray = RayleighCoefficients(5.0, 2e-5)
    plastic, elastic = ExplicitStepper(P, case.materials, ray, system=sys_a), \
        ExplicitStepper(P, case.materials, ray, system=sys_b)
    try:
        plastic.set_plasticity(1e30, 0.0)
        advance(plastic, CHECKPOINTS[-1])
        advance(elastic, CHECKPOINTS[-1])
        # array_equal, not bitwise: (f - y) + 0.0 may turn a -0.0 into +0.0
        assert np.array_equal(plastic.get_state(U), elastic.get_state(U))
        assert np.array_equal(plastic.get_state(V), elastic.get_state(V))
        assert np.abs(elastic.get_state(U)).max() > 0.0
        ps = plastic.plasticity()
        assert not ps.plastic_strain.any() and not ps.equivalent_plastic_strain.any() and not ps.plastic_work.any()
        assert plastic.plasticity_info().yielded_elements == 0
        assert not plastic.get_state(PF).any()
    finally:
        plastic.close()
        elastic.close()
        sys_a.close()
        sys_b.close()


# ---- 3. uniform simple shear ----------------------------------------------------------------------------------------
def test_uniform_simple_shear_has_the_closed_form_plastic_strain():
    """u_x = gamma z on a block whose nodes are all held -- but for one interior node, which stays free so that the
    stepper's stable-step estimate has a free DOF to iterate on (a handle without one is refused at create). What is
    checked is formed from u_0 in the first step's element pass, before any node moves. Perfect plasticity with
    gamma = 3 sy / (sqrt(3) mu): the trial stress is 3 sy, the return leaves ep_zx = gamma - sy / (sqrt(3) mu).
    Tolerance 1e-5 relative: u is stored as f32 (6e-8), times the cancellation in the gradient sums on this block,
    with a decade of margin. |p| at interior nodes is at most 1e-5 x the largest corner force: a constant stress has
    no divergence, what remains is the f32 rounding of about 24 corner forces."""
    case = mesh_case()
    P0 = case.packing
    N = P0.node_count
    X = case.mesh.coords
    lo, hi = X.min(0), X.max(0)
    interior = np.all((X > lo + 1e-9) & (X < hi - 1e-9), axis=1)
    assert np.count_nonzero(interior) == 12
    free = int(np.flatnonzero(interior)[0])
    mask = np.full(N, 7, np.uint32)
    mask[free] = 0
    sy = 40.0e6
    mu = float(np.asarray(case.materials[0].stiffness).reshape(6, 6)[3, 3])
    gamma = 3.0 * sy / (math.sqrt(3.0) * mu)
    u0 = np.zeros((N, 3), np.float32)
    u0[:, 0] = (gamma * X[:, 2]).astype(np.float32)
    u0 = u0.reshape(-1)
    P = dataclasses.replace(P0, bc_mask=mask, bc_value=u0.copy(), external_force=np.zeros_like(P0.external_force))
    system = pcg.MatrixFreeSystem.from_packing(P, case.materials, 1.0, 0.0, mode=_lib.MODE_PARITY)
    st = ExplicitStepper(P, case.materials, RayleighCoefficients(0.0, 0.0), system=system)
    try:
        st.set_state(U, u0)
        st.set_plasticity(sy, 0.0)
        advance(st, 1)
        ps = st.plasticity()
        want = gamma - sy / (math.sqrt(3.0) * mu)
        err = np.abs(ps.plastic_strain[:, 5] - want).max() / want
        print(f"ep_zx relative error {err:.3e}")
        assert err <= 1e-5
        others = np.abs(ps.plastic_strain[:, [0, 1, 2, 3, 4]]).max()
        assert others <= 1e-5 * want
        assert st.plasticity_info().yielded_elements == P.element_count
        R = pc.Restatement(P, case.materials, sy, 0.0)
        R.step(u0)
        cmax = float(np.abs(R.corner).max())
        p = st.get_state(PF).reshape(-1, 3)
        inside = np.abs(p[interior]).max()
        print(f"|p| inside {inside:.3e}, largest corner force {cmax:.3e}")
        assert cmax > 0.0 and inside <= 1e-5 * cmax
        assert np.abs(p[~interior]).max() > 0.1 * cmax  # the boundary carries the traction
        # the carried stress D (e - ep) is on the yield surface
        q = pc.von_mises(ps.stress(R.strain(u0)))
        assert np.abs(q - sy).max() <= 1e-5 * sy
    finally:
        st.close()
        system.close()


# ---- 4. permanent set -----------------------------------------------------------------------------------------------
def test_a_pulse_leaves_a_permanent_set():
    """A one-cycle (full sine, zero net impulse) shear pulse on the tip face of the clamped block, mass-proportional
    damping. The elastic twin rings down to below 1 % of its peak tip displacement; the plastic block, whose yield
    stress is 40 % of the twin's peak von Mises stress, keeps more than 10 x the twin's."""
    case = mesh_case()
    P0 = case.packing
    N, D = P0.node_count, P0.dof_count
    tip = case.mesh.node_groups[case.mesh.group_names["TIP"]].astype(np.int64)
    P = dataclasses.replace(P0, external_force=np.zeros_like(P0.external_force))
    pattern = np.zeros((N, 3))
    pattern[tip, 2] = 1.0e6
    pattern = pattern.reshape(-1)
    alpha = 4.0e3
    sys_a, sys_b, sys_c = (new_system(case, "parity") for _ in range(3))
    ray = RayleighCoefficients(alpha, 0.0)
    plastic, twin = ExplicitStepper(P, case.materials, ray, system=sys_a), \
        ExplicitStepper(P, case.materials, ray, system=sys_b)
    try:
        dt = twin.telemetry().dt
        cycle = 40
        curve = [(k * dt, math.sin(2.0 * math.pi * k / cycle)) for k in range(cycle + 1)] + [((cycle + 1) * dt, 0.0)]
        curve[cycle] = (cycle * dt, 0.0)
        for s in (plastic, twin):
            s.set_load_pattern(np.zeros(D), pattern)
            s.set_load_curve(curve)
        twin.set_element_monitors(envelope_every=1, von_mises=True)
        tipz = 3 * tip + 2
        peak, steps, last = 0.0, 0, 0.0
        while steps < 4000:
            advance(twin, 20)
            steps += 20
            last = float(np.abs(twin.get_state(U)[tipz]).max())
            peak = max(peak, last)
            if steps > cycle and last < 0.01 * peak:
                break
        assert steps < 4000 and peak > 0.0
        sy = 0.4 * float(twin.envelopes().von_mises.max())
        # the restatement first: the pulse and the yield stress do what this test needs there
        R = pc.Restatement(P, case.materials, sy, 0.0)
        force_at = xc.curve_force(np.zeros(D), pattern, curve, dt, explicit.curve_value)
        u, v, p = pc.plastic_scheme(P, applier(sys_c, D), R, force_at, alpha, 0.0, dt, np.zeros(D, np.float32),
                                    np.zeros(D, np.float32), 0, steps)
        kept_ref = float(np.abs(u[tipz]).max())
        print(f"{steps} steps: twin peak {peak:.3e}, twin left {last:.3e}, restatement kept {kept_ref:.3e}")
        assert kept_ref > 10.0 * last and R.wp.sum() > 0.0
        plastic.set_plasticity(sy, 0.0)
        advance(plastic, steps)
        kept = float(np.abs(plastic.get_state(U)[tipz]).max())
        print(f"plastic kept {kept:.3e}")
        assert kept > 10.0 * last
        assert_bitwise(plastic.get_state(U), u, "permanent set: u")
        ps = plastic.plasticity()
        assert ps.plastic_work.sum() > 0.0 and np.all(ps.plastic_work >= 0.0)
        assert 0 < plastic.plasticity_info().yielded_elements
    finally:
        plastic.close()
        twin.close()
        for s_ in (sys_a, sys_b, sys_c):
            s_.close()


# ---- 5. mixed materials ---------------------------------------------------------------------------------------------
def test_two_layers_only_the_upper_one_plastic():
    case = scenarios.layered_case(5, 4, 4, [0, 0, 1, 1], materials=scenarios.LAYER_MATERIALS[:2])
    P = case.packing
    mat = np.asarray(P.material_index, np.int64)
    assert set(np.unique(mat)) == {0, 1}
    upper = mat == 1
    conn, _ = pc.ec.corners(P)
    affected = np.unique(conn[upper])
    system = pcg.MatrixFreeSystem.from_packing(P, case.materials, 1.0, 0.0, mode=_lib.MODE_FAST)
    other = pcg.MatrixFreeSystem.from_packing(P, case.materials, 1.0, 0.0, mode=_lib.MODE_FAST)
    L = _lib.load()
    kernel = (L.cwf_hip_system_keff_kernel(system.handle()) or b"").decode()
    assert "k_keff_lattice_layered" in kernel
    st = ExplicitStepper(P, case.materials, RayleighCoefficients(0.0, 0.0), system=system)
    try:
        dt = st.telemetry().dt
        apply = applier(other, P.dof_count)
        # the soft upper soil under the block's own loads: a yield stress its elastic response passes in 20 steps
        sy_of = lambda s: [0.0, s]
        probe = pc.Restatement(P, case.materials, sy_of(1.0), 0.0)
        u, v = np.zeros(P.dof_count, np.float32), np.zeros(P.dof_count, np.float32)
        peak = np.zeros(probe.elem.size)
        for n in range(20):
            peak = np.maximum(peak, pc.von_mises(pc.iso_row_fold(probe.D, probe.strain(u))))
            u, v, _ = pc.plastic_scheme(P, apply, None, lambda n: P.external_force, 0.0, 0.0, dt, u, v, n, 1)
        sy = float(np.quantile(peak, 0.5))
        assert sy > 0.0
        st.set_plasticity(sy_of(sy), [0.0, HARDENING])
        info = st.plasticity_info()
        assert info.plastic_elements == np.count_nonzero(upper) and info.affected_nodes == affected.size
        assert 0 < info.affected_nodes < P.node_count
        R = pc.Restatement(P, case.materials, sy_of(sy), [0.0, HARDENING])
        assert np.array_equal(R.elem, np.flatnonzero(upper)) and np.array_equal(R.affected, affected)
        advance(st, 20)
        u, v, p = pc.plastic_scheme(P, apply, R, lambda n: P.external_force, 0.0, 0.0, dt,
                                    np.zeros(P.dof_count, np.float32), np.zeros(P.dof_count, np.float32), 0, 20)
        assert R.abar.max() > 0.0
        assert_bitwise(st.get_state(U), u, "layered: u")
        assert_bitwise(st.get_state(V), v, "layered: v")
        assert_bitwise(st.get_state(PF), p, "layered: p")
        pc.assert_state(st, R.full(), "layered")
        ps = st.plasticity()
        assert not ps.plastic_strain[~upper].any() and not ps.equivalent_plastic_strain[~upper].any()
        unaffected = np.setdiff1d(np.arange(P.node_count), affected)
        assert not st.get_state(PF).reshape(-1, 3)[unaffected].any()
        assert (L.cwf_hip_system_keff_kernel(system.handle()) or b"").decode() == kernel
    finally:
        st.close()
        system.close()
        other.close()


# ---- 6. refusals and lifecycle --------------------------------------------------------------------------------------
def test_refusals():
    # a hex8 handle
    hexc = mesh_case(element="hex8")
    hsys = pcg.MatrixFreeSystem.from_packing(hexc.packing, hexc.materials, 1.0, 0.0, mode=_lib.MODE_FAST)
    hst = ExplicitStepper(hexc.packing, hexc.materials, RayleighCoefficients(0.0, 0.0), system=hsys)
    try:
        refused(lambda: hst.set_plasticity(1e6), "plasticity needs tet4 elements")
    finally:
        hst.close()
        hsys.close()
    # two materials, the second one anisotropic
    base = mesh_case()
    mixed = MC.MaterialCase(base, [MC.ISO, MC.ROT], MC.scattered(base, 2), name="mixed")
    msys = pcg.MatrixFreeSystem.from_packing(mixed.packing, mixed.materials, 1.0, 0.0, mode=_lib.MODE_PARITY)
    mst = ExplicitStepper(mixed.packing, mixed.materials, RayleighCoefficients(0.0, 0.0), system=msys)
    try:
        refused(lambda: mst.set_plasticity([1e6, 1e6]), "a plastic material needs an isotropic stiffness", ["material=1"])
        refused(lambda: mst.set_plasticity([1e6]), "plasticity material count mismatch",
                ["material_count=1", "materials=2"])
        refused(lambda: mst.set_plasticity([1e6, 0.0, 0.0]), "plasticity material count mismatch")
        refused(lambda: mst.set_plasticity([-1.0, 0.0]), "yield stress and hardening must be non-negative", ["material=0"])
        refused(lambda: mst.set_plasticity([1e6, float("nan")]), "yield stress and hardening must be non-negative",
                ["material=1"])
        refused(lambda: mst.set_plasticity([1e6, 0.0], [float("nan"), 0.0]),
                "yield stress and hardening must be non-negative", ["material=0"])
        refused(lambda: mst.set_plasticity([1e6, 0.0], [0.0, -2.0]), "yield stress and hardening must be non-negative",
                ["material=1"])
        refused(lambda: mst.plasticity(), "no plasticity is set")
        refused(lambda: mst.get_state(PF), "unknown state field")
        mst.set_plasticity([1e6, float("inf")])  # the anisotropic material stays elastic: accepted
        assert mst.plasticity_info().plastic_elements == np.count_nonzero(mixed.packing.material_index == 0)
        # the ledger and plasticity exclude each other, whichever comes second
        refused(lambda: mst.set_monitors(energy_every=1, energy_capacity=4),
                "the energy ledger and plasticity exclude each other")
        mst.set_monitors(peaks=True)  # peak maps are fine
        mst.clear_plasticity()
        mst.set_monitors(energy_every=1, energy_capacity=4)
        refused(lambda: mst.set_plasticity([1e6, 0.0]), "the energy ledger and plasticity exclude each other")
        assert mst.plasticity_info().plastic_elements == 0
    finally:
        mst.close()
        msys.close()


@pytest.mark.parametrize("kind", ["parity", "groups"])
def test_lifecycle_and_neighbours(kind):
    case = case_of(kind)
    P = case.packing
    D, N = P.dof_count, P.node_count
    fixed = xc.constrained(P)
    alpha = 5.0
    ray = RayleighCoefficients(alpha, 0.0)
    sys_a, sys_b, sys_c = (new_system(case, kind) for _ in range(3))
    st, fresh = ExplicitStepper(P, case.materials, ray, system=sys_a), \
        ExplicitStepper(P, case.materials, ray, system=sys_c)
    try:
        dt = st.telemetry().dt
        apply = applier(sys_b, D)
        rng = np.random.Generator(np.random.PCG64(9))
        # a state that strains the block well past a small yield stress
        u0 = (1e-4 * rng.standard_normal(D)).astype(np.float32)
        u0[fixed] = P.bc_value[fixed]
        sy = 1.0e6
        # dashpots on the tip face, a one-node source and peak maps alongside
        tip = case.mesh.node_groups[case.mesh.group_names["TIP"]].astype(np.uint32)
        A = rng.standard_normal((tip.size, 3, 3))
        Cn = 1e5 * (A @ A.transpose(0, 2, 1))
        Pm, Qm = ac.update_matrices(Cn, P.lumped_mass[tip], alpha, dt)
        sources = sc.one_node_source(rng, case, dt)
        st.set_dashpots(tip, Cn)
        st.set_sources(sources)
        st.set_monitors(peaks=True)
        st.set_state(U, u0)
        st.set_plasticity(sy, HARDENING)
        advance(st, 10)
        R = pc.Restatement(P, case.materials, sy, HARDENING)
        force_at = lambda n: sc.source_force(P.external_force, sources, n, dt)
        u, v, p = pc.plastic_scheme(P, apply, R, force_at, alpha, 0.0, dt, u0, np.zeros(D, np.float32), 0, 10,
                                    dash=(tip.astype(np.int64), Pm, Qm))
        assert np.count_nonzero(R.abar > 0.0) > 0
        assert_bitwise(st.get_state(U), u, "combined: u")
        assert_bitwise(st.get_state(V), v, "combined: v")
        assert_bitwise(st.get_state(PF), p, "combined: p")
        pc.assert_state(st, R.full(), "combined")
        assert st.peaks()[0].max() > 0.0
        # set_state leaves the plastic state alone
        st.set_state(U, np.zeros(D, np.float32))
        st.set_state(V, np.zeros(D, np.float32))
        pc.assert_state(st, R.full(), "after set_state")
        # reset zeroes it
        st.reset_plasticity()
        ps = st.plasticity()
        assert not ps.plastic_strain.any() and not ps.equivalent_plastic_strain.any() and not ps.plastic_work.any()
        assert not st.get_state(PF).any() and st.plasticity_info().yielded_elements == 0
        assert st.plasticity_info().plastic_elements == P.element_count
        # clear: today's behaviour, against a stepper that never had plasticity, from the same state
        st.clear_plasticity()
        st.clear_dashpots()
        st.clear_sources()
        st.clear_monitors()
        info = st.plasticity_info()
        assert (info.plastic_elements, info.affected_nodes, info.bytes) == (0, 0, 0)
        st.set_state(U, u0)
        fresh.set_state(U, u0)
        advance(st, 10)
        advance(fresh, 10)
        # the two steppers differ in their step count, so in nothing the plain scheme reads (the force is constant)
        assert_bitwise(st.get_state(U), fresh.get_state(U), "cleared: u")
        assert_bitwise(st.get_state(V), fresh.get_state(V), "cleared: v")
    finally:
        st.close()
        fresh.close()
        for s in (sys_a, sys_b, sys_c):
            s.close()


# ---- 7. the driver --------------------------------------------------------------------------------------------------
def test_run_applies_a_scenarios_yield_stress(tmp_path):
    scenario = pc.plastic_scenario(tmp_path, 100.0)
    out = tmp_path / "out"
    p = run_cli([scenario, "--integrator", "explicit", "--steps", "2", "--out", str(out), "--plastic-summary"])
    assert p.returncode == 0, p.stderr
    lines = [json.loads(l) for l in p.stdout.strip().splitlines()]
    summary = lines[-1]["summary"]
    line = [l["plastic_summary"] for l in lines if "plastic_summary" in l]
    assert len(line) == 1 and line[0]["plastic_elements"] == 216
    assert 0 < line[0]["yielded_elements"] <= 216 and line[0]["plastic_work"] > 0.0
    assert summary["yielded_elements"] == line[0]["yielded_elements"] and summary["plastic_work"] == line[0]["plastic_work"]
    frames = sorted(os.listdir(out / "vtu"))
    assert len(frames) == 2
    raw = open(out / "vtu" / frames[-1], "rb").read()
    head = raw[:raw.index(b"<AppendedData")].decode()
    cells = head[head.index("<CellData"):head.index("</CellData>")]
    names = re.findall(r'Name="([a-z_]+)" NumberOfComponents="(\d)"', cells)
    assert names == [("strain_elem", "6"), ("stress_elem", "6"), ("von_mises_elem", "1"), ("plastic_strain", "6"),
                     ("equivalent_plastic_strain", "1")]
    # the arrays are the stepper's state: the equivalent plastic strain of the last frame, from the appended block
    offs = [int(o) for o in re.findall(r'offset="(\d+)"', cells)]
    blob = raw[raw.index(b"<AppendedData"):]
    blob = blob[blob.index(b"_") + 1:]
    size = int(np.frombuffer(blob[offs[4]:offs[4] + 4], np.uint32)[0])
    abar = np.frombuffer(blob[offs[4] + 4:offs[4] + 4 + size], np.float32)
    assert abar.size == 216 and np.count_nonzero(abar > 0.0) == line[0]["yielded_elements"]
    q = run_cli([scenario, "--integrator", "newmark", "--steps", "1"])
    assert q.returncode == 1 and "plastic materials need the explicit integrator" in q.stderr
    r = run_cli([YAML, "--steps", "1", "--plastic-summary"])
    assert r.returncode == 1 and "belongs to the explicit integrator" in r.stderr
