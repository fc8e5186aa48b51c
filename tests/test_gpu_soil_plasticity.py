"""Drucker-Prager plasticity of the explicit stepper on the GPU (cwf_hip_explicit_set_soil_plasticity,
include/cwf_hip.h "Soil plasticity").

1. The stepper is the scheme: explicit_common.host_scheme with the soil pass of soil_plasticity_common as its p_at
   (numpy float64 in the header's statement order), each y from cwf_hip_apply_keff on a second handle -- u, v, the
   correction force p, ep, abar and wp bit for bit after 1, 2, 3 and 53 steps, on a PARITY handle, a FAST lattice and
   FAST fan groups (jittered, renumbered nodes), undamped and with Rayleigh damping, with and without a stress at
   rest. The cohesion is picked on the host so that in the restatement at least a quarter of the 216 elements return
   to the cone, at least one to the apex and at least one stays elastic; the counts are asserted there first.
2. A cohesion nothing reaches gives the elastic stepper's u and v.
3. Pressure dependence: a column in uniform simple shear whose three layers differ in their stress at rest alone.
4. Neighbours: either setter replaces the other's set and plasticity_model() follows; reset; clear; dashpots, a load
   source and peak maps alongside, against the restatement; the layered lattice kernel stays; every refusal.
5. python -m cwf.run: a scenario with a friction angle and a geostatic block runs under the explicit integrator, writes
   the two cell arrays and the summary line, and is refused under Newmark.

Shapes: the 216-tet, 80-node block of tests/test_gpu_explicit.py (one partial workgroup of slots and of nodes), the
2 x 2 x 6-cell column (144 tets) and the 5 x 4 x 4 two-layer block (480 tets, 240 slots).
"""
import dataclasses
import math

import numpy as np
import pytest

import absorbing_common as ac
import explicit_common as xc
import materials_common as MC
import plasticity_common as pc
import soil_plasticity_common as spc
import sources_common as sc
from cwf import _lib, pcg, scenarios, soil
from cwf.explicit import ExplicitStepper
from cwf.physics import RayleighCoefficients
from explicit_common import (CHECKPOINTS, PF, ROOT, U, V, advance, applier, case_of, mesh_case, new_system, refused,
                             run_cli)
from helpers import assert_bitwise
from plasticity_common import KINDS, VARIANTS

pytestmark = pytest.mark.gpu

ALPHA, BETA, HARDENING = 0.3, 0.1, 1.0e9


def rest_stress(P, scale):
    """A stress at rest that grows with depth below the block's top, [E,6]: sigma_v = -scale x depth / height along z,
    sigma_h = 0.5 sigma_v -- no confinement at the top, `scale` at the bottom."""
    z = soil.centroids(P)[:, 2]
    X = np.asarray(P.position64 if P.position64 is not None else P.position0, np.float64).reshape(-1, 3)
    top, height = X[:, 2].max(), X[:, 2].max() - X[:, 2].min()
    sv = -scale * (top - z) / height
    s = np.zeros((P.element_count, 6))
    s[:, 0], s[:, 1], s[:, 2] = 0.5 * sv, 0.5 * sv, sv
    return s


def elastic_peaks(case, apply, V_, dt, sig0):
    """The elastic host scheme's per-element peaks over u_0 .. u_52: (of the cone's J + 3 alpha pm with the stress at
    rest, of J alone), float64."""
    P = case.packing
    D = P.dof_count
    R = pc.Restatement(P, case.materials, 1.0, 0.0)  # every element a slot: its strain and D
    peak, peak_j = np.full(P.element_count, -np.inf), np.zeros(P.element_count)
    u, v = np.zeros(D, np.float32), np.zeros(D, np.float32)
    for n in range(CHECKPOINTS[-1]):
        st = pc.iso_row_fold(R.D, R.strain(u))
        if sig0 is not None:
            st = sig0 + st
        pm = st[:, :3].sum(1) / 3.0
        J = pc.von_mises(st) / math.sqrt(3.0)
        peak, peak_j = np.maximum(peak, J + 3.0 * ALPHA * pm), np.maximum(peak_j, J)
        u, v, _ = pc.plastic_scheme(P, apply, None, lambda n: P.external_force, V_["alpha"], V_["beta"], dt, u, v, n, 1)
    return peak, peak_j


def restated_run(case, apply, V_, dt, kappa, sig0, upto=CHECKPOINTS):
    """-> ([(steps, u, v, p, (ep, abar, wp))] of the restatement at the checkpoints, the outcomes met per element)."""
    P = case.packing
    D = P.dof_count
    R = spc.SoilRestatement(P, case.materials, ALPHA, kappa, BETA, HARDENING, sig0)
    u, v, done, out = np.zeros(D, np.float32), np.zeros(D, np.float32), 0, []
    for n in upto:
        u, v, p = pc.plastic_scheme(P, apply, R, lambda n: P.external_force, V_["alpha"], V_["beta"], dt, u, v, done,
                                    n - done)
        done = n
        out.append((n, u, v, p, R.full()))
    return out, R.seen


def pick_cohesion(case, apply, V_, dt, sig0_of):
    """The first candidate cohesion (a quantile of the elastic run's positive peaks of J + 3 alpha pm) for which the
    restatement sends at least a quarter of the elements to the cone, at least one to the apex, and leaves at least
    one elastic. -> (kappa, sig0, the restated run, the outcomes per element)."""
    E = case.packing.element_count
    _, peak_j = elastic_peaks(case, apply, V_, dt, None)
    sig0 = sig0_of(float(np.median(peak_j)))
    peak, _ = elastic_peaks(case, apply, V_, dt, sig0)
    assert np.count_nonzero(peak > 0.0) > E // 2
    for quantile in (0.5, 0.35, 0.65, 0.2, 0.8, 0.1):
        kappa = float(np.quantile(peak[peak > 0.0], quantile))
        run, seen = restated_run(case, apply, V_, dt, kappa, sig0)
        cone, apex, quiet = (np.count_nonzero(seen & 1), np.count_nonzero(seen & 2), np.count_nonzero(seen == 0))
        print(f"quantile {quantile}: kappa {kappa:.4e}, cone {cone}, apex {apex}, elastic {quiet} of {E}")
        if 4 * cone >= E and apex >= 1 and quiet >= 1:
            return kappa, sig0, run, seen
    raise AssertionError("no candidate cohesion gives a quarter on the cone, one at the apex and one elastic")


def assert_against(st, u, v, p, state, what):
    assert_bitwise(st.get_state(U), u, what + ": u")
    assert_bitwise(st.get_state(V), v, what + ": v")
    assert_bitwise(st.get_state(PF), p, what + ": p")
    pc.assert_state(st, state, what)


# ---- 1. the stepper is the scheme -----------------------------------------------------------------------------------
@pytest.mark.parametrize("rest", ["no_sig0", "sig0"])
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("kind", list(KINDS))
def test_stepper_is_the_scheme_bit_for_bit(kind, variant, rest):
    V_ = VARIANTS[variant]
    case = case_of(kind)
    P = case.packing
    E = P.element_count
    sys_a, sys_b = new_system(case, kind), new_system(case, kind)
    st = ExplicitStepper(P, case.materials, RayleighCoefficients(V_["alpha"], V_["beta"]), system=sys_a)
    try:
        dt = st.telemetry().dt
        apply = applier(sys_b, P.dof_count)
        sig0_of = (lambda scale: rest_stress(P, scale)) if rest == "sig0" else (lambda scale: None)
        kappa, sig0, ref, seen = pick_cohesion(case, apply, V_, dt, sig0_of)
        st.set_soil_plasticity(ALPHA, kappa, BETA, HARDENING, initial_stress=sig0)
        assert st.plasticity_model() == 2
        info = st.plasticity_info()
        assert (info.plastic_elements, info.affected_nodes, info.yielded_elements) == (E, P.node_count, 0)
        assert info.bytes >= E * (4 + 64 + 48 + (48 if sig0 is not None else 0)) + 12 * P.node_count + 32
        done = 0
        for upto, u, v, p, state in ref:
            assert advance(st, upto - done).steps == upto
            done = upto
            assert_against(st, u, v, p, state, f"{kind}/{variant}/{rest} after {upto} steps")
        assert st.plasticity_info().yielded_elements == np.count_nonzero(ref[-1][4][1] > 0.0)
        assert np.abs(ref[-1][3]).max() > 0.0
    finally:
        st.close()
        sys_a.close()
        sys_b.close()


# ---- 2. never yielding is the elastic stepper -----------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_a_cohesion_nothing_reaches_is_the_elastic_stepper(kind):
    case = case_of(kind)
    P = case.packing
    sys_a, sys_b = new_system(case, kind), new_system(case, kind)
    ray = RayleighCoefficients(5.0, 2e-5)
    plastic, elastic = ExplicitStepper(P, case.materials, ray, system=sys_a), \
        ExplicitStepper(P, case.materials, ray, system=sys_b)
    try:
        plastic.set_soil_plasticity(ALPHA, 1e30, BETA, 0.0, initial_stress=rest_stress(P, 1.0e6))
        advance(plastic, CHECKPOINTS[-1])
        advance(elastic, CHECKPOINTS[-1])
        # array_equal, not bitwise: (f - y) + 0.0 may turn a -0.0 into +0.0
        assert np.array_equal(plastic.get_state(U), elastic.get_state(U))
        assert np.array_equal(plastic.get_state(V), elastic.get_state(V))
        assert np.abs(elastic.get_state(U)).max() > 0.0
        ps = plastic.plasticity()
        assert not ps.plastic_strain.any() and not ps.equivalent_plastic_strain.any() and not ps.plastic_work.any()
        assert plastic.plasticity_info().yielded_elements == 0 and plastic.plasticity_info().plastic_elements == P.element_count
        assert not plastic.get_state(PF).any()
    finally:
        plastic.close()
        elastic.close()
        sys_a.close()
        sys_b.close()


# ---- 3. pressure dependence -----------------------------------------------------------------------------------------
def test_strength_grows_with_the_stress_at_rest():
    """u_x = gamma z on a 2 x 2 x 6-cell column of one material whose nodes are all held but one interior node (the
    stable-step estimate needs a free DOF; what is checked is formed from u_0 in the first step's element pass, before
    any node moves). Perfect plasticity without dilation; the stress at rest is -p0 I with p0 = 0 in the upper third,
    p0 > 0 in the middle third, and in the lower third a p0 that lifts the strength above mu gamma. Then ep_zx =
    gamma - kappa / mu above, gamma - (kappa + 3 alpha p0) / mu in the middle, and nothing yields below. Tolerance
    1e-5 relative, the J2 simple-shear test's: u is stored as f32 (6e-8), times the cancellation in the gradient sums,
    with a decade of margin."""
    case = scenarios.block_case(2, 2, 6, h=0.25)
    P0 = case.packing
    N, E = P0.node_count, P0.element_count
    assert E == 144
    X = case.mesh.coords
    lo, hi = X.min(0), X.max(0)
    interior = np.all((X > lo + 1e-9) & (X < hi - 1e-9), axis=1)
    assert np.count_nonzero(interior) == 5
    mask = np.full(N, 7, np.uint32)
    mask[int(np.flatnonzero(interior)[0])] = 0
    mu = float(np.asarray(case.materials[0].stiffness).reshape(6, 6)[3, 3])
    alpha, kappa, p_mid, p_low = 0.2, 23.0e6, 20.0e6, 100.0e6
    gamma = 2.0 * kappa / mu
    assert kappa + 3.0 * alpha * p_mid < mu * gamma < kappa + 3.0 * alpha * p_low
    u0 = np.zeros((N, 3), np.float32)
    u0[:, 0] = (gamma * X[:, 2]).astype(np.float32)
    u0 = u0.reshape(-1)
    P = dataclasses.replace(P0, bc_mask=mask, bc_value=u0.copy(), external_force=np.zeros_like(P0.external_force))
    z = soil.centroids(P)[:, 2]
    third = (hi[2] - lo[2]) / 3.0
    upper, lower = z > lo[2] + 2.0 * third, z < lo[2] + third
    middle = ~upper & ~lower
    assert np.count_nonzero(upper) == np.count_nonzero(middle) == np.count_nonzero(lower) == 48
    p0 = np.where(upper, 0.0, np.where(middle, p_mid, p_low))
    sig0 = np.zeros((E, 6))
    sig0[:, :3] = -p0[:, None]
    system = pcg.MatrixFreeSystem.from_packing(P, case.materials, 1.0, 0.0, mode=_lib.MODE_PARITY)
    st = ExplicitStepper(P, case.materials, RayleighCoefficients(0.0, 0.0), system=system)
    try:
        st.set_state(U, u0)
        st.set_soil_plasticity(alpha, kappa, 0.0, 0.0, initial_stress=sig0)
        advance(st, 1)
        ps = st.plasticity()
        for name, where, want in (("upper", upper, gamma - kappa / mu),
                                  ("middle", middle, gamma - (kappa + 3.0 * alpha * p_mid) / mu)):
            err = np.abs(ps.plastic_strain[where, 5] - want).max() / want
            print(f"{name} layer: ep_zx relative error {err:.3e}")
            assert err <= 1e-5
            assert np.abs(ps.plastic_strain[where][:, [0, 1, 2, 3, 4]]).max() <= 1e-5 * want
        assert not ps.equivalent_plastic_strain[lower].any() and not ps.plastic_strain[lower].any()
        assert st.plasticity_info().yielded_elements == 96
        # the carried stress sig0 + D (e - ep) is on the cone where the element yielded
        R = spc.SoilRestatement(P, case.materials, alpha, kappa, 0.0, 0.0, sig0)
        sig = ps.stress(R.strain(u0), initial_stress=sig0)
        pm = sig[:, :3].sum(1) / 3.0
        f = pc.von_mises(sig) / math.sqrt(3.0) + 3.0 * alpha * pm - kappa
        assert np.abs(f[~lower]).max() <= 1e-5 * kappa and np.all(f[lower] < 0.0)
    finally:
        st.close()
        system.close()


# ---- 4. neighbours --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["parity", "groups"])
def test_lifecycle_and_neighbours(kind):
    case = case_of(kind)
    P = case.packing
    D, N, E = P.dof_count, P.node_count, P.element_count
    fixed = xc.constrained(P)
    alpha_r = 5.0
    ray = RayleighCoefficients(alpha_r, 0.0)
    sys_a, sys_b, sys_c = (new_system(case, kind) for _ in range(3))
    st, fresh = ExplicitStepper(P, case.materials, ray, system=sys_a), \
        ExplicitStepper(P, case.materials, ray, system=sys_c)
    try:
        dt = st.telemetry().dt
        apply = applier(sys_b, D)
        rng = np.random.Generator(np.random.PCG64(9))
        u0 = (1e-4 * rng.standard_normal(D)).astype(np.float32)  # strains the block well past a small cohesion
        u0[fixed] = P.bc_value[fixed]
        kappa, sig0 = 0.5e6, rest_stress(P, 2.0e6)
        # either setter replaces the other's set, the state starting at zero
        assert st.plasticity_model() == 0
        st.set_plasticity(1.0e6, pc.HARDENING)
        assert st.plasticity_model() == 1
        st.set_state(U, u0)
        advance(st, 2)
        assert st.plasticity_info().yielded_elements > 0
        st.set_soil_plasticity(ALPHA, kappa, BETA, HARDENING, initial_stress=sig0)
        assert st.plasticity_model() == 2
        info = st.plasticity_info()
        assert (info.plastic_elements, info.yielded_elements) == (E, 0) and not st.get_state(PF).any()
        st.set_plasticity(1.0e6, pc.HARDENING)
        assert st.plasticity_model() == 1 and st.plasticity_info().yielded_elements == 0
        # dashpots on the tip face, a one-node source and peak maps alongside the soil set
        tip = case.mesh.node_groups[case.mesh.group_names["TIP"]].astype(np.uint32)
        A = rng.standard_normal((tip.size, 3, 3))
        Cn = 1e5 * (A @ A.transpose(0, 2, 1))
        Pm, Qm = ac.update_matrices(Cn, P.lumped_mass[tip], alpha_r, dt)
        sources = sc.one_node_source(rng, case, dt)
        st.set_dashpots(tip, Cn)
        st.set_sources(sources)
        st.set_monitors(peaks=True)
        st.set_state(U, u0)
        st.set_state(V, np.zeros(D, np.float32))
        first = st.telemetry().steps
        st.set_soil_plasticity(ALPHA, kappa, BETA, HARDENING, initial_stress=sig0)
        advance(st, 10)
        R = spc.SoilRestatement(P, case.materials, ALPHA, kappa, BETA, HARDENING, sig0)
        force_at = lambda n: sc.source_force(P.external_force, sources, n, dt)
        u, v, p = pc.plastic_scheme(P, apply, R, force_at, alpha_r, 0.0, dt, u0, np.zeros(D, np.float32), first, 10,
                                    dash=(tip.astype(np.int64), Pm, Qm))
        assert np.count_nonzero(R.abar > 0.0) > 0
        assert_against(st, u, v, p, R.full(), "combined")
        assert st.peaks()[0].max() > 0.0
        # set_state leaves the plastic state alone; reset zeroes it and keeps the set
        st.set_state(U, np.zeros(D, np.float32))
        st.set_state(V, np.zeros(D, np.float32))
        assert_against(st, np.zeros(D, np.float32), np.zeros(D, np.float32), p, R.full(), "after set_state")
        st.reset_plasticity()
        ps = st.plasticity()
        assert not ps.plastic_strain.any() and not ps.equivalent_plastic_strain.any() and not ps.plastic_work.any()
        assert not st.get_state(PF).any() and st.plasticity_info().yielded_elements == 0
        assert st.plasticity_info().plastic_elements == E and st.plasticity_model() == 2
        # clear: against a stepper that never had plasticity, from the same state
        st.clear_plasticity()
        st.clear_dashpots()
        st.clear_sources()
        st.clear_monitors()
        info = st.plasticity_info()
        assert (info.plastic_elements, info.affected_nodes, info.bytes) == (0, 0, 0) and st.plasticity_model() == 0
        st.set_state(U, u0)
        fresh.set_state(U, u0)
        advance(st, 10)
        advance(fresh, 10)
        assert_bitwise(st.get_state(U), fresh.get_state(U), "cleared: u")
        assert_bitwise(st.get_state(V), fresh.get_state(V), "cleared: v")
    finally:
        st.close()
        fresh.close()
        for s in (sys_a, sys_b, sys_c):
            s.close()


def test_two_layers_only_the_upper_one_plastic_keeps_the_layered_kernel():
    case = scenarios.layered_case(5, 4, 4, [0, 0, 1, 1], materials=scenarios.LAYER_MATERIALS[:2])
    P = case.packing
    mat = np.asarray(P.material_index, np.int64)
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
        inf = float("inf")
        # a cohesion the soft upper soil's elastic response passes within 20 steps under the block's own loads
        probe = pc.Restatement(P, case.materials, [0.0, 1.0], 0.0)
        u, v = np.zeros(P.dof_count, np.float32), np.zeros(P.dof_count, np.float32)
        peak = np.zeros(probe.elem.size)
        for n in range(20):
            peak = np.maximum(peak, pc.von_mises(pc.iso_row_fold(probe.D, probe.strain(u))) / math.sqrt(3.0))
            u, v, _ = pc.plastic_scheme(P, apply, None, lambda n: P.external_force, 0.0, 0.0, dt, u, v, n, 1)
        kappa = 0.5 * float(np.quantile(peak, 0.5))
        assert kappa > 0.0
        st.set_soil_plasticity([0.0, ALPHA], [inf, kappa], [0.0, BETA], [0.0, HARDENING])
        info = st.plasticity_info()
        assert info.plastic_elements == np.count_nonzero(upper) and info.affected_nodes == affected.size
        R = spc.SoilRestatement(P, case.materials, [0.0, ALPHA], [inf, kappa], [0.0, BETA], [0.0, HARDENING])
        assert np.array_equal(R.elem, np.flatnonzero(upper)) and np.array_equal(R.affected, affected)
        advance(st, 20)
        u, v, p = pc.plastic_scheme(P, apply, R, lambda n: P.external_force, 0.0, 0.0, dt,
                                    np.zeros(P.dof_count, np.float32), np.zeros(P.dof_count, np.float32), 0, 20)
        assert R.abar.max() > 0.0
        assert_against(st, u, v, p, R.full(), "layered")
        ps = st.plasticity()
        assert not ps.plastic_strain[~upper].any() and not ps.equivalent_plastic_strain[~upper].any()
        assert (L.cwf_hip_system_keff_kernel(system.handle()) or b"").decode() == kernel
    finally:
        st.close()
        system.close()
        other.close()


def test_refusals_leave_the_previous_set_in_force():
    # a hex8 handle
    hexc = mesh_case(element="hex8")
    hsys = pcg.MatrixFreeSystem.from_packing(hexc.packing, hexc.materials, 1.0, 0.0, mode=_lib.MODE_FAST)
    hst = ExplicitStepper(hexc.packing, hexc.materials, RayleighCoefficients(0.0, 0.0), system=hsys)
    try:
        refused(lambda: hst.set_soil_plasticity(0.2, 1e6), "plasticity needs tet4 elements")
    finally:
        hst.close()
        hsys.close()
    # two materials, the second one anisotropic
    base = mesh_case()
    mixed = MC.MaterialCase(base, [MC.ISO, MC.ROT], MC.scattered(base, 2), name="mixed")
    P = mixed.packing
    E = P.element_count
    msys = pcg.MatrixFreeSystem.from_packing(P, mixed.materials, 1.0, 0.0, mode=_lib.MODE_PARITY)
    mst = ExplicitStepper(P, mixed.materials, RayleighCoefficients(0.0, 0.0), system=msys)
    inf, nan = float("inf"), float("nan")
    first = int(np.flatnonzero(np.asarray(P.material_index) == 0)[0])
    try:
        mst.set_plasticity([2.0e6, inf], [1.0e6, 0.0])  # the set every refusal below has to leave in force
        before = mst.plasticity_info()
        out_of_range = "soil plasticity parameters out of range"
        calls = [
            (lambda: mst.set_soil_plasticity([0.2, 0.2], [1e6, 1e6]), "a plastic material needs an isotropic stiffness",
             ["material=1"]),
            (lambda: mst.set_soil_plasticity([0.2], [1e6]), "plasticity material count mismatch",
             ["material_count=1", "materials=2"]),
            (lambda: mst.set_soil_plasticity([-0.5, 0.2], [1e6, inf]), out_of_range, ["material=0", "alpha=-0.5"]),
            (lambda: mst.set_soil_plasticity([0.2, 0.2], [1e6, -1.0]), out_of_range, ["material=1", "kappa=-1"]),
            (lambda: mst.set_soil_plasticity([0.2, 0.2], [1e6, inf], [0.3, 0.0]), out_of_range, ["material=0"]),
            (lambda: mst.set_soil_plasticity([0.2, 0.2], [1e6, inf], [-0.1, 0.0]), out_of_range, ["material=0"]),
            (lambda: mst.set_soil_plasticity([0.2, 0.2], [1e6, inf], 0.0, [0.0, -2.0]), out_of_range,
             ["material=1", "hardening=-2"]),
            (lambda: mst.set_soil_plasticity([nan, 0.2], [1e6, inf]), out_of_range, ["material=0"]),
            (lambda: mst.set_soil_plasticity([0.2, 0.2], [nan, inf]), out_of_range, ["material=0"]),
            (lambda: mst.set_soil_plasticity([0.2, 0.2], [1e6, inf], [nan, 0.0]), out_of_range, ["material=0"]),
            (lambda: mst.set_soil_plasticity([0.2, 0.2], [1e6, inf], 0.0, [nan, 0.0]), out_of_range, ["material=0"]),
            (lambda: mst.set_soil_plasticity([0.0, 0.2], [0.0, inf]), out_of_range, ["material=0", "alpha=0", "kappa=0"]),
            (lambda: mst.set_soil_plasticity([0.2, 0.2], [1e6, inf], initial_stress=np.zeros((E - 1, 6))),
             "initial stress span size mismatch", [f"span={E - 1}", f"elements={E}"]),
        ]
        bad = np.zeros((E, 6))
        bad[first, 4] = nan
        calls.append((lambda: mst.set_soil_plasticity([0.2, 0.2], [1e6, inf], initial_stress=bad),
                      "initial stress is not finite", [f"element={first}", "component=4"]))
        for call, msg, ctx in calls:
            refused(call, msg, ctx)
            assert mst.plasticity_model() == 1 and mst.plasticity_info() == before, msg
        # a non-finite row of an elastic element is ignored; the anisotropic material stays elastic: accepted
        ok = np.zeros((E, 6))
        ok[int(np.flatnonzero(np.asarray(P.material_index) == 1)[0]), 2] = nan
        mst.set_soil_plasticity([0.2, 0.2], [1e6, inf], initial_stress=ok)
        assert mst.plasticity_model() == 2
        assert mst.plasticity_info().plastic_elements == np.count_nonzero(P.material_index == 0)
        # the ledger and plasticity exclude each other, whichever comes second
        refused(lambda: mst.set_monitors(energy_every=1, energy_capacity=4),
                "the energy ledger and plasticity exclude each other")
        mst.clear_plasticity()
        refused(lambda: mst.plasticity(), "no plasticity is set")
        refused(lambda: mst.get_state(PF), "unknown state field")
        mst.set_monitors(energy_every=1, energy_capacity=4)
        refused(lambda: mst.set_soil_plasticity([0.2, 0.2], [1e6, inf]),
                "the energy ledger and plasticity exclude each other")
        assert mst.plasticity_info().plastic_elements == 0 and mst.plasticity_model() == 0
        # every material elastic removes the set
        mst.clear_monitors()
        mst.set_soil_plasticity([0.2, 0.2], [1e6, inf])
        mst.set_soil_plasticity([0.2, 0.2], [inf, inf])
        assert mst.plasticity_model() == 0
    finally:
        mst.close()
        msys.close()


# ---- 5. the driver --------------------------------------------------------------------------------------------------
def soil_scenario(tmp_path):
    """plasticity_common.plastic_scenario with a cohesion and a friction angle in place of its yield stress,
    and a geostatic stress along z with Jaky's K0."""
    path = pc.plastic_scenario(tmp_path, 100.0)
    text = open(path).read()
    assert text.count("    yield_stress: 100.0\n") == 1
    text = text.replace("    yield_stress: 100.0\n", "    cohesion: 50.0\n    friction_angle: 30.0\n    dilation_angle: 5.0\n")
    text += "\ngeostatic:\n  gravity: 9.81\n  axis: 2\n"
    y = tmp_path / "soil.yaml"
    y.write_text(text)
    return str(y)


def test_run_applies_a_scenarios_soil_model(tmp_path):
    import json
    import os
    import re

    scenario = soil_scenario(tmp_path)
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
    assert names[-2:] == [("plastic_strain", "6"), ("equivalent_plastic_strain", "1")]
    q = run_cli([scenario, "--integrator", "newmark", "--steps", "1"])
    assert q.returncode == 1 and "plastic materials need the explicit integrator" in q.stderr
    # the C++ runner steps by Newmark: the same refusal
    import subprocess

    exe = os.path.join(ROOT, "civiwave-fem_amd", "lib", "cwf_run")
    r = subprocess.run([exe, scenario, "--steps", "1"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode != 0 and "plastic materials need the explicit integrator" in r.stdout + r.stderr


# ---- 6. the two node passes -----------------------------------------------------------------------------------------
def plastic_around(P, nodes):
    """A material index that makes exactly the elements touching `nodes` material 1 (the plastic one)."""
    conn, _ = pc.ec.corners(P)
    return np.isin(conn, nodes).any(axis=1).astype(np.uint32)


def affected_sets(P):
    """Material indices whose plastic elements (material 1) touch exactly 63, 64 and 65 nodes: one short of a
    wavefront, a full one, and one node into the next. Grown from element 0 one element at a time, each adding as many
    new nodes as still fit."""
    conn, _ = pc.ec.corners(P)
    out = {}
    chosen = np.zeros(P.element_count, bool)
    chosen[0] = True
    nodes = set(conn[0].tolist())
    for want in (63, 64, 65):
        while len(nodes) < want:
            new = np.array([len(set(c.tolist()) - nodes) for c in conn])
            new[chosen] = 0
            room = want - len(nodes)
            cand = np.flatnonzero((new >= 1) & (new <= room))
            assert cand.size, (want, len(nodes))
            e = int(cand[np.argmax(new[cand])])
            chosen[e] = True
            nodes |= set(conn[e].tolist())
        assert len(nodes) == want
        out[want] = chosen.astype(np.uint32).copy()
    return out


@pytest.mark.parametrize("shape", ["all", "n4", "n63", "n64", "n65"])
def test_the_cooperative_node_pass_gives_the_plain_ones_p(shape):
    """The jittered, renumbered block (run lengths vary from node to node), every element plastic, and sets whose
    affected nodes number 63, 64 and 65 -- a wavefront short of one lane, full, and one node into the next -- and 4:
    a set of one affected node does not exist, since the four corners of a plastic tet are all affected, so the
    smallest set there is (one tet) stands in for it. Three passes from the same state for 12 steps -- the plain one,
    the cooperative one, and the cooperative one with LDS rounds of 96 words (node_pass 3) -- and p, u, v and the
    plastic state are equal bit for bit. A round of 96 words holds 32 corner entries; the block's 80 nodes have 864
    entries (up to 24 a node), so the first wavefront's span takes more than 20 rounds and the second's several, runs
    begin in one round and end in the next (their sums carried over in the accumulators), and the rounds after the
    first overwrite the LDS share the lanes have just read. The 63-, 64- and 65-node sets take 3 or more rounds."""
    base = case_of("groups")
    P0 = base.packing
    if shape == "all":
        case, P = base, P0
        alpha, kappa, beta, H = ALPHA, 0.5e6, BETA, HARDENING
    else:
        want = int(shape[1:])
        index = affected_sets(P0)[want] if want != 4 else np.eye(1, P0.element_count, 0, dtype=np.uint32)[0]
        case = MC.MaterialCase(base, [MC.ISO, MC.ISO], index, name=shape)
        P = case.packing
        alpha, kappa, beta, H = [0.0, ALPHA], [float("inf"), 0.5e6], [0.0, BETA], [0.0, HARDENING]
    rng = np.random.Generator(np.random.PCG64(17))
    fixed = xc.constrained(P)
    u0 = (1e-4 * rng.standard_normal(P.dof_count)).astype(np.float32)
    u0[fixed] = P.bc_value[fixed]
    sig0 = rest_stress(P, 2.0e6)
    got = {}
    for node_pass in (1, 2, 3):
        system = pcg.MatrixFreeSystem.from_packing(P, case.materials, 1.0, 0.0, mode=_lib.MODE_FAST)
        st = ExplicitStepper(P, case.materials, RayleighCoefficients(5.0, 0.0), system=system)
        try:
            st.set_state(U, u0)
            st.set_soil_plasticity(alpha, kappa, beta, H, initial_stress=sig0, node_pass=node_pass)
            if shape != "all":
                assert st.plasticity_info().affected_nodes == int(shape[1:])
            advance(st, 12)
            ps = st.plasticity()
            got[node_pass] = (st.get_state(PF), st.get_state(U), st.get_state(V), ps.plastic_strain,
                              ps.equivalent_plastic_strain, st.plasticity_info().yielded_elements)
        finally:
            st.close()
            system.close()
    assert got[1][5] > 0 and np.abs(got[1][0]).max() > 0.0
    for other in (2, 3):
        for k, name in ((0, "p"), (1, "u"), (2, "v")):
            assert_bitwise(got[1][k], got[other][k], f"{shape}: {name} of node pass {other}")
        assert np.array_equal(pc.bits64(got[1][3]), pc.bits64(got[other][3])), other
        assert np.array_equal(pc.bits64(got[1][4]), pc.bits64(got[other][4])), other
        assert got[1][5] == got[other][5]
    if shape != "n4":  # more corner words than a short round holds: node pass 3 took several rounds
        plastic = np.ones(P.element_count, bool) if shape == "all" else np.asarray(P.material_index) == 1
        assert 12 * np.count_nonzero(plastic) > 2 * 96
    refused_pass = pcg.MatrixFreeSystem.from_packing(P, case.materials, 1.0, 0.0, mode=_lib.MODE_FAST)
    st = ExplicitStepper(P, case.materials, RayleighCoefficients(5.0, 0.0), system=refused_pass)
    try:
        refused(lambda: st.set_soil_plasticity(alpha, kappa, beta, H, node_pass=4), "unknown node pass", ["node_pass=4"])
    finally:
        st.close()
        refused_pass.close()
