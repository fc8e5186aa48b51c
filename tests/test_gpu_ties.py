"""Tied (laminar and periodic) lateral boundaries of the explicit stepper on the GPU (cwf_hip_explicit_set_ties).

1. The stepper is the scheme, bit for bit: explicit_common.host_scheme (the header's arithmetic and summation order, P_G | Q_G
   from cwf_explicit_dashpot_update, y from cwf_hip_apply_keff on a second handle) against ExplicitStepper.advance on a
   PARITY handle and the three FAST operator kinds, undamped, damped, and with a load curve, non-zero constraints and a
   seeded state; the lateral perimeter tied by level, dashpots on the base (the z = 0 level has dashpot members, the
   base's interior nodes are untied dashpot nodes).
2. Group sizes on both sides of the gather kernel's two summation orders and of its lane count, over two workgroups of
   the update pass; one large group next to many pairs.
3. Order of set_dashpots and set_ties, replace, get, clear, refusals, and the projection of v.
4. With J2 plasticity that yields. 5. With load sources.
6. The tied 3-D soil column: the compliant-base conditions without held axes; the untied control loses its planes.
7. The energy ledger on that column: the balance drift within the restatement's, each base node's own C_i.
8. Ties at 0.9 x the untied critical step stay bounded over 2,000 steps.
9. python -m cwf.run --integrator explicit with a ``tied:`` scenario (both entry forms) and ``absorbing:``; the Newmark
   drivers refuse it.
"""
import math

import numpy as np
import pytest

import absorbing_common as ac
import explicit_common as xc
import monitors_common as mc
import sources_common as sc
import ties_common as tc
from cwf import _lib, explicit, pack, pcg, ties
from cwf.explicit import ExplicitStepper, LoadSource
from cwf.physics import RayleighCoefficients
from explicit_common import CHECKPOINTS, KINDS, PF, U, V, VARIANTS, applier, deviation, group, new_system, random_spd
from helpers import assert_bitwise

pytestmark = pytest.mark.gpu


def level_ties(case):
    off, ids = ties.levels(case.mesh.coords, group(case, "SIDE"), 2)
    return off, ids, ties.groups_of(off, ids)


def assert_groups_move_together(st, groups, u_equal, what):
    u, v = st.get_state(U).reshape(-1, 3), st.get_state(V).reshape(-1, 3)
    for members in groups:
        assert np.all(v[members].view(np.uint32) == v[members[0]].view(np.uint32)), f"{what}: v of a group differs"
        if u_equal:
            assert np.all(u[members].view(np.uint32) == u[members[0]].view(np.uint32)), f"{what}: u of a group differs"


def check_scheme(case, kind, variant, tie_set, dash_ids, checkpoints, what, sources=False):
    """ExplicitStepper with random dashpots on dash_ids and the tie set against the restatement, u and v bitwise."""
    off, tids, groups = tie_set
    with xc.SchemeRun(case, kind, variant, seed=11) as S:
        P, st, rng, dt = case.packing, S.st, S.rng, S.dt
        dash = None
        tie_dash = None
        if len(dash_ids):
            ids = rng.permutation(np.asarray(dash_ids, np.int64))
            Cn = random_spd(rng, P.lumped_mass[ids], dt)
            Pm, Qm = ac.update_matrices(Cn, P.lumped_mass[ids], S.alpha, dt)
            st.set_dashpots(ids, Cn)
            dash, tie_dash = (ids, Pm, Qm), (ids, Cn)
        st.set_ties(off, tids)
        info = st.tie_info()
        assert (info.group_count, info.member_count) == (len(groups), tids.size) and info.device_bytes > 0
        tie = (groups,) + tc.group_records(groups, P.lumped_mass, S.alpha, dt, tie_dash)
        S.load()
        if S.curve:
            S.v0 = tc.project(S.v0, groups, P.lumped_mass, S.fixed)
            assert_bitwise(st.get_state(V), S.v0, f"{what}: set_state projects v")
        elif sources:
            f_ext = P.external_force.copy()
            nodes = np.concatenate([groups[0][:5], groups[-1][-3:], [int(np.setdiff1d(np.arange(P.node_count), tids)[0])]])
            pts = [(0.0, 0.0), (2.0 * dt, 1.0), (5.0 * dt, -0.5)]
            src = [LoadSource(pts, nodes, 50.0 * rng.standard_normal((nodes.size, 3)), dt * rng.uniform(0, 2, nodes.size))]
            st.set_sources(src)
            S.force_at = lambda n: sc.source_force(f_ext, src, n, dt)
        S.check(checkpoints, what, dash, tie, lambda at: assert_groups_move_together(st, groups, not S.curve, at))
        # the ties did something: the same scheme without them gives other bits at the tied nodes
        _, v_plain = S.host(S.u0, S.v0, 0, 1, dash)
        _, v_tied = S.host(S.u0, S.v0, 0, 1, dash, tie)
        assert not np.array_equal(v_plain.reshape(-1, 3)[tids], v_tied.reshape(-1, 3)[tids])
        S.check_mask_wins(tids)  # a constrained component of a tied node
        return st.get_state(U), st.get_state(V)


# ---- 1. the stepper is the scheme -----------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("kind", list(KINDS))
def test_stepper_with_ties_is_the_scheme_bit_for_bit(kind, variant):
    k = KINDS[kind]
    case = tc.tie_case(jitter=k.get("jitter", False), element=k.get("element", "tet4"),
                       harmonic=5.0 if VARIANTS[variant].get("curve") else None)
    tie_set = level_ties(case)
    assert [len(g) for g in tie_set[2]] == [14, 14, 14, 14]
    base = group(case, "BASE")
    assert np.intersect1d(base, tie_set[2][0]).size == 14 and np.setdiff1d(base, tie_set[1]).size == 6
    check_scheme(case, kind, variant, tie_set, base, CHECKPOINTS, f"{kind}/{variant}")


# ---- 2. group sizes -------------------------------------------------------------------------------------------------
def sized_ties(node_count, sizes, seed):
    perm = np.random.Generator(np.random.PCG64(seed)).permutation(node_count).astype(np.uint32)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    ids = perm[:int(off[-1])]
    return off, ids, ties.groups_of(off, ids)


@pytest.mark.parametrize("kind", ["parity", "lattice"])
def test_group_sizes_on_both_sides_of_the_summation_orders(kind):
    case = tc.tie_case(7, 6, 6, 0.1, hold_side=False)
    assert case.packing.node_count == 392
    tie_set = sized_ties(392, [2, 3, 8, 9, 63, 64, 65, 130], 5)
    first = check_scheme(case, kind, "undamped", tie_set, group(case, "BASE"), (3,), f"{kind}/sizes")
    again = check_scheme(case, kind, "undamped", tie_set, group(case, "BASE"), (3,), f"{kind}/sizes again")
    assert_bitwise(first[0], again[0], "two runs: u")
    assert_bitwise(first[1], again[1], "two runs: v")


@pytest.mark.parametrize("kind", ["parity", "lattice"])
def test_one_large_group_next_to_many_pairs(kind):
    case = tc.tie_case(12, 10, 9, 0.1, hold_side=False)
    assert case.packing.node_count == 1430
    tie_set = sized_ties(1430, [600] + [2] * 100, 6)
    check_scheme(case, kind, "damped", tie_set, [], (3,), f"{kind}/600+pairs")


# ---- 3. order and lifecycle -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["parity", "lattice"])
def test_order_replace_clear_and_refusals(kind):
    case = tc.tie_case()
    P = case.packing
    D, N = P.dof_count, P.node_count
    fixed = xc.constrained(P)
    mass = np.repeat(P.lumped_mass, 3)
    bcv, f = P.bc_value, P.external_force.copy()
    rng = np.random.Generator(np.random.PCG64(23))
    sys_a, sys_b = new_system(case, kind), new_system(case, kind)
    steppers = [ExplicitStepper(P, case.materials, RayleighCoefficients(5.0, 0.0), system=sys_a) for _ in range(3)]
    st, other, fresh = steppers
    try:
        dt = st.telemetry().dt
        apply = applier(sys_b, D)
        off_a, ids_a, groups_a = level_ties(case)
        side = group(case, "SIDE")
        off_b, ids_b, groups_b = sized_ties(side.size, [3, 5, 9], 3)
        ids_b = side[ids_b].astype(np.uint32)  # perimeter nodes only: one mask
        groups_b = ties.groups_of(off_b, ids_b)
        base = rng.permutation(group(case, "BASE"))
        Cn = random_spd(rng, P.lumped_mass[base], dt)
        # No coupling between y, which the base's perimeter nodes hold, and x or z: while such a node is an untied
        # dashpot node (under B, and after the clear) its rows would otherwise read the operator's constrained row,
        # which the FAST fold and cwf_hip_apply_keff leave different (an untied dashpot node is not this test's subject)
        Cn[:, 0, 1] = Cn[:, 1, 0] = Cn[:, 1, 2] = Cn[:, 2, 1] = 0.0
        dash = (base,) + ac.update_matrices(Cn, P.lumped_mass[base], 5.0, dt)

        def host(u, v, first, steps, groups, with_dash=True):
            tie = None
            if groups is not None:
                tie = (groups,) + tc.group_records(groups, P.lumped_mass, 5.0, dt, (base, Cn) if with_dash else None)
            return xc.host_scheme(apply, mass, fixed, bcv, lambda n: f, 5.0, 0.0, dt, u, v, first, steps,
                                  dash if with_dash else None, tie)

        # either order of the two sets: the same bits
        st.set_dashpots(base, Cn)
        st.set_ties(off_a, ids_a)
        other.set_ties(off_a, ids_a)
        other.set_dashpots(base, Cn)
        assert st.tie_info() == other.tie_info() and st.tie_info().dashed_groups == 1
        got_off, got_ids = st.get_ties()
        assert np.array_equal(got_off, off_a) and np.array_equal(got_ids, ids_a)
        assert st.advance(5).has_value() and other.advance(5).has_value()
        u, v = host(np.zeros(D, np.float32), np.zeros(D, np.float32), 0, 5, groups_a)
        for s, name in ((st, "dashpots then ties"), (other, "ties then dashpots")):
            assert_bitwise(s.get_state(U), u, f"{name}: u")
            assert_bitwise(s.get_state(V), v, f"{name}: v")
        # replace A by B: u and the step count kept, v projected onto B's groups
        st.set_ties(off_b, ids_b)
        assert st.telemetry().steps == 5
        assert_bitwise(st.get_state(U), u, "after the replacement: u")
        v = tc.project(v, groups_b, P.lumped_mass, fixed)
        assert_bitwise(st.get_state(V), v, "after the replacement: v projected")
        # refusals: each leaves B in force
        mixed = np.array([side[0], np.setdiff1d(np.arange(N), side)[0]], np.uint32)  # masks 2 and 0
        step = 5
        for bad_off, bad_ids, msg, ctx in (
                ([0, 2], [3, N], "tied node out of range", ["index=1", f"node={N}"]),
                ([0, 2, 4], [side[0], side[1], side[2], side[0]], "tied node listed twice", ["index=3"]),
                ([0, 2, 3], [side[0], side[1], side[2]], "tie group needs at least two nodes", ["group=1", "nodes=1"]),
                ([0, 3, 2], [side[0], side[1], side[2]], "tie offsets must ascend from 0", ["group=1"]),
                ([1, 3], [side[0], side[1], side[2]], "tie offsets must ascend from 0", ["group=0"]),
                ([0, 2], mixed, "tied nodes differ in their constraints",
                 ["group=0", f"node={mixed[1]}", "mask=0", "first_mask=2"])):
            with pytest.raises(RuntimeError) as e:
                st._check(_lib.load().cwf_hip_explicit_set_ties(
                    st._ex, len(bad_off) - 1, _lib.ptr(np.array(bad_off, np.uint64)), _lib.ptr(np.array(bad_ids, np.uint32))))
            assert msg in str(e.value) and all(f"'{c}'" in str(e.value) for c in ctx), str(e.value)
            got_off, got_ids = st.get_ties()
            assert np.array_equal(got_off, off_b) and np.array_equal(got_ids, ids_b)
            assert st.advance(1).has_value()  # B is still in force: the bits of the following step
            u, v = host(u, v, step, 1, groups_b)
            step += 1
            assert_bitwise(st.get_state(U), u, f"B after '{msg}': u")
            assert_bitwise(st.get_state(V), v, f"B after '{msg}': v")
        # a group's C_G refused through set_dashpots while ties are in force: the dashpots and the ties stay
        with pytest.raises(RuntimeError) as e:
            st.set_dashpots(base[:1], np.full((1, 3, 3), np.nan))
        assert "dashpot matrix is not finite" in str(e.value)
        assert np.array_equal(st.get_dashpots()[0], base.astype(np.uint32))
        assert st.advance(1).has_value()
        u, v = host(u, v, step, 1, groups_b)
        step += 1
        assert_bitwise(st.get_state(U), u, "B after the refusals: u")
        assert_bitwise(st.get_state(V), v, "B after the refusals: v")
        # set_state(V) projects
        v_in = (1e-3 * rng.standard_normal(D)).astype(np.float32)
        v_in[fixed] = 0.0
        st.set_state(V, v_in)
        v = tc.project(v_in, groups_b, P.lumped_mass, fixed)
        assert_bitwise(st.get_state(V), v, "set_state(V): projected")
        assert st.advance(2).has_value()
        u, v = host(u, v, step, 2, groups_b)
        step += 2
        assert_bitwise(st.get_state(U), u, "after set_state: u")
        # cleared: the next steps are a never-tied stepper's from the same state
        st.clear_ties()
        assert st.tie_info().group_count == 0 and st.get_ties()[1].size == 0
        fresh.set_dashpots(base, Cn)
        fresh.set_state(U, st.get_state(U))
        fresh.set_state(V, st.get_state(V))
        assert st.advance(3).has_value() and fresh.advance(3).has_value()
        assert_bitwise(st.get_state(U), fresh.get_state(U), "cleared: u")
        assert_bitwise(st.get_state(V), fresh.get_state(V), "cleared: v")
        u, v = host(u, v, step, 3, None)
        assert_bitwise(st.get_state(U), u, "cleared, against the scheme: u")
        assert_bitwise(st.get_state(V), v, "cleared, against the scheme: v")
    finally:
        for s in steppers:
            s.close()
        sys_a.close()
        sys_b.close()


# ---- 4. with plasticity ---------------------------------------------------------------------------------------------
def test_ties_with_yielding_plasticity_take_the_correction_force():
    case = tc.tie_case()
    P = case.packing
    D = P.dof_count
    fixed = xc.constrained(P)
    mass = np.repeat(P.lumped_mass, 3)
    sy = 40.0e6
    mu = float(np.asarray(case.materials[0].stiffness).reshape(6, 6)[3, 3])
    gamma = 3.0 * sy / (math.sqrt(3.0) * mu)
    u0 = np.zeros((P.node_count, 3), np.float32)
    u0[:, 0] = (gamma * case.mesh.coords[:, 2]).astype(np.float32)
    u0 = u0.reshape(-1)
    off, tids, groups = level_ties(case)
    sys_a, sys_b = new_system(case, "parity"), new_system(case, "parity")
    st = ExplicitStepper(P, case.materials, RayleighCoefficients(0.0, 0.0), system=sys_a)
    try:
        dt = st.telemetry().dt
        st.set_state(U, u0)
        st.set_plasticity(sy, 0.0)
        st.set_ties(off, tids)
        tie = (groups,) + tc.group_records(groups, P.lumped_mass, 0.0, dt)
        apply = applier(sys_b, D)
        f = P.external_force.copy()
        u, v = u0, np.zeros(D, np.float32)
        for n in range(3):
            assert st.advance(1).has_value()
            p = st.get_state(PF)
            assert np.abs(p.reshape(-1, 3)[tids]).max() > 0.0
            u, v = xc.host_scheme(apply, mass, fixed, P.bc_value, lambda k: f, 0.0, 0.0, dt, u, v, n, 1, None, tie,
                                  lambda k, u_k: p)
            assert_bitwise(st.get_state(U), u, f"plastic step {n}: u")
            assert_bitwise(st.get_state(V), v, f"plastic step {n}: v")
        assert st.plasticity_info().yielded_elements > 0
    finally:
        st.close()
        sys_a.close()
        sys_b.close()


# ---- 5. with load sources (the load pattern is variant curve_bc_state of 1) -----------------------------------------
@pytest.mark.parametrize("kind", ["parity", "lattice"])
def test_ties_see_the_load_sources_force(kind):
    case = tc.tie_case()
    check_scheme(case, kind, "undamped", level_ties(case), group(case, "BASE"), (3,), f"{kind}/sources", sources=True)


# ---- 6. the tied 3-D column -----------------------------------------------------------------------------------------
def test_tied_column_doubles_at_the_surface_and_absorbs():
    """The figures are in DESIGN section 3, "Tied boundaries"."""
    R = tc.column_reference()
    case = tc.column3d_case()
    P = case.packing
    D = P.dof_count
    dt, steps = R["dt"], R["steps"]
    print(f"fp64 reduced run ({steps} steps, dt {dt:.4e}): {R['conditions']}; untied control spread / peak "
          f"{R['control_spread']:.3e}; restatement floors u {R['floor_u']:.2e} v {R['floor_v']:.2e}")
    R["assert_conditions"]()
    top = 3 * group(case, "TOP")
    sys_p = pcg.MatrixFreeSystem.from_packing(P, case.materials, 1.0, 0.0, mode=_lib.MODE_PARITY)
    sys_b = pcg.MatrixFreeSystem.from_packing(P, case.materials, 1.0, 0.0, mode=_lib.MODE_PARITY)
    apply = applier(sys_b, D)
    mass = np.repeat(P.lumped_mass.astype(np.float64), 3)

    def gpu_run(tied):
        st = ExplicitStepper(P, case.materials, RayleighCoefficients(0.0, 0.0), system=sys_p, dt=dt)
        try:
            st.set_load_pattern(np.zeros(D), R["pattern"])
            st.set_load_curve(R["pts"])
            st.set_dashpots(R["ids"], R["Cn"])
            if tied:
                st.set_ties(*R["ties"])
            states = [(st.get_state(U), st.get_state(V))]
            for _ in range(steps + 1):
                r = st.advance(1)
                assert r.has_value() and r.value().finite
                states.append((st.get_state(U), st.get_state(V)))
        finally:
            st.close()
        return states

    try:
        states = gpu_run(True)
        E = np.array([ac.energy(apply(states[n][0]), mass, states[n][0], states[n][1], states[n + 1][1])
                      for n in range(steps + 1)])
        top_v = np.array([s[1][top].astype(np.float64).mean() for s in states])
        doubling, left = float(np.abs(top_v).max()) / 1e-3, float(E[-1] / E.max())
        du = deviation(states[steps][0], R["u_end"])
        dv = deviation(states[steps][1], R["v_end"])
        print(f"GPU tied column: peak top velocity / incident peak {doubling:.4f}, energy end / peak {left:.2e}; "
              f"deviation from the fp64 reduced run at the end u {du:.2e} v {dv:.2e} "
              f"(bounds {8 * R['floor_u']:.2e} {8 * R['floor_v']:.2e})")
        assert abs(doubling - 2.0) <= 0.02 * 2.0 and left <= 1e-3
        control = gpu_run(False)
        npk = R["npk"]
        ux = control[npk][0][top].astype(np.float64)
        spread = float(ux.max() - ux.min()) / float(np.abs(R["top_u_peak"]))
        tied_ux = states[npk][0][top]
        print(f"GPU untied control: spread of u_x across the top plane at step {npk} / peak {spread:.3e}")
        assert spread >= 0.5 * R["control_spread"]
        assert np.all(tied_ux.view(np.uint32) == tied_ux.view(np.uint32)[0])
        assert du <= 8.0 * R["floor_u"] and dv <= 8.0 * R["floor_v"], (du, dv, R["floor_u"], R["floor_v"])
    finally:
        sys_p.close()
        sys_b.close()


# ---- 8. the step limit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["parity", "lattice"])
def test_ties_leave_the_step_limit_alone(kind):
    case = tc.tie_case(hold_side=False)
    P = case.packing
    D = P.dof_count
    mass = np.repeat(P.lumped_mass.astype(np.float64), 3)
    off, tids, groups = level_ties(case)
    rng = np.random.Generator(np.random.PCG64(9))
    u0 = (1e-6 * rng.standard_normal(D)).astype(np.float32)
    sys_a, sys_b = new_system(case, kind), new_system(case, "parity")
    st = ExplicitStepper(P, case.materials, RayleighCoefficients(0.0, 0.0), system=sys_a)
    try:
        before = st.telemetry()
        st.set_ties(off, tids)
        tel = st.telemetry()
        assert (tel.dt, tel.critical_dt, tel.lambda_max) == (before.dt, before.critical_dt, before.lambda_max)
        assert tel.dt == 0.9 * tel.critical_dt
        apply = applier(sys_b, D)
        st.set_external_force(np.zeros(D, np.float32))
        st.set_state(U, u0)

        def energy_now():
            a = (st.get_state(U), st.get_state(V))
            assert st.advance(1).has_value()
            return ac.energy(apply(a[0]), mass, a[0], a[1], st.get_state(V))

        E0 = energy_now()
        ratios, done = [], 1
        for upto in range(200, 2001, 200):
            r = st.advance(upto - 1 - done)
            assert r.has_value() and r.value().finite
            ratios.append(energy_now() / E0)
            done = upto
        print(f"tied step limit {kind}: energy / initial at ten checkpoints {np.array2string(np.array(ratios), precision=3)}")
        assert st.telemetry().steps == 2000 and max(ratios) <= 4.0 and min(ratios) > 0.0
    finally:
        st.close()
        sys_a.close()
        sys_b.close()


# ---- 7. the energy ledger on the tied column ------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode", [("PARITY", _lib.MODE_PARITY), ("FAST lattice", _lib.MODE_FAST)])
def test_tied_column_ledger(name, mode):
    """The construction and the bound of tests/test_gpu_monitors.py's column ledger test: the device's balance drift
    against the float32 restatement's ledger, whose dissipation uses each base node's own C_i (a copy of C_G per member
    would count the base's dissipation nine times). Peaks of tied members are equal."""
    R = tc.column_reference()
    case = tc.column3d_case()
    P = case.packing
    D = P.dof_count
    mass32 = np.repeat(P.lumped_mass, 3)
    fixed = xc.constrained(P)
    dt, steps, groups = R["dt"], R["steps"] + 1, R["groups"]
    sysm = pcg.MatrixFreeSystem.from_packing(P, case.materials, 1.0, 0.0, mode=mode)
    sys_r = pcg.MatrixFreeSystem.from_packing(P, case.materials, 1.0, 0.0, mode=mode)
    st = ExplicitStepper(P, case.materials, RayleighCoefficients(0.0, 0.0), system=sysm, dt=dt)
    try:
        force_at = xc.curve_force(np.zeros(D), R["pattern"], R["pts"], dt, explicit.curve_value)
        tie = (groups,) + tc.group_records(groups, P.lumped_mass, 0.0, dt, (R["ids"], R["Cn"]))
        led = mc.LedgerReference()
        for s in xc.scheme_steps(applier(sys_r, D), mass32, fixed, P.bc_value, force_at, 0.0, 0.0, dt,
                                 np.zeros(D, np.float32), np.zeros(D, np.float32), 0, steps, None, tie):
            led.add(s.n + 1, mc.energy_terms(mass32, fixed, 0.0, dt, s.v, s.y, s.f, s.un, s.vn, (R["ids"], R["Cn"])))
        ref_steps, ref_rows, ref_bounds = led.arrays()
        drift_f32 = mc.balance_drift(ref_rows)
        slack = 2.0 * float(ref_bounds.sum(1).max()) / float((ref_rows[:, 0] + ref_rows[:, 1]).max())
        st.set_load_pattern(np.zeros(D), R["pattern"])
        st.set_load_curve(R["pts"])
        st.set_dashpots(R["ids"], R["Cn"])
        st.set_ties(*R["ties"])
        st.set_monitors(energy_every=1, energy_capacity=steps, peaks=True)
        r = st.advance(steps)
        assert r.has_value() and r.value().finite
        e = st.energy()
        assert np.array_equal(e.steps, ref_steps)
        rows = np.stack([e.kinetic, e.potential, e.work, e.dissipated], 1)
        drift = mc.balance_drift(rows)
        ratio = float(e.dissipated[-1] / e.work[-1])
        worst = float(np.abs(rows - ref_rows).max() / np.abs(ref_rows).max())
        print(f"tied column ledger {name} ({steps} steps): dissipated / work {ratio:.9f}; balance drift / max total: "
              f"f32 restatement {drift_f32:.2e}, device {drift:.2e} (summation slack {slack:.1e}); rows against the "
              f"restatement's, largest difference / largest entry {worst:.2e}")
        assert drift <= drift_f32 + slack, (drift, drift_f32, slack)
        assert abs(1.0 - ratio) <= R["left"], (ratio, R["left"])  # the work that went in left through the base, once
        assert_bitwise(st.get_state(U), s.un, f"{name}: u at the end")
        for pk in st.peaks():
            for members in groups:
                assert np.all(pk[members].view(np.uint32) == pk[members[0]].view(np.uint32))
            assert pk.max() > 0.0
    finally:
        st.close()
        sysm.close()
        sys_r.close()


# ---- 9. the driver --------------------------------------------------------------------------------------------------
SCENARIO = """mesh:
  path: block.msh
materials:
  - name: soil
    E: 3.0e9
    nu: 0.3
    rho: 1800.0
assignments:
  - group: SOLID
    material: soil
damping:
  xi: 0.02
  w1: 5.0
  w2: 50.0
time:
  dt: 1.0e-4
  adaptive: false
solver:
  type: pcg
  preconditioner: block_jacobi
  tol_runtime: 3.0e-4
  tol_pause: 1.0e-5
  max_iters: 200
precision:
  vectors: fp32
  reductions: fp64
curves:
  quake:
    - [0.0, 0.0]
    - [1.0e-4, 1.0e-3]
    - [3.0e-4, -5.0e-4]
    - [1.0e-3, 0.0]
loads:
  gravity: [0.0, 0.0, -9.81]
absorbing:
  - group: BASE
    incident: {direction: [1, 0, 0.25], velocity_curve: quake}
tied:
  - group: YSIDE
    axis: 2
  - pair: [XLO, XHI]
    axis: 0
output:
  vtu_stride: 1
  probes: [0, 5]
"""


def test_run_with_a_tied_scenario(tmp_path):
    """python -m cwf.run --integrator explicit on a scenario with both forms of ``tied:`` and ``absorbing:``: the frames
    are a direct ExplicitStepper run's; the Newmark drivers refuse the scenario. The groups are disjoint (a Gmsh node
    belongs to one entity): the base, the two x faces above it, and the rest of the two y faces."""
    import glob
    import json
    import os
    import subprocess
    import sys

    from cwf import absorbing, meshgen, run
    from cwf.physics import compute_rayleigh

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    runner = os.path.join(os.path.dirname(_lib.LIB_PATH), "cwf_run")
    tm = meshgen.kuhn_block(4, 3, 3, 0.25)
    X = tm.coords
    up, lo, hi = X[:, 2] > 0.0, X.min(0), X.max(0)
    tm.node_groups["BASE"] = np.nonzero(~up)[0].astype(np.uint32)
    tm.node_groups["XLO"] = np.nonzero(up & (X[:, 0] == lo[0]))[0].astype(np.uint32)
    tm.node_groups["XHI"] = np.nonzero(up & (X[:, 0] == hi[0]))[0].astype(np.uint32)
    tm.node_groups["YSIDE"] = np.nonzero(up & (X[:, 0] > lo[0]) & (X[:, 0] < hi[0]) &
                                         ((X[:, 1] == lo[1]) | (X[:, 1] == hi[1])))[0].astype(np.uint32)
    names = ["BASE", "XLO", "XHI", "YSIDE"]
    meshgen.write_gmsh(tm, str(tmp_path / "block.msh"), surface_groups=("BASE",), node_groups=names)
    y = tmp_path / "block.yaml"
    y.write_text(SCENARIO)
    env = dict(os.environ, PYTHONPATH=os.path.join(root, "civiwave-fem_amd"))
    out = tmp_path / "out"
    p = subprocess.run([sys.executable, "-m", "cwf.run", str(y), "--integrator", "explicit", "--steps", "5", "--out",
                        str(out)], capture_output=True, text=True, cwd=root, env=env)
    assert p.returncode == 0, p.stderr
    summary = json.loads(p.stdout.strip().splitlines()[-1])["summary"]
    assert summary["integrator"] == "explicit" and summary["steps"] == 5 and summary["absorbing_nodes"] == 20
    assert (summary["tie_groups"], summary["tied_nodes"]) == (12 + 3, 24 + 18)
    frames = sorted(os.path.basename(f) for f in glob.glob(str(out / "vtu" / "*.vtu")))
    assert frames == [f"frame_{i:05d}.vtu" for i in range(5)]
    cfg, m, P, mats = run.load_scenario(str(y))
    for n in names:
        assert np.array_equal(np.sort(m.node_groups[m.group_names[n]]), tm.node_groups[n]), n
    raw = open(out / "vtu" / "frame_00004.vtu", "rb").read()
    at = raw.index(b'encoding="raw">\n_') + len(b'encoding="raw">\n_')
    assert int(np.frombuffer(raw, np.uint32, 1, at)[0]) == 12 * P.node_count
    vtu_u = np.frombuffer(raw, np.float32, 3 * P.node_count, at + 4)
    # the stepper driven directly: the same dashpots, pattern and curve, and the set built by cwf.ties, ties first
    ids, Cn = absorbing.dashpots(m, cfg, absorbing.faces_of_group(m, "BASE"))
    entry = cfg.absorbing[0]
    off, tids = ties.merge(P.node_count, ties.levels(m.coords, tm.node_groups["YSIDE"], 2),
                           ties.periodic(m.coords, tm.node_groups["XLO"], tm.node_groups["XHI"], 0))
    assert [len(g) for g in ties.groups_of(off, tids)].count(6) == 3
    st = ExplicitStepper(P, mats, compute_rayleigh(cfg.damping), cfg.solver, cfg.time)
    try:
        assert st.telemetry().dt == summary["dt"]
        st.set_ties(off, tids)
        st.set_load_pattern(pack.assemble_load_vector(m, cfg, P.lumped_mass64),
                            absorbing.incident_pattern(ids, Cn, entry.incident.direction, P.node_count))
        st.set_load_curve(cfg.curves[entry.incident.velocity_curve])
        st.set_dashpots(ids, Cn)
        r = st.advance(5 * summary["steps_per_frame"])
        assert r.has_value() and r.value().steps == summary["explicit_steps"]
        u = st.get_state(U)
        assert_bitwise(vtu_u, u, "frame 4: u")
        assert np.abs(u).max() > 0.0
        ux = u.reshape(-1, 3)[tm.node_groups["XLO"]] - u.reshape(-1, 3)[tm.node_groups["XHI"]]
        assert np.all(ux == 0.0)  # the two x faces started equal and moved together
    finally:
        st.close()
        st.system.close()
    # the Newmark drivers refuse the scenario instead of ignoring the key (absorbing: is answered first: take it out)
    y.write_text(SCENARIO.replace("absorbing:\n  - group: BASE\n    incident: {direction: [1, 0, 0.25], "
                                  "velocity_curve: quake}\n", ""))
    p = subprocess.run([sys.executable, "-m", "cwf.run", str(y), "--steps", "1"], capture_output=True, text=True,
                       cwd=root, env=env)
    assert p.returncode != 0 and "tied boundaries need the explicit integrator" in p.stderr, p.stderr
    p = subprocess.run([runner, str(y), "--steps", "1"], capture_output=True, text=True)
    assert p.returncode != 0 and "tied boundaries need the explicit integrator" in p.stderr, p.stderr
