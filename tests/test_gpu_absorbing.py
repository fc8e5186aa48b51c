"""Absorbing boundaries and the incident wave of the explicit stepper on the GPU (cwf_hip_explicit_set_dashpots,
cwf.absorbing).

1. The stepper is the scheme, bit for bit: the numpy restatement of the header's arithmetic with the matrix rows of
   the dashpot nodes (explicit_common.host_scheme; P, Q from cwf_explicit_dashpot_update, y from cwf_hip_apply_keff
   on a second handle) against ExplicitStepper.advance, on a PARITY handle and the three FAST operator kinds, undamped,
   damped, and with a load curve, non-zero constraints and a seeded state.
2. More than one workgroup: 392 nodes, dashpots on five faces and on every node.
3. Set, replace, clear, get, and the refusals that leave the previous set in force.
4. The compliant base: a Gaussian incident velocity fed through the dashpots of a 1-D soil column doubles at the free
   surface and leaves through the base again. The conditions are asserted on an all-fp64 numpy run of the scheme with
   the dense K first, then on the GPU runs.
5. An outgoing pulse is absorbed; a fixed base keeps it.
6. Dashpots 1e4 times the physical ones do not lower the step limit.
7. python -m cwf.run --integrator explicit with an ``absorbing:`` scenario; the Newmark drivers refuse it.

The control of 4 is the same load on the same column with the base's dashpots taken away, a base that reflects. The
base cannot be held by a constraint there: a force on a constrained DOF does no work, so no energy would enter and the
ratio end / peak would be 0 / 0. 5, where the energy is in the initial state, has the constrained (fixed) base.
"""
import ctypes as C
import functools
import glob
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import absorbing_common as ac
import explicit_common as xc
from cwf import _lib, absorbing, meshgen, pack, pcg, run, scenarios
from cwf.explicit import ExplicitStepper
from cwf.physics import RayleighCoefficients, compute_rayleigh
from explicit_common import (CHECKPOINTS, KINDS, ROOT, U, V, VARIANTS, applier, big_case, constrained, deviation,
                             group, mesh_case, new_system, random_spd)
from helpers import assert_bitwise

pytestmark = pytest.mark.gpu

RUNNER = os.path.join(os.path.dirname(_lib.LIB_PATH), "cwf_run")


def check_scheme(case, kind, variant, ids, checkpoints, what):
    """ExplicitStepper with random dashpots on `ids` against the restatement at every checkpoint, u and v bitwise."""
    with xc.SchemeRun(case, kind, variant) as S:
        P = case.packing
        ids = S.rng.permutation(np.asarray(ids, np.int64))  # the caller's order is not ascending
        Cn = random_spd(S.rng, P.lumped_mass[ids], S.dt)
        assert np.abs(Cn[:, 0, 1]).min() > 0.0
        dash = (ids,) + ac.update_matrices(Cn, P.lumped_mass[ids], S.alpha, S.dt)
        S.st.set_dashpots(ids, Cn)
        S.load()
        S.check(checkpoints, what, dash)
        # the dashpots did something: the scalar scheme alone gives other bits at the dashpot nodes
        u_plain, v_plain = S.host(S.u0, S.v0, 0, 1)
        u_dash, v_dash = S.host(S.u0, S.v0, 0, 1, dash)
        free_dash = ~S.fixed.reshape(-1, 3)[ids]
        if free_dash.any() and np.abs(v_plain).max() > 0.0:
            assert not np.array_equal(v_plain.reshape(-1, 3)[ids][free_dash], v_dash.reshape(-1, 3)[ids][free_dash])
        S.check_mask_wins(ids)  # a constrained dashpot node


# ---- 1. the stepper is the scheme -----------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("kind", list(KINDS))
def test_stepper_with_dashpots_is_the_scheme_bit_for_bit(kind, variant):
    case = xc.case_of(kind, 5.0 if VARIANTS[variant].get("curve") else None)
    ids = np.concatenate([group(case, "TIP"), group(case, "FIXED")[[0, 7, 13]]])
    check_scheme(case, kind, variant, ids, CHECKPOINTS, f"{kind}/{variant}")


# ---- 2. more than one workgroup -------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["five_faces", "every_node"])
@pytest.mark.parametrize("kind", ["parity", "lattice"])
def test_two_workgroups(kind, which):
    case = big_case()
    X = case.mesh.coords
    assert case.packing.node_count == 392
    if which == "every_node":
        ids = np.arange(392)
    else:
        lo, hi = X.min(0), X.max(0)
        on = (X[:, 0] == lo[0]) | (X[:, 0] == hi[0]) | (X[:, 1] == lo[1]) | (X[:, 1] == hi[1]) | (X[:, 2] == lo[2])
        ids = np.nonzero(on)[0]
        assert ids.min() < 256 <= ids.max() and ids.size == 392 - 6 * 5 * 6
    check_scheme(case, kind, "undamped", ids, (3, 10), f"{kind}/{which}")


# ---- 3. set, replace, clear -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["parity", "lattice"])
def test_set_replace_clear_and_refusals(kind):
    case = mesh_case()
    P = case.packing
    D, N = P.dof_count, P.node_count
    fixed = constrained(P)
    mass = np.repeat(P.lumped_mass, 3)
    bcv = P.bc_value
    f = P.external_force.copy()
    rng = np.random.Generator(np.random.PCG64(21))
    sys_a, sys_b = new_system(case, kind), new_system(case, kind)
    st = ExplicitStepper(P, case.materials, RayleighCoefficients(5.0, 0.0), system=sys_a)
    fresh = ExplicitStepper(P, case.materials, RayleighCoefficients(5.0, 0.0), system=sys_a)
    try:
        dt = st.telemetry().dt
        apply = applier(sys_b, D)

        def host(u, v, first, steps, dash):
            return xc.host_scheme(apply, mass, fixed, bcv, lambda n: f, 5.0, 0.0, dt, u, v, first, steps, dash)

        def dash_of(ids):
            Cn = random_spd(rng, P.lumped_mass[ids], dt)
            return ids, Cn, (ids,) + ac.update_matrices(Cn, P.lumped_mass[ids], 5.0, dt)

        ids_a, C_a, dash_a = dash_of(group(case, "TIP")[::-1])
        ids_b, C_b, dash_b = dash_of(np.concatenate([group(case, "TIP")[:7], [21, 22, 26]]))
        # cleared before the first step: a stepper that never had dashpots
        st.set_dashpots(ids_a, C_a)
        got_ids, got_C = st.get_dashpots()
        assert np.array_equal(got_ids, ids_a.astype(np.uint32)) and np.array_equal(got_C, C_a)
        st.clear_dashpots()
        assert st.get_dashpots()[0].size == 0
        assert st.advance(20).has_value() and fresh.advance(20).has_value()
        assert_bitwise(st.get_state(U), fresh.get_state(U), "cleared before the first step: u")
        assert_bitwise(st.get_state(V), fresh.get_state(V), "cleared before the first step: v")
        u, v = host(np.zeros(D, np.float32), np.zeros(D, np.float32), 0, 20, None)
        assert_bitwise(st.get_state(U), u, "20 steps without dashpots: u")
        # set A, 5 steps; replace by B: state and step count kept; 5 steps; clear; 5 steps
        st.set_dashpots(ids_a, C_a)
        assert st.advance(5).has_value()
        u, v = host(u, v, 20, 5, dash_a)
        assert_bitwise(st.get_state(U), u, "A: u")
        assert_bitwise(st.get_state(V), v, "A: v")
        st.set_dashpots(ids_b, C_b)
        assert st.telemetry().steps == 25
        assert_bitwise(st.get_state(U), u, "after the replacement: u")
        assert_bitwise(st.get_state(V), v, "after the replacement: v")
        # refusals: each leaves B in force
        for bad_ids, bad_C, msg, ctx in (
                (np.array([3, 9, 3]), C_b[:3], "dashpot node listed twice", "index=2"),
                (np.array([3, N]), C_b[:2], "dashpot node out of range", "index=1"),
                (np.array([3, 9]), np.stack([C_b[0], C_b[1] + np.array([[0, 1e-3 * C_b[1, 0, 0], 0], [0] * 3, [0] * 3])]),
                 "dashpot matrix is not symmetric", "index=1"),
                (np.array([3, 9]), np.stack([-C_b[0], C_b[1]]), "dashpot matrix is not positive semidefinite",
                 "index=0"),
                (np.array([9]), np.full((1, 3, 3), np.nan), "dashpot matrix is not finite", "index=0")):
            with pytest.raises(RuntimeError) as e:
                st.set_dashpots(bad_ids, bad_C)
            assert msg in str(e.value) and f"'{ctx}'" in str(e.value), str(e.value)
            got_ids, got_C = st.get_dashpots()
            assert np.array_equal(got_ids, ids_b.astype(np.uint32)) and np.array_equal(got_C, C_b)
        assert st.advance(5).has_value()
        u, v = host(u, v, 25, 5, dash_b)
        assert_bitwise(st.get_state(U), u, "B after the refusals: u")
        assert_bitwise(st.get_state(V), v, "B after the refusals: v")
        st.set_dashpots(np.zeros(0, np.uint32), np.zeros((0, 3, 3)))  # count == 0
        assert st.advance(5).has_value()
        u, v = host(u, v, 30, 5, None)
        assert_bitwise(st.get_state(U), u, "dashpots dropped at step 30: u")
        assert_bitwise(st.get_state(V), v, "dashpots dropped at step 30: v")
        assert st.telemetry().steps == 35
    finally:
        st.close()
        fresh.close()
        sys_a.close()
        sys_b.close()


# ---- 4 / 5. physics on the soil column ------------------------------------------------------------------------------
def gpu_states(st, steps):
    """[(u_n, v_(n-1/2))] for n = 0 .. steps, one step per advance."""
    out = [(st.get_state(U), st.get_state(V))]
    for _ in range(steps):
        r = st.advance(1)
        assert r.has_value() and r.value().finite, r.error() if not r.has_value() else "non-finite"
        out.append((st.get_state(U), st.get_state(V)))
    return out


def gpu_energies(states, apply, mass, at):
    return np.array([ac.energy(apply(states[n][0]), mass, states[n][0], states[n][1], states[n + 1][1]) for n in at])


def top_dofs(wave):
    return 3 * group(ac.column_case(wave), "TOP") + ac.column_axis(wave)


@functools.lru_cache(maxsize=None)
def incident_reference(wave, dt):
    """The all-fp64 runs of the incident-wave case at step dt: absorbing base (A), the same with the operator and the
    force through float32 (B, the f32-operator floor), and the reflecting control."""
    case, ref = ac.column_case(wave), ac.column_dense(wave)
    K, mass, fixed = ref["K"], ref["mass"], ref["fixed"]
    ids, Cn = ac.column_dashpots(wave)
    d = np.zeros(3)
    d[ac.column_axis(wave)] = 1.0
    pattern = absorbing.incident_pattern(ids, Cn, d, case.packing.node_count)
    pts, steps = ac.incident_curve(wave, dt)
    assert steps + 2 <= 4096  # CWF_EXPLICIT_MAX_CURVE_POINTS
    vals = np.array([p[1] for p in pts] + [pts[-1][1]])

    def force_at(n):
        return vals[n] * pattern

    runs = {}
    for name, dash, rnd in (("A", (ids, Cn), False), ("B", (ids, Cn), True), ("control", None, False)):
        runs[name] = list(ac.scheme_f64(K, mass, fixed, dt, steps + 1, force_at, dash, round_operator=rnd))
    top = top_dofs(wave)
    out = dict(ids=ids, Cn=Cn, pattern=pattern, pts=pts, steps=steps, runs=runs)
    for name in ("A", "control"):
        out["E_" + name] = ac.energies_f64(K, mass, runs[name])
        out["top_" + name] = np.array([s[2][top].mean() for s in runs[name]])
    npk = int(np.abs(out["top_A"]).argmax())
    out["npk"] = npk
    out["floor_u"] = deviation(runs["B"][npk][1], runs["A"][npk][1])
    out["floor_v"] = deviation(runs["B"][npk][2], runs["A"][npk][2])
    return out


def physical_conditions(top_v, E, E_control, what):
    doubling = float(np.abs(top_v).max()) / 1e-3
    left = float(E[-1] / E.max())
    kept = float(E_control[-1] / E_control.max())
    print(f"{what}: peak top velocity / incident peak {doubling:.4f}, energy end / peak {left:.2e}, "
          f"control end / peak {kept:.3f}")
    assert abs(doubling - 2.0) <= 0.02 * 2.0, (what, doubling)
    assert left <= 1e-3, (what, left)
    assert kept >= 0.5, (what, kept)


@pytest.mark.parametrize("wave", ["P", "S"])
def test_compliant_base_doubles_at_the_surface_and_absorbs(wave):
    """Measured on an MI355X ("Absorbing boundaries"): peak top velocity / incident peak 2.0036 on the
    fp64 reference, PARITY and FAST lattice, P (149 steps) and S (278 steps); energy end / peak 7.2e-7 (P), 1.7e-6 (S);
    the control keeps 1.000. At the peak step, floors u 3.4e-7 v 5.4e-6 (P), u 7.3e-7 v 2.0e-5 (S); PARITY against the
    fp64 reference u 2.9e-7 v 4.4e-6 (P), u 4.6e-7 v 1.8e-5 (S); FAST lattice against PARITY u 4.5e-7 v 7.6e-6 (P),
    u 6.7e-7 v 2.3e-5 (S), recorded only."""
    case = ac.column_case(wave)
    P = case.packing
    D = P.dof_count
    mass = np.repeat(P.lumped_mass.astype(np.float64), 3)
    top = top_dofs(wave)
    sys_p = pcg.MatrixFreeSystem.from_packing(P, case.materials, 1.0, 0.0, mode=_lib.MODE_PARITY)
    sys_f = pcg.MatrixFreeSystem.from_packing(P, case.materials, 1.0, 0.0, mode=_lib.MODE_FAST)
    sys_b = pcg.MatrixFreeSystem.from_packing(P, case.materials, 1.0, 0.0, mode=_lib.MODE_PARITY)
    apply = applier(sys_b, D)
    probe = ExplicitStepper(P, case.materials, RayleighCoefficients(0.0, 0.0), system=sys_p)
    dt = probe.telemetry().dt
    probe.close()
    try:
        R = incident_reference(wave, dt)
        steps, npk = R["steps"], R["npk"]
        # the conditions on the fp64 reference first
        physical_conditions(R["top_A"], R["E_A"], R["E_control"], f"{wave} fp64 reference ({steps} steps, dt {dt:.4e})")
        bu = min(max(8.0 * R["floor_u"], 1e-6), 1e-3)
        bv = min(max(8.0 * R["floor_v"], 1e-6), 1e-3)
        print(f"{wave}: f32-operator floor at step {npk}: u {R['floor_u']:.2e} v {R['floor_v']:.2e}, "
              f"bounds u {bu:.2e} v {bv:.2e}")
        assert 0 < npk < steps

        def gpu_run(sysm, dashpots):
            st = ExplicitStepper(P, case.materials, RayleighCoefficients(0.0, 0.0), system=sysm, dt=dt)
            try:
                st.set_load_pattern(np.zeros(D), R["pattern"])
                st.set_load_curve(R["pts"])
                if dashpots:
                    st.set_dashpots(R["ids"], R["Cn"])
                states = gpu_states(st, steps + 1)
            finally:
                st.close()
            E = gpu_energies(states, apply, mass, range(steps + 1))
            return states, E, np.array([s[1][top].astype(np.float64).mean() for s in states])

        parity = None
        for name, sysm in (("PARITY", sys_p), ("FAST lattice", sys_f)):
            states, E, top_v = gpu_run(sysm, True)
            _, E_control, _ = gpu_run(sysm, False)
            physical_conditions(top_v, E, E_control, f"{wave} {name}")
            if parity is None:
                parity = states
                du = deviation(states[npk][0], R["runs"]["A"][npk][1])
                dv = deviation(states[npk][1], R["runs"]["A"][npk][2])
                print(f"{wave} PARITY deviation from the fp64 reference at step {npk}: u {du:.2e} v {dv:.2e}")
                assert du <= bu and dv <= bv, (du, bu, dv, bv)
            else:
                du = deviation(states[npk][0], parity[npk][0].astype(np.float64))
                dv = deviation(states[npk][1], parity[npk][1].astype(np.float64))
                print(f"{wave} FAST lattice deviation from PARITY at step {npk}: u {du:.2e} v {dv:.2e}")
                assert math.isfinite(du) and math.isfinite(dv)
    finally:
        sys_p.close()
        sys_f.close()
        sys_b.close()


@functools.lru_cache(maxsize=None)
def pulse_reference(wave, dt):
    u0, v0, steps = ac.outgoing_pulse(wave, dt)
    ids, Cn = ac.column_dashpots(wave)
    out = dict(u0=u0, v0=v0, steps=steps, ids=ids, Cn=Cn)
    for name, dash, fixed_base in (("absorbing", (ids, Cn), False), ("fixed", None, True)):
        r = ac.column_dense(wave, fixed_base)
        st = list(ac.scheme_f64(r["K"], r["mass"], r["fixed"], dt, steps + 1, None, dash, u0, v0))
        E = ac.energies_f64(r["K"], r["mass"], st)
        out[name] = float(E[steps] / E[0])
    return out


@pytest.mark.parametrize("wave", ["P", "S"])
def test_outgoing_pulse_leaves_through_the_base(wave):
    case, held = ac.column_case(wave), ac.column_case(wave, True)
    P = case.packing
    D = P.dof_count
    mass = np.repeat(P.lumped_mass.astype(np.float64), 3)
    systems = []

    def system(c, mode):
        systems.append(pcg.MatrixFreeSystem.from_packing(c.packing, c.materials, 1.0, 0.0, mode=mode))
        return systems[-1]

    try:
        sys_p = system(case, _lib.MODE_PARITY)
        probe = ExplicitStepper(P, case.materials, RayleighCoefficients(0.0, 0.0), system=sys_p)
        dt = probe.telemetry().dt
        probe.close()
        R = pulse_reference(wave, dt)
        steps = R["steps"]
        print(f"{wave} pulse fp64 reference ({steps} steps): energy left / initial {R['absorbing']:.2e} absorbing, "
              f"{R['fixed']:.3f} fixed base")
        assert R["absorbing"] <= 2e-2 and R["fixed"] >= 0.9, R
        apply = {False: applier(system(case, _lib.MODE_PARITY), D), True: applier(system(held, _lib.MODE_PARITY), D)}
        for name, mode in (("PARITY", _lib.MODE_PARITY), ("FAST lattice", _lib.MODE_FAST)):
            left = {}
            for fixed_base, c in ((False, case), (True, held)):
                st = ExplicitStepper(c.packing, c.materials, RayleighCoefficients(0.0, 0.0), system=system(c, mode),
                                     dt=dt)
                try:
                    if not fixed_base:
                        st.set_dashpots(R["ids"], R["Cn"])
                    free = ~constrained(c.packing)
                    st.set_state(U, np.where(free, R["u0"], 0.0).astype(np.float32))
                    st.set_state(V, np.where(free, R["v0"], 0.0).astype(np.float32))
                    first = gpu_states(st, 1)
                    assert st.advance(steps - 1).has_value()
                    last = gpu_states(st, 1)
                finally:
                    st.close()
                E0 = ac.energy(apply[fixed_base](first[0][0]), mass, first[0][0], first[0][1], first[1][1])
                E1 = ac.energy(apply[fixed_base](last[0][0]), mass, last[0][0], last[0][1], last[1][1])
                left[fixed_base] = E1 / E0
            print(f"{wave} pulse {name}: energy left / initial {left[False]:.2e} absorbing, {left[True]:.3f} fixed base")
            assert left[False] <= 2e-2 and left[True] >= 0.9, (name, left)
    finally:
        for s in systems:
            s.close()


# ---- 6. the step limit is unchanged ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def limit_case():
    return scenarios.block_case(4, 3, 3)


@functools.lru_cache(maxsize=None)
def limit_dense():
    return ac.dense_of(limit_case())


def limit_dashpots():
    """Physical dashpots of random unit normals on the TIP face's nodes, scaled by 1e4."""
    case = limit_case()
    ids = group(case, "TIP")
    rng = np.random.Generator(np.random.PCG64(9))
    nu = rng.standard_normal((ids.size, 3))
    nu /= np.linalg.norm(nu, axis=1)[:, None]
    nn = nu[:, :, None] * nu[:, None, :]
    mat = case.cfg.materials[0]
    vp, vs = ac.wave_speed(mat, "P"), ac.wave_speed(mat, "S")
    Cn = 1e4 * mat.density * 0.1 * 0.1 * (vp * nn + vs * (np.eye(3) - nn))
    u0 = (1e-6 * rng.standard_normal(case.packing.dof_count)).astype(np.float32)
    u0[constrained(case.packing)] = 0.0
    return ids, Cn, u0


@pytest.mark.parametrize("kind", ["parity", "lattice"])
def test_large_dashpots_leave_the_step_limit_alone(kind):
    case = limit_case()
    P = case.packing
    D = P.dof_count
    ref = limit_dense()
    mass = ref["mass"]
    ids, Cn, u0 = limit_dashpots()
    sys_a, sys_b = new_system(case, kind), new_system(case, "parity")
    st = ExplicitStepper(P, case.materials, RayleighCoefficients(0.0, 0.0), system=sys_a)
    plain = ExplicitStepper(P, case.materials, RayleighCoefficients(0.0, 0.0), system=sys_a)
    try:
        before = st.telemetry()
        st.set_dashpots(ids, Cn)
        tel, tel_plain = st.telemetry(), plain.telemetry()
        for name in ("lambda_max", "critical_dt", "dt"):
            a, b, c = (np.float64(getattr(t, name)).view(np.uint64) for t in (tel, tel_plain, before))
            assert a == b == c, name
        dt = tel.dt
        assert dt == 0.9 * tel.critical_dt
        # the fp64 reference on this block, every step, first
        states = list(ac.scheme_f64(ref["K"], mass, ref["fixed"], dt, 2001, None, (ids, Cn), u0.astype(np.float64)))
        E = ac.energies_f64(ref["K"], mass, states)
        print(f"step limit {kind}: dt {dt:.4e}, fp64 reference energy peak / initial {E.max() / E[0]:.3f}")
        assert np.all(np.isfinite(E)) and E.max() <= 4.0 * E[0]
        apply = applier(sys_b, D)
        # the zero external force of the reference
        st.set_external_force(np.zeros(D, np.float32))
        st.set_state(U, u0)
        first = gpu_states(st, 1)
        E0 = ac.energy(apply(first[0][0]), mass, first[0][0], first[0][1], first[1][1])
        ratios, done = [], 1
        for upto in range(200, 2001, 200):
            r = st.advance(upto - 1 - done)
            assert r.has_value() and r.value().finite
            s = gpu_states(st, 1)
            done = upto
            ratios.append(ac.energy(apply(s[0][0]), mass, s[0][0], s[0][1], s[1][1]) / E0)
        t = st.telemetry()
        assert t.finite and t.steps == 2000
        print(f"step limit {kind}: energy / initial at ten checkpoints {np.array2string(np.array(ratios), precision=3)}")
        assert len(ratios) == 10 and max(ratios) <= 4.0 and min(ratios) > 0.0
    finally:
        st.close()
        plain.close()
        sys_a.close()
        sys_b.close()


# ---- 7. the driver --------------------------------------------------------------------------------------------------
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
output:
  vtu_stride: 1
  probes: [0, 5]
"""


def test_run_with_an_absorbing_scenario(tmp_path):
    tm = meshgen.kuhn_block(4, 3, 3, 0.25)
    tm.node_groups["BASE"] = np.nonzero(tm.coords[:, 2] == 0.0)[0].astype(np.uint32)
    meshgen.write_gmsh(tm, str(tmp_path / "block.msh"), surface_groups=("BASE",), node_groups=["BASE"])
    y = tmp_path / "block.yaml"
    y.write_text(SCENARIO)
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "civiwave-fem_amd"))
    out = tmp_path / "out"
    p = subprocess.run([sys.executable, "-m", "cwf.run", str(y), "--integrator", "explicit", "--steps", "5", "--out",
                        str(out)], capture_output=True, text=True, cwd=ROOT, env=env)
    assert p.returncode == 0, p.stderr
    summary = json.loads(p.stdout.strip().splitlines()[-1])["summary"]
    assert summary["integrator"] == "explicit" and summary["steps"] == 5
    assert summary["absorbing_nodes"] == 20
    frames = sorted(os.path.basename(f) for f in glob.glob(str(out / "vtu" / "*.vtu")))
    assert frames == [f"frame_{i:05d}.vtu" for i in range(5)]
    cfg, m, P, mats = run.load_scenario(str(y))
    raw = open(out / "vtu" / "frame_00004.vtu", "rb").read()
    at = raw.index(b'encoding="raw">\n_') + len(b'encoding="raw">\n_')
    nbytes = int(np.frombuffer(raw, np.uint32, 1, at)[0])
    assert nbytes == 12 * P.node_count
    vtu_u = np.frombuffer(raw, np.float32, 3 * P.node_count, at + 4)
    # the stepper driven directly with the same dashpots, pattern and curve
    ids, Cn = absorbing.dashpots(m, cfg, absorbing.faces_of_group(m, "BASE"))
    assert ids.size == 20
    entry = cfg.absorbing[0]
    st = ExplicitStepper(P, mats, compute_rayleigh(cfg.damping), cfg.solver, cfg.time)
    try:
        assert st.telemetry().dt == summary["dt"]
        st.set_load_pattern(pack.assemble_load_vector(m, cfg, P.lumped_mass64),
                            absorbing.incident_pattern(ids, Cn, entry.incident.direction, P.node_count))
        st.set_load_curve(cfg.curves[entry.incident.velocity_curve])
        st.set_dashpots(ids, Cn)
        r = st.advance(5 * summary["steps_per_frame"])
        assert r.has_value() and r.value().steps == summary["explicit_steps"]
        u = st.get_state(U)
        assert_bitwise(vtu_u, u, "frame 4: u")
        assert np.abs(u).max() > 0.0
    finally:
        st.close()
        st.system.close()
    # the Newmark drivers refuse the scenario instead of ignoring the key
    p = subprocess.run([sys.executable, "-m", "cwf.run", str(y), "--steps", "1"], capture_output=True, text=True,
                       cwd=ROOT, env=env)
    assert p.returncode != 0 and "absorbing boundaries need the explicit integrator" in p.stderr, p.stderr
    p = subprocess.run([RUNNER, str(y), "--steps", "1"], capture_output=True, text=True)
    assert p.returncode != 0 and "absorbing boundaries need the explicit integrator" in p.stderr, p.stderr
