"""The explicit stepper's monitors on the GPU (cwf_hip_explicit_set_monitors, include/cwf_hip.h "Monitors"): receiver
traces, peak maps and the energy ledger against the numpy restatement of the scheme (explicit_common.scheme_steps,
y from cwf_hip_apply_keff on a second handle).

1. Receivers are the state, bit for bit, at every recorded step count; a full buffer drops and counts.
2. Peaks are the running maxima of the stated expressions, bit for bit.
3. The ledger's four columns are the restatement's sums within the worst-case summation bound; two steppers agree bit
   for bit; an unsampled step still enters the cumulative columns.
4. Two workgroups with a tail (392 nodes); 5. more than 256 workgroups in the fold (70,602 nodes).
6. The soil column: work enters, leaves through the base, and the balance stays put.
7. Refusals and lifecycle. 8. python -m cwf.run's three flags.
"""
import functools
import json
import os

import numpy as np
import pytest

import absorbing_common as ac
import explicit_common as xc
import monitors_common as mc
from cwf import _lib, explicit, pcg, run, scenarios
from cwf.explicit import ExplicitStepper
from cwf.physics import RayleighCoefficients, compute_rayleigh
from explicit_common import (CHECKPOINTS, KINDS, U, V, YAML, advance, applier, big_case, check_ledger, group,
                             new_system, random_spd, run_cli)
from helpers import assert_bitwise

pytestmark = pytest.mark.gpu

CONFIGS = dict(  # the shared variants (curve_bc_state also seeds the state here), and two the ledger accepts (beta = 0)
    xc.VARIANTS,
    curve_bc_state=dict(xc.VARIANTS["curve_bc_state"], state=True),
    ledger=dict(alpha=0.0, beta=0.0, curve=True),
    ledger_alpha=dict(alpha=5.0, beta=0.0, curve=True),
)
STATE_VARIANTS = ["undamped", "damped", "curve_bc_state"]
LEDGER_VARIANTS = ["ledger", "ledger_alpha"]
STEPS, EXTRA = 53, 5  # the restatement runs STEPS + EXTRA steps: the refill after reset_monitors


def eq64(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


class Setup:
    """What a stepper of one case is given, and the restatement's per-update record of the run it then makes."""


def build_setup(case, kind, config, dash_ids, receivers, steps):
    """Everything deterministic about one run: inputs (dashpots, loads, constraints, initial state, dt) and the
    restatement's u_n, v_(n-1/2) for n = 0 .. steps, the peak candidates and the ledger terms of every update."""
    cfg = CONFIGS[config]
    P = case.packing
    D = P.dof_count
    S = Setup()
    S.case, S.kind, S.cfg = case, kind, cfg
    S.alpha, S.beta = cfg["alpha"], cfg["beta"]
    S.fixed = xc.constrained(P)
    S.mass = np.repeat(P.lumped_mass, 3)
    rng = np.random.Generator(np.random.PCG64(7))
    S.bcv, S.u0, S.v0 = xc.seeded_state(P, S.fixed, rng if cfg.get("state") else None)
    S.packing = xc.with_bc(P, S.bcv) if cfg.get("state") else P
    sys_a, sys_b = new_system(case, kind), new_system(case, kind)
    probe = ExplicitStepper(S.packing, case.materials, RayleighCoefficients(S.alpha, S.beta), system=sys_a)
    try:
        S.dt = probe.telemetry().dt
        S.ids = rng.permutation(np.asarray(dash_ids, np.int64))
        S.Cn = random_spd(rng, P.lumped_mass[S.ids], S.dt)
        Pm, Qm = ac.update_matrices(S.Cn, P.lumped_mass[S.ids], S.alpha, S.dt)
        S.receivers = rng.permutation(np.asarray(receivers, np.int64))
        if cfg.get("curve"):
            S.base, S.pattern = case.load_pattern()
            _, S.curve = case.load_curve
            S.force_at = xc.curve_force(S.base, S.pattern, S.curve, S.dt)
        else:
            S.curve = None
            S.force_at = xc.constant_force(P)
        S.U, S.V, S.cand, S.terms = [S.u0], [S.v0], [], []
        for s in xc.scheme_steps(applier(sys_b, D), S.mass, S.fixed, S.bcv, S.force_at, S.alpha, S.beta, S.dt, S.u0,
                                 S.v0, 0, steps, (S.ids, Pm, Qm)):
            S.U.append(s.un)
            S.V.append(s.vn)
            S.cand.append(mc.peak_candidates(s.v, s.un, s.vn, S.dt))
            if S.beta == 0.0:
                S.terms.append(mc.energy_terms(S.mass, S.fixed, S.alpha, S.dt, s.v, s.y, s.f, s.un, s.vn,
                                               (S.ids, S.Cn)))
        assert np.abs(S.U[-1][~S.fixed]).max() > 0.0 and np.abs(S.V[-1][~S.fixed]).max() > 0.0
    finally:
        probe.close()
        sys_a.close()
        sys_b.close()
    return S


def small_case(kind, config):
    return xc.case_of(kind, 5.0 if CONFIGS[config].get("curve") else None)


@functools.lru_cache(maxsize=None)
def small_setup(kind, config):
    case = small_case(kind, config)
    dash_ids = np.concatenate([group(case, "TIP"), group(case, "FIXED")[[0, 7, 13]]])
    receivers = np.unique(np.concatenate([group(case, "FIXED")[[0, 7, 13]], group(case, "TIP")[[0, 2]],
                                          [21, 22, 26, 33, 41]]))
    return build_setup(case, kind, config, dash_ids, receivers, STEPS + EXTRA)


def stepper_of(S, system, dashpots=True):
    st = ExplicitStepper(S.packing, S.case.materials, RayleighCoefficients(S.alpha, S.beta), system=system, dt=S.dt)
    assert st.telemetry().dt == S.dt
    if dashpots:
        st.set_dashpots(S.ids, S.Cn)
    if S.curve is not None:
        st.set_load_pattern(S.base, S.pattern)
        st.set_load_curve(S.curve)
    if S.cfg.get("state"):
        st.set_state(U, S.u0)
        st.set_state(V, S.v0)
    return st


def check_rows(S, tr, want_steps, what):
    assert np.array_equal(tr.steps, np.asarray(want_steps, np.uint64)), (what, tr.steps)
    assert np.array_equal(tr.time, tr.steps.astype(np.float64) * S.dt)
    r = S.receivers
    assert tr.u.shape == tr.v.shape == (len(want_steps), r.size, 3)
    for i, n in enumerate(want_steps):
        assert_bitwise(tr.u[i].reshape(-1), S.U[n].reshape(-1, 3)[r].reshape(-1), f"{what}: u row of step {n}")
        assert_bitwise(tr.v[i].reshape(-1), S.V[n].reshape(-1, 3)[r].reshape(-1), f"{what}: v row of step {n}")


def running_peaks(S, first, last):
    """The maxima over the updates first .. last - 1, from zero."""
    peaks = [np.zeros(S.case.packing.node_count, np.float32) for _ in range(3)]
    for n in range(first, last):
        mc.raise_peaks(peaks, S.cand[n])
    return peaks


def check_peaks(got, want, what):
    for name, g, w in zip(("peak_u", "peak_v", "peak_a"), got, want):
        assert_bitwise(g, w, f"{what}: {name}")


def ledger_reference(S, first, last, every=1):
    led = mc.LedgerReference()
    for n in range(first, last):
        led.add(n + 1, S.terms[n], sample=(n + 1) % every == 0)
    return led.arrays()


# ---- 1. receivers are the state -------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", STATE_VARIANTS)
@pytest.mark.parametrize("kind", list(KINDS))
def test_receivers_are_the_state_bit_for_bit(kind, variant):
    S = small_setup(kind, variant)
    assert S.fixed.reshape(-1, 3)[S.receivers].all(1).any() and not np.array_equal(S.receivers, np.sort(S.receivers))
    system = new_system(S.case, kind)
    every1, every7, short = (stepper_of(S, system) for _ in range(3))
    try:
        every1.set_monitors(receivers=S.receivers, receiver_every=1, receiver_capacity=64)
        every7.set_monitors(receivers=S.receivers, receiver_every=7, receiver_capacity=64)
        short.set_monitors(receivers=S.receivers, receiver_every=1, receiver_capacity=5)
        done = 0
        for upto in CHECKPOINTS:
            assert advance(every1, upto - done).steps == upto
            done = upto
            check_rows(S, every1.receiver_traces(), range(1, upto + 1), f"{kind}/{variant} every 1 at {upto}")
        i = every1.monitor_info()
        assert (i.receiver_count, i.receiver_every, i.receiver_capacity, i.receiver_samples, i.receiver_dropped) == \
            (S.receivers.size, 1, 64, 53, 0)
        advance(every7, STEPS)
        check_rows(S, every7.receiver_traces(), range(7, 50, 7), f"{kind}/{variant} every 7")
        advance(short, STEPS)
        check_rows(S, short.receiver_traces(), range(1, 6), f"{kind}/{variant} capacity 5")
        i = short.monitor_info()
        assert i.receiver_samples == 5 and i.receiver_dropped == 48
        for st in (every1, every7, short):
            assert_bitwise(st.get_state(U), S.U[STEPS], "u after 53 steps")
            assert_bitwise(st.get_state(V), S.V[STEPS], "v after 53 steps")
        # the accelerations of consecutive rows
        tr = every1.receiver_traces()
        assert np.array_equal(tr.acceleration(), np.diff(tr.v.astype(np.float64), axis=0) / S.dt)
        with pytest.raises(ValueError):
            every7.receiver_traces().acceleration()
    finally:
        for st in (every1, every7, short):
            st.close()
        system.close()


# ---- 2. peaks are the running maxima --------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", STATE_VARIANTS)
@pytest.mark.parametrize("kind", list(KINDS))
def test_peaks_are_the_running_maxima_bit_for_bit(kind, variant):
    """Every entry is compared bit for bit: the device's fp64 square root gave the correctly rounded value in all of
    them (0 entries needed the one-ulp allowance)."""
    S = small_setup(kind, variant)
    system = new_system(S.case, kind)
    st = stepper_of(S, system)
    try:
        st.set_monitors(peaks=True)
        assert st.monitor_info().peaks
        check_peaks(st.peaks(), running_peaks(S, 0, 0), "at set")
        done = 0
        for upto in CHECKPOINTS:
            advance(st, upto - done)
            done = upto
            check_peaks(st.peaks(), running_peaks(S, 0, upto), f"{kind}/{variant} after {upto} steps")
        pu, pv, pa = st.peaks()
        free_nodes = ~S.fixed.reshape(-1, 3).all(1)
        held_nodes = S.fixed.reshape(-1, 3).all(1)
        assert held_nodes.any() and free_nodes.any()
        assert np.all(pu[free_nodes] > 0.0) and np.all(pv[free_nodes] > 0.0) and np.all(pa[free_nodes] > 0.0)
        assert_bitwise(pu[held_nodes], mc.norm3(S.bcv.astype(np.float64))[held_nodes], "peak_u of held nodes is |bc|")
        assert np.all(pv[held_nodes] == 0.0) and np.all(pa[held_nodes] == 0.0)
        if S.cfg.get("state"):
            assert np.all(pu[held_nodes] > 0.0)
        assert_bitwise(st.get_state(U), S.U[STEPS], "u with peaks")
        assert_bitwise(st.get_state(V), S.V[STEPS], "v with peaks")
        st.reset_monitors()
        check_peaks(st.peaks(), running_peaks(S, 0, 0), "after reset")
        advance(st, EXTRA)
        check_peaks(st.peaks(), running_peaks(S, STEPS, STEPS + EXTRA), f"{kind}/{variant} refilled after the reset")
    finally:
        st.close()
        system.close()


# ---- 3. the ledger is the restatement -------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", LEDGER_VARIANTS)
@pytest.mark.parametrize("kind", list(KINDS))
def test_ledger_is_the_restatement(kind, variant):
    S = small_setup(kind, variant)
    system = new_system(S.case, kind)
    a, b, tenth = (stepper_of(S, system) for _ in range(3))
    try:
        a.set_monitors(energy_every=1, energy_capacity=64)
        b.set_monitors(energy_every=1, energy_capacity=64)
        tenth.set_monitors(energy_every=10, energy_capacity=8)
        done = 0
        for upto in CHECKPOINTS:
            advance(a, upto - done)
            done = upto
        advance(b, STEPS)
        advance(tenth, STEPS)
        ref = ledger_reference(S, 0, STEPS)
        got_a = check_ledger(a.energy(), ref, f"{kind}/{variant} every step")
        assert np.abs(ref[1][:, 2]).max() > 0.0 and ref[1][-1, 3] > 0.0 and ref[1][-1, 0] > 0.0
        eb = b.energy()
        assert eq64(got_a, np.stack([eb.kinetic, eb.potential, eb.work, eb.dissipated], axis=1))
        led = tenth.energy()
        assert list(led.steps) == [10, 20, 30, 40, 50]
        got_t = check_ledger(led, ledger_reference(S, 0, STEPS, every=10), f"{kind}/{variant} every 10")
        # the cumulative sums are sums over every step whatever is sampled, and in the same order: same bits
        assert eq64(got_t[:, 2:], got_a[9::10, 2:][:5]) and eq64(got_t[:, :2], got_a[9::10, :2][:5])
        e = a.energy()
        assert np.array_equal(e.total(), e.kinetic + e.potential)
        assert np.array_equal(e.balance(), e.total() - e.work + e.dissipated)
        i = tenth.monitor_info()
        assert (i.energy_every, i.energy_capacity, i.energy_samples, i.energy_dropped) == (10, 8, 5, 0)
        for st in (a, b, tenth):
            assert_bitwise(st.get_state(U), S.U[STEPS], "u with a ledger")
            assert_bitwise(st.get_state(V), S.V[STEPS], "v with a ledger")
    finally:
        for st in (a, b, tenth):
            st.close()
        system.close()


# ---- 4. more than one workgroup, and the tail -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def big_setup(kind):
    case = big_case()
    X = case.mesh.coords
    lo, hi = X.min(0), X.max(0)
    on = (X[:, 0] == lo[0]) | (X[:, 0] == hi[0]) | (X[:, 1] == lo[1]) | (X[:, 1] == hi[1]) | (X[:, 2] == lo[2])
    return build_setup(case, kind, "undamped", np.nonzero(on)[0], np.arange(392), 10)


@pytest.mark.parametrize("kind", ["parity", "lattice"])
def test_two_workgroups_and_the_tail(kind):
    S = big_setup(kind)
    assert S.case.packing.node_count == 392 and S.receivers.size == 392
    system = new_system(S.case, kind)
    st = stepper_of(S, system)
    try:
        st.set_monitors(receivers=S.receivers, receiver_every=1, receiver_capacity=16, peaks=True, energy_every=1,
                        energy_capacity=16)
        for upto, n in ((3, 3), (10, 7)):
            advance(st, n)
            check_rows(S, st.receiver_traces(), range(1, upto + 1), f"{kind} 392 nodes at {upto}")
            check_peaks(st.peaks(), running_peaks(S, 0, upto), f"{kind} 392 nodes at {upto}")
            check_ledger(st.energy(), ledger_reference(S, 0, upto), f"{kind} 392 nodes at {upto}")
        assert_bitwise(st.get_state(U), S.U[10], "u")
        assert_bitwise(st.get_state(V), S.V[10], "v")
    finally:
        st.close()
        system.close()


# ---- 5. more than 256 workgroups in the fold ------------------------------------------------------------------------
def test_fold_of_more_than_256_workgroups():
    case = scenarios.block_case(41, 40, 40, harmonic=5.0)
    N = case.packing.node_count
    assert N == 70602 and (N + 255) // 256 == 276
    X = case.mesh.coords
    base = np.nonzero(X[:, 2] == X[:, 2].min())[0]
    receivers = np.array([0, 255, 256, 65535, 65536, 70601, 12345, 40000])
    steps = 5
    S = build_setup(case, "lattice", "ledger", base, receivers, steps)
    system = new_system(case, "lattice")
    st = stepper_of(S, system)
    try:
        st.set_monitors(receivers=S.receivers, receiver_every=1, receiver_capacity=steps, energy_every=1,
                        energy_capacity=steps)
        advance(st, steps)
        check_rows(S, st.receiver_traces(), range(1, steps + 1), "70,602 nodes")
        check_ledger(st.energy(), ledger_reference(S, 0, steps), "70,602 nodes")
        assert_bitwise(st.get_state(U), S.U[steps], "u")
    finally:
        st.close()
        system.close()


# ---- 6. physics on the soil column ----------------------------------------------------------------------------------
@pytest.mark.parametrize("wave", ["P", "S"])
def test_soil_column_ledger(wave):
    """Measured on an MI355X ("Monitors"), max |balance_i - balance_0| / max total: P (150 steps)
    fp64 reference 4.5e-14, f32 restatement and device alike 8.3e-08 (PARITY) and 1.9e-07 (FAST lattice); S (279 steps)
    1.5e-13, 1.4e-07 (PARITY), 2.1e-07 (FAST lattice). 1 - dissipated / work: 3.9e-07 and 2.6e-07 (P), 8.7e-07 and
    9.5e-07 (S), inside the energy-left figures 7.2e-07 and 1.7e-06."""
    case = ac.column_case(wave)
    P = case.packing
    D = P.dof_count
    mass32 = np.repeat(P.lumped_mass, 3)
    mass = mass32.astype(np.float64)
    fixed = xc.constrained(P)
    systems = {}
    for name, mode in (("PARITY", _lib.MODE_PARITY), ("FAST lattice", _lib.MODE_FAST)):
        systems[name] = [pcg.MatrixFreeSystem.from_packing(P, case.materials, 1.0, 0.0, mode=mode) for _ in range(2)]
    apply = applier(systems["PARITY"][1], D)  # the energy of a state, as test_gpu_absorbing computes it
    probe = ExplicitStepper(P, case.materials, RayleighCoefficients(0.0, 0.0), system=systems["PARITY"][0])
    dt = probe.telemetry().dt
    probe.close()
    try:
        R = mc.column_incident(wave, dt)
        steps = R["steps"] + 1
        assert steps + 1 <= 4096
        drift_f64 = mc.balance_drift(mc.ledger_of_f64_run(wave, dt))
        Pm, Qm = ac.update_matrices(R["Cn"], P.lumped_mass[R["ids"]], 0.0, dt)

        force_at = xc.curve_force(np.zeros(D), R["pattern"], R["pts"], dt, explicit.curve_value)  # the stepper's c(t_n)
        c = ac.wave_speed(ac.SOIL, wave)
        n0 = int(4.0 * 6.0 * ac.COLUMN_H / c / dt)  # the pulse's peak enters at t0 = 4 sigma / c
        for name, (sysm, sys_r) in systems.items():
            # the f32 restatement with this kind's operator, and its ledger
            led = mc.LedgerReference()
            for s in xc.scheme_steps(applier(sys_r, D), mass32, fixed, P.bc_value, force_at, 0.0, 0.0, dt,
                                     np.zeros(D, np.float32), np.zeros(D, np.float32), 0, steps, (R["ids"], Pm, Qm)):
                led.add(s.n + 1, mc.energy_terms(mass32, fixed, 0.0, dt, s.v, s.y, s.f, s.un, s.vn,
                                                 (R["ids"], R["Cn"])))
            ref_steps, ref_rows, ref_bounds = led.arrays()
            drift_f32 = mc.balance_drift(ref_rows)
            total_max = float((ref_rows[:, 0] + ref_rows[:, 1]).max())
            # a row's balance is off by at most the sum of its columns' bounds; the drift compares two rows
            slack = 2.0 * float(ref_bounds.sum(1).max()) / total_max
            st = ExplicitStepper(P, case.materials, RayleighCoefficients(0.0, 0.0), system=sysm, dt=dt)
            try:
                st.set_load_pattern(np.zeros(D), R["pattern"])
                st.set_load_curve(R["pts"])
                st.set_dashpots(R["ids"], R["Cn"])
                st.set_monitors(energy_every=1, energy_capacity=steps)
                # test_gpu_absorbing's energy-left figure of this run, by its own computation
                states = [(st.get_state(U), st.get_state(V))]
                for _ in range(steps):
                    advance(st, 1)
                    states.append((st.get_state(U), st.get_state(V)))
                E = np.array([ac.energy(apply(states[n][0]), mass, states[n][0], states[n][1], states[n + 1][1])
                              for n in range(steps)])
                left = float(E[-1] / E.max())
                e = st.energy()
            finally:
                st.close()
            rows = check_ledger(e, (ref_steps, ref_rows, ref_bounds), f"{wave} {name}")
            assert e.work[n0] > 0.0 and np.all(np.diff(e.work[:n0 + 1]) >= 0.0), "work rises while the pulse enters"
            ratio = float(e.dissipated[-1] / e.work[-1])
            drift = mc.balance_drift(rows)
            print(f"{wave} {name} ({steps} steps): energy end / peak {left:.2e}, dissipated / work {ratio:.9f} "
                  f"(1 - ratio {1.0 - ratio:.2e}); balance drift / max total: fp64 reference {drift_f64:.2e}, "
                  f"f32 restatement {drift_f32:.2e}, device {drift:.2e} (summation slack {slack:.1e})")
            assert abs(1.0 - ratio) <= left, (ratio, left)
            assert drift <= drift_f32 + slack, (drift, drift_f32, slack)
    finally:
        for pair in systems.values():
            for x in pair:
                x.close()


# ---- 7. refusals and lifecycle --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["parity", "lattice"])
def test_refusals_and_lifecycle(kind):
    S = small_setup(kind, "ledger_alpha")
    N = S.case.packing.node_count
    system = new_system(S.case, kind)
    st, plain = stepper_of(S, system), stepper_of(S, system)
    try:
        r = S.receivers
        st.set_monitors(receivers=r, receiver_every=1, receiver_capacity=64, energy_every=1, energy_capacity=64)
        advance(st, 5)
        for bad, kw, msg, ctx in (
                (np.array([3, 9, 3]), {}, "receiver node listed twice", ["index=2", "node=3"]),
                (np.array([3, N]), {}, "receiver node out of range", ["index=1", f"node={N}"]),
                (np.array([3, 4]), dict(receiver_capacity=0), "monitor capacity must not be zero", []),
                (np.array([3, 4]), dict(receiver_every=0), "receiver_every must be at least 1", []),
                (None, dict(energy_every=2, energy_capacity=0), "monitor capacity must not be zero", [])):
            with pytest.raises(RuntimeError) as e:
                st.set_monitors(**dict(dict(receivers=bad, receiver_every=1, receiver_capacity=8), **kw))
            assert msg in str(e.value) and all(f"'{c}'" in str(e.value) for c in ctx), str(e.value)
        # the previous set is in force: the recording goes on across the refused calls
        advance(st, 5)
        check_rows(S, st.receiver_traces(), range(1, 11), f"{kind}: across the refusals")
        check_ledger(st.energy(), ledger_reference(S, 0, 10), f"{kind}: across the refusals")
        # a new set between advances keeps u, v, the step count and the dashpots; its counts and sums start at zero
        st.set_monitors(receivers=r[:3], receiver_every=2, receiver_capacity=8, peaks=True, energy_every=1,
                        energy_capacity=64)
        assert st.telemetry().steps == 10
        assert_bitwise(st.get_state(U), S.U[10], "u after set_monitors")
        assert_bitwise(st.get_state(V), S.V[10], "v after set_monitors")
        ids, Cn = st.get_dashpots()
        assert np.array_equal(ids, S.ids.astype(np.uint32)) and np.array_equal(Cn, S.Cn)
        advance(st, 6)
        tr = st.receiver_traces()
        assert list(tr.steps) == [12, 14, 16]
        assert_bitwise(tr.u[-1].reshape(-1), S.U[16].reshape(-1, 3)[r[:3]].reshape(-1), "the new set's rows")
        check_peaks(st.peaks(), running_peaks(S, 10, 16), f"{kind}: peaks from the set on")
        check_ledger(st.energy(), ledger_reference(S, 10, 16), f"{kind}: ledger from the set on")
        # set_dashpots while a ledger is active: the dissipation follows the new matrices
        rng = np.random.Generator(np.random.PCG64(33))
        C2 = random_spd(rng, S.case.packing.lumped_mass[S.ids], S.dt)
        st.set_dashpots(S.ids, C2)
        st.reset_monitors()
        sys_b = new_system(S.case, kind)
        try:
            P2, Q2 = ac.update_matrices(C2, S.case.packing.lumped_mass[S.ids], S.alpha, S.dt)
            led, led_old = mc.LedgerReference(), mc.LedgerReference()
            for s in xc.scheme_steps(applier(sys_b, S.case.packing.dof_count), S.mass, S.fixed, S.bcv, S.force_at,
                                     S.alpha, S.beta, S.dt, S.U[16], S.V[16], 16, 4, (S.ids, P2, Q2)):
                for ledger, Cn in ((led, C2), (led_old, S.Cn)):
                    ledger.add(s.n + 1, mc.energy_terms(S.mass, S.fixed, S.alpha, S.dt, s.v, s.y, s.f, s.un, s.vn,
                                                        (S.ids, Cn)))
            u20 = s.un
        finally:
            sys_b.close()
        advance(st, 4)
        got = check_ledger(st.energy(), led.arrays(), f"{kind}: ledger after set_dashpots")
        old = led_old.arrays()
        assert np.all(np.abs(got[:, 3] - old[1][:, 3]) > 10.0 * old[2][:, 3]), "the old matrices give another sum"
        assert_bitwise(st.get_state(U), u20, "u after the new dashpots")
        # clear: the same bits as a stepper that never had monitors, from the same state on
        advance(plain, 16)
        plain.set_dashpots(S.ids, C2)
        advance(plain, 4)
        st.clear_monitors()
        i = st.monitor_info()
        assert (i.receiver_count, i.energy_every, i.peaks) == (0, 0, False)
        with pytest.raises(RuntimeError) as e:
            st.peaks()
        assert "no peak maps are set" in str(e.value)
        advance(st, 7)
        advance(plain, 7)
        assert_bitwise(st.get_state(U), plain.get_state(U), "u after clear_monitors")
        assert_bitwise(st.get_state(V), plain.get_state(V), "v after clear_monitors")
    finally:
        st.close()
        plain.close()
        system.close()


@pytest.mark.parametrize("kind", ["parity", "lattice"])
def test_ledger_is_refused_with_stiffness_damping(kind):
    S = small_setup(kind, "damped")
    system = new_system(S.case, kind)
    st = stepper_of(S, system)
    try:
        st.set_monitors(receivers=S.receivers[:2], receiver_every=1, receiver_capacity=4, peaks=True)
        with pytest.raises(RuntimeError) as e:
            st.set_monitors(energy_every=1, energy_capacity=4)
        assert "the energy ledger needs rayleigh_beta == 0" in str(e.value)
        L = _lib.load()
        d = _lib.ExplicitMonitorDescC(0, None, 0, 0, 1, 4, 0, 0)
        import ctypes as C

        assert L.cwf_hip_explicit_set_monitors(st._ex, C.byref(d)) == -13  # CWF_ERR_UNSUPPORTED
        assert _lib.last_error(system._h)[0] == "the energy ledger needs rayleigh_beta == 0"
        # peaks and receivers work with any damping, and the refused call left them in force
        advance(st, 3)
        assert list(st.receiver_traces().steps) == [1, 2, 3]
        check_peaks(st.peaks(), running_peaks(S, 0, 3), f"{kind}: peaks with beta")
    finally:
        st.close()
        system.close()


# ---- 8. the scenario run --------------------------------------------------------------------------------------------
def test_run_writes_traces_peaks_and_energy(tmp_path):
    """A scenario's damping always has beta_R > 0 (xi in (0, 1)), for which the ledger is refused: the cantilever runs
    with the traces and the peaks, is refused with all three flags (the next test), and runs with all three under
    --mass-damping-only (alpha_R kept, beta_R = 0)."""
    cfg, m, P, mats = run.load_scenario(YAML)
    probes = list(cfg.output.probes)
    rayleigh = compute_rayleigh(cfg.damping)
    assert rayleigh.beta > 0.0
    for name, flags, ray, energy in (
            ("damped", ["--trace-every", "1", "--peaks"], rayleigh, False),
            ("mass_only", ["--trace-every", "1", "--peaks", "--energy-every", "1", "--mass-damping-only"],
             RayleighCoefficients(rayleigh.alpha, 0.0), True)):
        out = tmp_path / name
        p = run_cli([YAML, "--integrator", "explicit", "--steps", "2", "--out", str(out), *flags])
        assert p.returncode == 0, p.stderr
        summary = json.loads(p.stdout.strip().splitlines()[-1])["summary"]
        total = 2 * summary["steps_per_frame"]
        assert summary["explicit_steps"] == total and summary["trace_samples"] == total
        rows = open(out / "probes" / "traces.csv").read().strip().splitlines()
        assert rows[0] == "step,time,node,ux,uy,uz,vx,vy,vz"
        assert len(rows) == 1 + total * len(probes)
        st = ExplicitStepper(P, mats, ray, cfg.solver, cfg.time)
        try:
            assert st.telemetry().dt == summary["dt"]
            advance(st, total)
            u, v = st.get_state(U).reshape(-1, 3), st.get_state(V).reshape(-1, 3)
        finally:
            st.close()
            st.system.close()
        for row, node in zip((r.split(",") for r in rows[-len(probes):]), probes):
            assert int(row[0]) == total and int(row[2]) == node and float(row[1]) == total * summary["dt"]
            got = np.array([float(x) for x in row[3:]], np.float32)
            assert_bitwise(got, np.concatenate([u[node], v[node]]), f"{name}: last trace row of node {node}")
        peaks = np.load(out / "monitors" / "peaks.npy")
        assert peaks.shape == (P.node_count, 3) and peaks.dtype == np.float32 and peaks.max() > 0.0
        assert os.path.exists(out / "monitors" / "energy.csv") == energy
        if energy:
            erows = open(out / "monitors" / "energy.csv").read().strip().splitlines()
            assert erows[0] == "step,time,kinetic,potential,work,dissipated,balance" and len(erows) == 1 + total
            assert summary["energy_samples"] == total
    # without the flags: the files of the plain run, byte for byte those of the monitored one it shares
    plain = tmp_path / "plain"
    p = run_cli([YAML, "--integrator", "explicit", "--steps", "2", "--out", str(plain)])
    assert p.returncode == 0, p.stderr
    assert not os.path.exists(plain / "monitors") and not os.path.exists(plain / "probes" / "traces.csv")
    for rel in ("probes/probes.csv", "vtu/frame_00000.vtu"):
        assert open(plain / rel, "rb").read() == open(tmp_path / "damped" / rel, "rb").read(), rel
    s = json.loads(p.stdout.strip().splitlines()[-1])["summary"]
    assert "trace_samples" not in s and "energy_samples" not in s
    # the Newmark integrator refuses the flags


def test_ledger_flag_is_refused_with_the_scenarios_stiffness_damping(capsys, tmp_path):
    assert run.main([YAML, "--integrator", "explicit", "--steps", "2", "--trace-every", "1", "--peaks",
                     "--energy-every", "1", "--out", str(tmp_path / "refused")]) == 1
    assert "the energy ledger needs rayleigh_beta == 0" in capsys.readouterr().err
    assert not os.path.exists(tmp_path / "refused" / "monitors")


def test_newmark_refuses_the_monitor_flags(capsys):
    for flag in (["--trace-every", "1"], ["--peaks"], ["--energy-every", "1"], ["--mass-damping-only"]):
        assert run.main([YAML, "--steps", "1", *flag]) == 1
        assert "belong to the explicit integrator" in capsys.readouterr().err
