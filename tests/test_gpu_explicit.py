"""The explicit central-difference stepper on the GPU (cwf_hip_explicit_*, cwf.explicit).

1. The stepper is the scheme: a numpy restatement of the header's arithmetic (float32 state, float64 math, rounded
   where stored), each y from cwf_hip_apply_keff on a second handle of the same mesh at scalars (1, 0), against
   ExplicitStepper.advance -- u and v bit for bit, on a PARITY handle and the three FAST operator kinds.
2. The scheme is the physics (PARITY): 200 steps from rest against the same scheme in all-fp64 numpy with the dense
   K. The floor is what rounding the operator's input and output to f32 costs that numpy run; the bound is 8 x the
   floor clamped to [1e-6, 1e-3] (the modal test's convention).
3. The stable step: the power iteration against the dense eigenvalue, its determinism, the default step, the refusal
   of a step above the limit, and the non-finite report (seeded through set_state: nothing is stepped unstably).
4. Neighbours: a Newmark Stepper on the same handle is unaffected; a sharded handle is refused; cwf.run's explicit
   integrator writes frames whose last displacement is the stepper's.

Measured on an MI355X (profiles/explicit_accuracy.txt): every case of 1 is bit-exact; 2 gives u 3.5e-06 / v 2.2e-05
against bounds 3.1e-05 / 3.1e-04; the power iteration reaches 0.9975 of the dense eigenvalue on both handles.
"""
import ctypes as C
import functools
import glob
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import absorbing_common as ac
import explicit_common as xc
from cwf import _lib, explicit, pcg, run, scenarios, shard
from cwf.explicit import ExplicitStepper
from cwf.physics import RayleighCoefficients, compute_rayleigh
from cwf.stepper import Stepper
from explicit_common import CHECKPOINTS, KINDS, ROOT, VARIANTS, YAML, constrained, deviation, mesh_case, new_system
from helpers import assert_bitwise

pytestmark = pytest.mark.gpu


# ---- 1. the stepper is the scheme -----------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("kind", list(KINDS))
def test_stepper_is_the_scheme_bit_for_bit(kind, variant):
    V = VARIANTS[variant]
    with xc.SchemeRun(xc.case_of(kind, 5.0 if V.get("curve") else None), kind, variant) as S:
        tel = S.st.telemetry()
        assert tel.steps == 0 and tel.time == 0.0 and tel.finite
        assert tel.dt == 0.9 * tel.critical_dt and tel.critical_dt == explicit.critical_dt(tel.lambda_max, V["beta"])
        S.load()
        S.check(CHECKPOINTS, f"{kind}/{variant}")
        assert_bitwise(S.st.get_state(ExplicitStepper.EXTERNAL_FORCE), S.force_at(CHECKPOINTS[-1] - 1),
                       "external force of the last step")


# ---- 2. the scheme is the physics -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dense_reference():
    """K (dense, fp64 geometry), the f32 lumped mass and the constrained DOFs of the tet4 block; lambda_max of
    M^-1/2 K M^-1/2 over the free DOFs. Computed once, shared, never modified."""
    return ac.dense_of(mesh_case())


def numpy_run(dt, steps, round_operator, checkpoints=()):
    """The scheme from rest under the packed load in fp64 state and math; round_operator: the operator's input and
    output pass through float32 (reference B), else nothing is rounded (reference A)."""
    ref = dense_reference()
    K, fixed, m = ref["K"], ref["fixed"], ref["mass"]
    f = mesh_case().packing.external_force.astype(np.float64)
    u, v = np.zeros(m.size), np.zeros(m.size)
    out = {}
    for n in range(steps):
        w = np.where(fixed, 0.0, u)
        if round_operator:
            w = w.astype(np.float32).astype(np.float64)
        y = K @ w
        if round_operator:
            y = y.astype(np.float32).astype(np.float64)
        v = np.where(fixed, 0.0, v + dt * ((f - y) / m))
        u = np.where(fixed, 0.0, u + dt * v)
        if n + 1 in checkpoints or n + 1 == steps:
            out[n + 1] = (u.copy(), v.copy())
    return out


def physics_floor(dt, steps=200):
    A = numpy_run(dt, steps, False)[steps]
    B = numpy_run(dt, steps, True)[steps]
    return A, deviation(B[0], A[0]), deviation(B[1], A[1])


def test_scheme_is_the_physics_against_fp64_numpy():
    """Measured on an MI355X (profiles/explicit_accuracy.txt), dt 4.1233e-05: floors u 3.86e-06 v 3.93e-05, bounds
    3.09e-05 3.14e-04, the PARITY stepper's deviation from the all-fp64 run u 3.45e-06 v 2.22e-05."""
    case = mesh_case()
    sysm = new_system(case, "parity")
    st = ExplicitStepper(case.packing, case.materials, RayleighCoefficients(0.0, 0.0), system=sysm)
    try:
        dt = st.telemetry().dt
        A, floor_u, floor_v = physics_floor(dt)
        assert 8.0 * max(floor_u, floor_v) < 1e-3, (floor_u, floor_v)  # else the run is too long for the cap
        r = st.advance(200)
        assert r.has_value(), r.error()
        du = deviation(st.get_state(ExplicitStepper.DISPLACEMENT), A[0])
        dv = deviation(st.get_state(ExplicitStepper.VELOCITY), A[1])
        bu, bv = min(max(8.0 * floor_u, 1e-6), 1e-3), min(max(8.0 * floor_v, 1e-6), 1e-3)
        print(f"explicit physics: dt {dt:.6e} floor u {floor_u:.2e} v {floor_v:.2e} bound u {bu:.2e} v {bv:.2e} "
              f"parity u {du:.2e} v {dv:.2e}")
        assert du <= bu and dv <= bv, (du, bu, dv, bv)
    finally:
        st.close()
        sysm.close()


def test_fast_lattice_deviation_from_parity_is_recorded():
    """Recorded, not asserted beyond finiteness (the issue sets no FAST bound): the FAST lattice run's deviation from
    the PARITY run at 50 and 200 steps, at the PARITY stepper's dt. Measured on an MI355X
    (profiles/explicit_accuracy.txt): 50 steps u 1.29e-06 v 1.47e-05, 200 steps u 6.19e-06 v 2.64e-05."""
    case = mesh_case()
    sp, sf = new_system(case, "parity"), new_system(case, "lattice")
    a = ExplicitStepper(case.packing, case.materials, RayleighCoefficients(0.0, 0.0), system=sp)
    dt = a.telemetry().dt
    b = ExplicitStepper(case.packing, case.materials, RayleighCoefficients(0.0, 0.0), system=sf, dt=dt)
    try:
        for upto, n in ((50, 50), (200, 150)):
            assert a.advance(n).has_value() and b.advance(n).has_value()
            du = deviation(b.get_state(0), a.get_state(0).astype(np.float64))
            dv = deviation(b.get_state(1), a.get_state(1).astype(np.float64))
            print(f"explicit fast-vs-parity: {upto} steps u {du:.2e} v {dv:.2e}")
            assert math.isfinite(du) and math.isfinite(dv)
    finally:
        a.close()
        b.close()
        sp.close()
        sf.close()


# ---- 3. the stable step ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["parity", "lattice"])
def test_lambda_max_against_the_dense_eigenvalue_and_the_step_limits(kind):
    """Measured on an MI355X (profiles/explicit_accuracy.txt): lambda / dense = 0.997527 on both handles (1.905720864e9
    parity, 1.905720855e9 lattice, dense 1.910445799e9), last change 9.0e-05."""
    ref = dense_reference()
    case = mesh_case()
    sysm = new_system(case, kind, case.scalars())
    try:
        lam, change = explicit.lambda_max(sysm, 60)
        lam2, change2 = explicit.lambda_max(sysm, 60)
        print(f"explicit lambda_max {kind}: {lam:.9e} dense {ref['lam_max']:.9e} ratio {lam / ref['lam_max']:.6f} "
              f"last change {change:.2e}")
        assert np.float64(lam).view(np.uint64) == np.float64(lam2).view(np.uint64) and change == change2
        assert 0.98 * ref["lam_max"] <= lam <= (1.0 + 1e-4) * ref["lam_max"], (lam, ref["lam_max"])
        assert 0.0 <= change < 1e-2
        for beta in (0.0, 2e-5):
            st = ExplicitStepper(case.packing, case.materials, RayleighCoefficients(0.0, beta), system=sysm)
            t = st.telemetry()
            st.close()
            assert np.float64(t.lambda_max).view(np.uint64) == np.float64(lam).view(np.uint64)
            assert t.critical_dt == explicit.critical_dt(lam, beta) and t.dt == 0.9 * t.critical_dt
        too_long = 1.05 * explicit.critical_dt(ref["lam_max"], 0.0)
        with pytest.raises(RuntimeError) as e:
            ExplicitStepper(case.packing, case.materials, RayleighCoefficients(0.0, 0.0), system=sysm, dt=too_long)
        assert "time step exceeds the critical step" in str(e.value)
        nums = dict(re.findall(r"'(dt|critical_dt)=([^']+)'", str(e.value)))
        assert float(nums["dt"]) == too_long and float(nums["critical_dt"]) == explicit.critical_dt(lam, 0.0)
    finally:
        sysm.close()


@pytest.mark.parametrize("kind", ["parity", "lattice"])
def test_non_finite_state_is_reported(kind):
    case = mesh_case()
    P = case.packing
    sysm = new_system(case, kind)
    st = ExplicitStepper(P, case.materials, RayleighCoefficients(0.0, 0.0), system=sysm)
    try:
        v = np.zeros(P.dof_count, np.float32)
        v[int(np.nonzero(~constrained(P))[0][-1])] = np.inf
        st.set_state(ExplicitStepper.VELOCITY, v)
        r = st.advance(2)
        assert not r.has_value()
        assert r.error().message == "explicit step produced a non-finite value"
        assert r.error().context == ["steps=2"]
        assert _lib.load().cwf_hip_explicit_advance(st._ex, 0, None) == -10
        # a rewritten state clears the report
        st.set_state(ExplicitStepper.DISPLACEMENT, np.zeros(P.dof_count, np.float32))
        st.set_state(ExplicitStepper.VELOCITY, np.zeros(P.dof_count, np.float32))
        r = st.advance(1)
        assert r.has_value() and r.value().finite and r.value().steps == 3
    finally:
        st.close()
        sysm.close()


# ---- 4. neighbours --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["parity", "lattice"])
def test_newmark_stepper_on_the_same_handle_is_unaffected(kind):
    case = mesh_case()
    P = case.packing
    sysm = new_system(case, kind)

    def three_newmark_steps():
        nm = Stepper(P, case.materials, case.rayleigh, case.cfg.solver, case.cfg.time, system=sysm)
        out, t = [], 0.0
        for _ in range(3):
            r = nm.step(t)
            assert r.has_value(), r.error()
            t = r.value().simulation_time + r.value().time_step
            out.append((nm.get_state(Stepper.DISPLACEMENT), nm.get_state(Stepper.VELOCITY),
                        nm.get_state(Stepper.ACCELERATION), r.value().pcg.iterations))
        nm.close()
        return out

    try:
        before = three_newmark_steps()
        ex = ExplicitStepper(P, case.materials, RayleighCoefficients(5.0, 2e-5), system=sysm)
        assert ex.advance(10).has_value()
        ex.close()
        after = three_newmark_steps()
        for i, (b, a) in enumerate(zip(before, after)):
            for name, x, y in zip("uva", b[:3], a[:3]):
                assert_bitwise(y, x, f"{kind} newmark step {i}: {name}")
            assert a[3] == b[3]
    finally:
        sysm.close()


def test_sharded_handle_is_refused():
    L = _lib.load()
    glob_case = scenarios.block_case(6, 3, 4, h=0.1)
    comm = shard.Comm.local(2)
    src = pcg.MatrixFreeSystem.from_packing(glob_case.packing, glob_case.materials, 1.0, 0.0, mode=_lib.MODE_FAST)
    sh = shard.build_shard(src, shard.slab_ranges(glob_case.packing.node_count, 2), 0)
    member = sh.system(glob_case.materials, 1.0, 0.0)
    comm.attach(member, sh)
    h = member.handle()
    d = _lib.ExplicitDescC()
    out = C.c_void_p()
    assert L.cwf_hip_explicit_create(h, C.byref(d), C.byref(out)) == -13
    assert _lib.last_error(h)[0] == "explicit stepping of a sharded handle is not supported"
    assert not out.value
    lam = C.c_double()
    assert L.cwf_hip_lambda_max(h, 60, C.byref(lam), None) == -13


def test_run_with_the_explicit_integrator_writes_the_steppers_frames(tmp_path):
    out = tmp_path / "out"
    p = subprocess.run([sys.executable, "-m", "cwf.run", YAML, "--integrator", "explicit", "--steps", "20", "--out",
                        str(out)], capture_output=True, text=True, cwd=ROOT,
                       env=dict(os.environ, PYTHONPATH=os.path.join(ROOT, "civiwave-fem_amd")))
    assert p.returncode == 0, p.stderr
    summary = json.loads(p.stdout.strip().splitlines()[-1])["summary"]
    assert summary["integrator"] == "explicit" and summary["steps"] == 20
    cfg, m, P, mats = run.load_scenario(YAML)
    assert summary["steps_per_frame"] == math.ceil(cfg.time.initial_dt / summary["dt"]) >= 1
    assert summary["explicit_steps"] == 20 * summary["steps_per_frame"]
    assert sorted(os.path.basename(f) for f in glob.glob(str(out / "vtu" / "*.vtu"))) == \
        ["frame_00000.vtu", "frame_00010.vtu"]  # vtu_stride 10
    rows = open(out / "probes" / "probes.csv").read().strip().splitlines()
    assert len(rows) == 1 + 20 * len(cfg.output.probes)
    # the stepper driven directly, the same steps: the last VTU frame (10: after 11 frames' steps) holds its
    # displacement and velocity bit for bit, and the last frame's probe rows (20 frames' steps) print its values
    raw = open(out / "vtu" / "frame_00010.vtu", "rb").read()
    at = raw.index(b'encoding="raw">\n_') + len(b'encoding="raw">\n_')
    nbytes = int(np.frombuffer(raw, np.uint32, 1, at)[0])
    assert nbytes == 12 * P.node_count
    vtu_u = np.frombuffer(raw, np.float32, 3 * P.node_count, at + 4)
    vtu_v = np.frombuffer(raw, np.float32, 3 * P.node_count, at + 4 + nbytes + 4)
    st = ExplicitStepper(P, mats, compute_rayleigh(cfg.damping), cfg.solver, cfg.time)
    try:
        assert st.telemetry().dt == summary["dt"]
        assert st.advance(11 * summary["steps_per_frame"]).has_value()
        assert_bitwise(vtu_u, st.get_state(ExplicitStepper.DISPLACEMENT), "frame 10: u")
        assert_bitwise(vtu_v, st.get_state(ExplicitStepper.VELOCITY), "frame 10: v")
        assert np.abs(vtu_u).max() > 0.0
        r = st.advance(9 * summary["steps_per_frame"])
        assert r.has_value() and r.value().time == summary["final_time"] and r.value().steps == summary["explicit_steps"]
        u = st.get_state(ExplicitStepper.DISPLACEMENT).reshape(-1, 3)
    finally:
        st.close()
        st.system.close()
    header = rows[0].split(",")
    cols = [header.index(c) for c in ("ux", "uy", "uz")]
    for row in (r.split(",") for r in rows[-len(cfg.output.probes):]):
        assert int(row[0]) == 19
        node = int(row[header.index("node")])
        assert [row[c] for c in cols] == ["%.9f" % float(x) for x in u[node]], (node, row, u[node])
