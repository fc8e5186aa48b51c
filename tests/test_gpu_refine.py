"""The refined static solve on the GPU (cwf_hip_solve_refined, cwf_hip_residual_f64) against dense fp64 algebra.

Reference: K assembled densely in fp64 from the packed f32 records widened (oracle.dense_assemble over
P.gradients[:, :12] and P.volume as float64: the operator the handle itself holds, not helpers.dense_stiffness, whose
fp64 gradients come from the coordinates and differ from the records by 6e-8), K_eff = s_K K + s_M M with M the f32
lumped mass, x_ref = numpy.linalg.solve on the free DOFs with x_c = b_c. Every solve test first computes the
reference's own floor |b - K_eff x_ref| / |b| and asserts its precondition from the reference alone.

The load is an oblique tip load of 1e4 N in all, (6, 0, -8) kN over the TIP nodes, no gravity (E = 30 GPa, nu = 0.2, the
FIXED face clamped). The transverse part bends the block, the hard direction; the axial part keeps the jittered mesh's
reference floor at 7.4e-13, clear of the 1e-12 its precondition asks for (a purely transverse load leaves it at
0.9 - 1.4e-12, inside the spread between LAPACK builds).
Measured figures: profiles/refine_accuracy.txt.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle as O
from cwf import _lib, pcg, scenarios, shard
from helpers import assert_bitwise

pytestmark = pytest.mark.gpu

DOF_BITS = np.array([1, 2, 4], np.uint32)
EPS64 = np.finfo(np.float64).eps
LOAD = dict(point=(6.0e3, 0.0, -8.0e3), gravity=(0.0, 0.0, 0.0))
LAYERS = [0, 0, 1, 1, 2, 0]


@functools.lru_cache(maxsize=None)
def mesh_case(name):
    if name == "block":
        return scenarios.block_case(12, 3, 4, h=0.25, **LOAD)
    if name == "jitter":
        return scenarios.block_case(12, 3, 4, h=0.25, jitter=True, **LOAD)
    if name == "layered":
        return scenarios.layered_case(7, 5, 6, LAYERS, h=0.25, **LOAD)
    if name == "roller":
        return scenarios.roller_case(12, 3, 4, h=0.25, **LOAD)
    if name == "slender":
        return scenarios.block_case(33, 3, 3, h=0.25, **LOAD)
    raise KeyError(name)


def scalars_of(case, newmark):
    return case.scalars() if newmark else (1.0, 0.0)


@functools.lru_cache(maxsize=None)
def dense(name, newmark=False):
    """-> dict(K [D, D] = K_eff, free [D] bool, b [D] the static load): computed once per case, never modified."""
    case = mesh_case(name)
    P = case.packing
    D = P.dof_count
    packed = O.Packed(P.node_count, P.element_count, P.connectivity, P.gradients, P.volume, P.material_index,
                      P.lumped_mass64, P.lumped_mass, P.offsets, P.element_indices, P.local_indices)
    stiff = np.concatenate([np.asarray(m.stiffness, np.float64).reshape(-1) for m in case.materials])
    g64 = np.asarray(P.gradients).reshape(P.element_count, -1)[:, :12].astype(np.float64)
    K = O.dense_assemble(packed, case.mesh.tets, g64, P.volume.astype(np.float64), stiff).reshape(D, D)
    sK, sM = scalars_of(case, newmark)
    K *= sK
    K[np.diag_indices(D)] += sM * np.repeat(P.lumped_mass.astype(np.float64), 3)
    free = (np.repeat(P.bc_mask, 3) & np.tile(DOF_BITS, P.node_count)) == 0
    b = case.static_rhs().astype(np.float64)
    for a in (K, free, b):
        a.setflags(write=False)
    return dict(K=K, free=free, b=b)


@functools.lru_cache(maxsize=None)
def solved_reference(name, newmark=False):
    """-> dict(x [D], floor, cond) of the dense solve of the static load."""
    d = dense(name, newmark)
    free, b = d["free"], d["b"]
    A = d["K"][np.ix_(free, free)]
    x = np.zeros(b.size)
    x[free] = np.linalg.solve(A, b[free])
    floor = float(np.linalg.norm(b[free] - A @ x[free]) / np.linalg.norm(b[free]))
    x.setflags(write=False)
    return dict(x=x, floor=floor, cond=float(np.linalg.cond(A)))


def true_residual(d, b, x):
    """|b - K_eff x| / |b| over the free rows in numpy; constrained DOFs enter as 0 (the reference drops the columns)."""
    free = d["free"]
    xm = np.where(free, x, 0.0)
    return float(np.linalg.norm((b - d["K"] @ xm)[free]) / np.linalg.norm(b[free]))


def make_system(name, mode=_lib.MODE_FAST, newmark=False):
    case = mesh_case(name)
    sK, sM = scalars_of(case, newmark)
    return pcg.MatrixFreeSystem.from_packing(case.packing, case.materials, sK, sM, mode=mode)


def kernel_of(s):
    return _lib.load().cwf_hip_system_keff_kernel(s.handle()).decode()


# ---- 1. the residual kernel against the dense product ----------------------------------------------------------------
@pytest.mark.parametrize("name,mode", [("block", _lib.MODE_FAST), ("jitter", _lib.MODE_FAST),
                                       ("block", _lib.MODE_PARITY), ("layered", _lib.MODE_FAST),
                                       ("roller", _lib.MODE_FAST)])
def test_residual_against_dense_product(name, mode):
    """Random fp64 x and b (not f32-representable), Newmark scalars. Component-wise bound 4096 eps64 (|K_eff||x| + |b|):
    a row touches at most 32 tets of about 100 flops, so a rounding-analysis constant with slack; a wrong corner,
    material or mask is an O(1) error. 12 x 3 x 4 has 260 nodes: two node tiles, the second with 4 nodes. Measured
    worst ratio to (|K_eff||x| + |b|) eps64: profiles/refine_accuracy.txt."""
    d = dense(name, True)
    free = d["free"]
    D = free.size
    rng = np.random.Generator(np.random.PCG64(11))
    x = rng.uniform(-1.0, 1.0, D) * 1e-3
    b = rng.uniform(-1.0, 1.0, D) * 1e6
    assert np.any(x.astype(np.float32).astype(np.float64) != x)
    s = make_system(name, mode, newmark=True)
    if name == "jitter":
        assert kernel_of(s).startswith("k_keff_groups_pipe")  # the renumbered fan-group handle
    r_dev, norm = pcg.residual_f64(s, b, x).value()
    xm = np.where(free, x, 0.0)
    r_np = np.where(free, b - d["K"] @ xm, 0.0)
    scale = np.abs(d["K"]) @ np.abs(xm) + np.abs(b)
    ratio = float(np.max(np.abs(r_dev - r_np)[free] / (EPS64 * scale[free])))
    print(f"{name} mode={mode}: worst |r_dev - r_np| / (eps64 (|K||x| + |b|)) = {ratio:.2f}")
    assert np.all(r_dev[~free] == 0.0)
    assert np.all(np.abs(r_dev - r_np) <= 4096 * EPS64 * scale)
    assert abs(norm - np.linalg.norm(r_dev)) <= 1e-14 * norm
    r2, norm2 = pcg.residual_f64(s, b, x).value()
    assert_bitwise(r2, r_dev, "second call")
    assert norm2 == norm
    s.close()


# ---- 2. the residual kernel against the PARITY operator, many tiles ------------------------------------------------
@pytest.mark.parametrize("tiles", ["compact", "strip"])
def test_residual_matches_parity_operator_on_many_tiles(tiles, monkeypatch):
    """40 x 19 x 9 cells (8,200 nodes, 33 node tiles), b = 0, x random f32 values widened: f32(-r) is the PARITY
    handle's apply_keff(x) within ulp32(y_i) + 1e-13 |y|_inf per free DOF. The kernel keeps the PARITY fold order, so
    the two are in fact equal bit for bit (asserted too); both tile forms of CWF_PARITY_TILES."""
    if tiles == "strip":
        monkeypatch.setenv("CWF_PARITY_TILES", "strip")
    case = scenarios.block_case(40, 19, 9, h=0.25)
    P = case.packing
    assert P.node_count == 8200
    sK, sM = case.scalars()
    s = pcg.MatrixFreeSystem.from_packing(P, case.materials, sK, sM, mode=_lib.MODE_PARITY)
    rng = np.random.Generator(np.random.PCG64(12))
    x32 = rng.uniform(-1.0, 1.0, P.dof_count).astype(np.float32)
    y = np.zeros_like(x32)
    assert pcg.apply_keff(s, x32, y).has_value()
    r, norm = pcg.residual_f64(s, np.zeros(P.dof_count), x32.astype(np.float64)).value()
    free = (np.repeat(P.bc_mask, 3) & np.tile(DOF_BITS, P.node_count)) == 0
    assert np.all(r[~free] == 0.0)
    got = (-r).astype(np.float32)
    tol = np.spacing(np.abs(y)).astype(np.float64) + 1e-13 * float(np.abs(y).max())
    err = np.abs(got.astype(np.float64) - y.astype(np.float64))
    print(f"{tiles}: {int(np.count_nonzero(got[free] != y[free]))} of {int(free.sum())} free DOFs differ from PARITY")
    assert np.all(err[free] <= tol[free])
    assert_bitwise(got[free], y[free], "f32(-r) against the PARITY apply_keff")
    assert abs(norm - np.linalg.norm(r)) <= 1e-14 * norm
    s.close()


# ---- 3. the refined solve against the dense solution ---------------------------------------------------------------
SCHEDULES = {
    "resident": dict(),
    "fused": dict(env={"CWF_RESIDENT": "0"}),
    "two-kernel": dict(env={"CWF_RESIDENT": "0", "CWF_FUSED": "0"}),
    "fan-groups": dict(env={"CWF_LATTICE": "0"}),
    "jitter": dict(name="jitter"),
    "parity": dict(mode=_lib.MODE_PARITY),
    "layered": dict(name="layered"),
    "newmark": dict(newmark=True),
}


def check_history(t, bnorm):
    h = t.history
    assert h.size == t.outer_iterations + 1
    assert h[0] == t.rhs_norm == pytest.approx(bnorm, rel=1e-14)
    assert np.all(h[1:] < h[:-1]), h


@pytest.mark.parametrize("sched", list(SCHEDULES))
def test_refined_solve_against_dense_solution(sched, monkeypatch):
    """tol 1e-10 on the true residual, 100 x above what the dense reference itself attains (asserted). The residual of
    the returned x is evaluated by numpy (an independent evaluation; the factor 2 covers the two summation orders) and
    the error of x is bounded by cond(K_ff) times that. Histories per schedule: profiles/refine_accuracy.txt."""
    c = SCHEDULES[sched]
    name, newmark = c.get("name", "block"), c.get("newmark", False)
    for k, v in c.get("env", {}).items():
        monkeypatch.setenv(k, v)
    d, ref = dense(name, newmark), solved_reference(name, newmark)
    assert ref["floor"] <= 1e-12, ref["floor"]
    b, free = d["b"], d["free"]
    s = make_system(name, c.get("mode", _lib.MODE_FAST), newmark)
    if sched == "fan-groups":
        assert kernel_of(s).startswith("k_keff_groups_pipe")
    res = pcg.solve_refined(s, b, pcg.RefineSettings(relative_tolerance=1e-10))
    assert res.has_value(), res.error()
    x, t = res.value().solution, res.value().telemetry
    true = true_residual(d, b, x)
    err = float(np.linalg.norm(x - ref["x"]) / np.linalg.norm(ref["x"]))
    print(f"{sched}: floor {ref['floor']:.2e} cond {ref['cond']:.2e} outer {t.outer_iterations} inner "
          f"{t.inner_iterations} history/|b| {np.array2string(t.history / t.rhs_norm, precision=2)} numpy residual "
          f"{true:.2e} error {err:.2e} residual_ms {t.residual_ms:.3f} solve_ms {t.solve_ms:.3f}")
    assert t.converged and not t.stagnated
    assert t.residual_norm <= 1e-10 * t.rhs_norm
    assert t.residual_norm == t.history[-1]
    assert true <= 2e-10
    assert err <= ref["cond"] * 2e-10
    assert np.all(x[~free] == 0.0)
    check_history(t, np.linalg.norm(b[free]))
    if sched == "resident":
        # the problem the feature solves: the f32 solve reports convergence at 1e-6 with a true residual far above it
        x32, r32 = np.zeros(b.size, np.float32), np.zeros(b.size, np.float32)
        t32 = pcg.solve_pcg(s, b.astype(np.float32), pcg.PcgSettings(20000, 1e-6, False), pcg.PcgVectors(x32, r32))
        assert t32.has_value() and t32.value().converged
        plain = true_residual(d, b, x32.astype(np.float64))
        print(f"plain f32 solve_pcg at 1e-6: reports {t32.value().residual_norm / t32.value().rhs_norm:.2e}, "
              f"numpy residual {plain:.2e}")
        assert plain > 1e-6
    s.close()


# ---- 4. stagnation is reported, not raised -------------------------------------------------------------------------
def test_stagnation_is_reported_and_the_best_iterate_returned():
    """33 x 3 x 3 at tol 1e-13, at least 100 x below what the dense reference attains (asserted): the loop stops
    stagnated with status CWF_OK, the numpy-evaluated residual of the returned x within 8 x the reference's floor (the
    CPU loop reached 0.35 x; the margin covers another summation order), and x is the iterate with the smallest
    residual of the history, which the device's own fp64 residual of x confirms bit for bit."""
    d, ref = dense("slender"), solved_reference("slender")
    assert ref["floor"] >= 100 * 1e-13, ref["floor"]
    b = d["b"]
    s = make_system("slender")
    settings = pcg.RefineSettings(relative_tolerance=1e-13)
    res = pcg.solve_refined(s, b, settings)
    assert res.has_value(), res.error()
    x, t = res.value().solution, res.value().telemetry
    true = true_residual(d, b, x)
    print(f"slender: floor {ref['floor']:.2e} cond {ref['cond']:.2e} outer {t.outer_iterations} inner "
          f"{t.inner_iterations} history/|b| {np.array2string(t.history / t.rhs_norm, precision=2)} numpy residual "
          f"{true:.2e} = {true / ref['floor']:.2f} x floor")
    assert not t.converged and t.stagnated and t.outer_iterations < settings.max_outer
    assert true <= 8 * ref["floor"]
    assert t.residual_norm == t.history.min()
    _, norm = pcg.residual_f64(s, b, x).value()
    assert norm == t.residual_norm
    s.close()


# ---- 5. prescribed values and warm start ---------------------------------------------------------------------------
def test_prescribed_values_and_warm_start():
    d, ref = dense("block"), solved_reference("block")
    b, free = d["b"], d["free"]
    s = make_system("block")
    cold = pcg.solve_refined(s, b).value()
    # non-zero b_c comes back as x_c bit for bit and does not load the free rows (the reference drops those columns)
    rng = np.random.Generator(np.random.PCG64(13))
    bc = b.copy()
    bc[~free] = rng.uniform(-1e-3, 1e-3, int((~free).sum()))
    pres = pcg.solve_refined(s, bc).value()
    assert_bitwise(pres.solution[~free], bc[~free], "x_c")
    assert_bitwise(pres.solution[free], cold.solution[free], "free rows under prescribed values")
    assert_bitwise(pres.telemetry.history, cold.telemetry.history, "history under prescribed values")
    # |b| = 0 over the free DOFs: the prescribed values, converged, no inner solve
    b0 = np.where(free, 0.0, bc)
    z = pcg.solve_refined(s, b0, x=np.full(b.size, 7.0), settings=pcg.RefineSettings(warm_start=True)).value()
    assert_bitwise(z.solution, b0, "x for |b| = 0")
    assert z.telemetry.converged and (z.telemetry.outer_iterations, z.telemetry.inner_iterations) == (0, 0)
    # warm start from the reference rounded to f32
    x0 = ref["x"].astype(np.float32).astype(np.float64)
    warm = pcg.solve_refined(s, b, pcg.RefineSettings(warm_start=True), x=x0).value()
    tw, tc = warm.telemetry, cold.telemetry
    print(f"warm start: history[0]/|b| {tw.history[0] / tw.rhs_norm:.2e}, inner {tw.inner_iterations} against "
          f"{tc.inner_iterations} cold")
    assert warm.solution is x0 and tw.converged
    assert tw.history[0] <= 1e-2 * tw.rhs_norm
    assert tw.inner_iterations < tc.inner_iterations
    assert true_residual(d, b, x0) <= 2e-10
    s.close()


# ---- 6. the handle afterwards --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [_lib.MODE_FAST, _lib.MODE_PARITY])
def test_handle_is_unchanged_by_a_refined_solve(mode):
    d = dense("block", True)
    b = d["b"]
    s = make_system("block", mode, newmark=True)
    L = _lib.load()
    h = s.handle()  # pushes mode and scalars once; every call below goes through the C-ABI with this handle
    b32 = b.astype(np.float32)
    rng = np.random.Generator(np.random.PCG64(14))
    v = rng.uniform(-1, 1, b.size).astype(np.float32)

    def state():
        x, r, y = np.zeros_like(b32), np.zeros_like(b32), np.zeros_like(b32)
        cs = _lib.PcgSettingsC(2000, 1e-6, 0, 0)
        tel = _lib.PcgTelemetryC()
        assert L.cwf_hip_solve_pcg(h, _lib.ptr(b32), C.byref(cs), _lib.ptr(x), _lib.ptr(r), b.size, 0, C.byref(tel)) == 0
        assert L.cwf_hip_apply_keff(h, _lib.ptr(v), _lib.ptr(y), b.size, 0) == 0
        return x, r, y, tel.iterations, tel.residual_norm, L.cwf_hip_system_keff_kernel(h)

    def same(a, c, what):
        for i in range(3):
            assert_bitwise(a[i], c[i], what)
        assert a[3:] == c[3:], what

    before = state()
    x = np.zeros(b.size)
    tel = _lib.RefineTelemetryC()
    assert L.cwf_hip_solve_refined(h, _lib.ptr(b), None, _lib.ptr(x), b.size, 0, C.byref(tel)) == 0
    assert tel.converged == 1
    same(state(), before, "after a refined solve")
    bad = _lib.RefineSettingsC(40, 0.0, 0.0, _lib.PcgSettingsC(0, 0.0, 0, 0), 0, 0)
    assert L.cwf_hip_solve_refined(h, _lib.ptr(b), C.byref(bad), _lib.ptr(x), b.size, 0, C.byref(tel)) == -11
    assert _lib.last_error(h) == ("max_outer must be <= 31", ["max_outer=40"])
    assert L.cwf_hip_solve_refined(h, _lib.ptr(b), None, _lib.ptr(x), b.size - 3, 0, C.byref(tel)) == -1
    assert L.cwf_hip_solve_refined(h, None, None, _lib.ptr(x), b.size, 0, C.byref(tel)) == -11
    assert L.cwf_hip_residual_f64(h, _lib.ptr(b), None, None, b.size, 0, None) == -11
    assert L.cwf_hip_residual_f64(h, _lib.ptr(b), _lib.ptr(x), None, b.size + 3, 0, None) == -1
    same(state(), before, "after argument errors")
    s.close()


# ---- 7. refusals, max_outer, pointer kinds -------------------------------------------------------------------------
def test_refusals_and_max_outer():
    L = _lib.load()
    tel = _lib.RefineTelemetryC()
    hexc = scenarios.block_case(4, 3, 3, h=0.25, element="hex8")
    hs = pcg.MatrixFreeSystem.from_packing(hexc.packing, hexc.materials, 1.0, 0.0, mode=_lib.MODE_FAST)
    bh = hexc.static_rhs().astype(np.float64)
    e = pcg.solve_refined(hs, bh)
    assert not e.has_value() and e.error().message == "the refined solve of a hex8 handle is not supported"
    assert e.error().context == ["there is no fp64 hex8 operator on the device"]
    xh = np.zeros_like(bh)
    assert L.cwf_hip_solve_refined(hs.handle(), _lib.ptr(bh), None, _lib.ptr(xh), bh.size, 0, C.byref(tel)) == -13
    e = pcg.residual_f64(hs, bh, xh)
    assert not e.has_value() and e.error().message == "the fp64 residual of a hex8 handle is not supported"
    hs.close()
    # a handle attached to a (LOCAL) communicator
    glob = scenarios.block_case(6, 3, 4, h=0.1)
    comm = shard.Comm.local(2)
    src = pcg.MatrixFreeSystem.from_packing(glob.packing, glob.materials, 1.0, 0.0, mode=_lib.MODE_FAST)
    sh = shard.build_shard(src, shard.slab_ranges(glob.packing.node_count, 2), 0)
    member = sh.system(glob.materials, 1.0, 0.0)
    comm.attach(member, sh)
    bm = np.zeros(member.dof_count)
    e = pcg.solve_refined(member, bm)
    assert not e.has_value() and e.error().message == "the refined solve of a sharded handle is not supported"
    xm = np.zeros_like(bm)
    assert L.cwf_hip_solve_refined(member.handle(), _lib.ptr(bm), None, _lib.ptr(xm), bm.size, 0, C.byref(tel)) == -13
    # max_outer = 1: one correction, reported as not converged
    d = dense("block")
    s = make_system("block")
    r = pcg.solve_refined(s, d["b"], pcg.RefineSettings(max_outer=1))
    assert r.has_value(), r.error()
    t = r.value().telemetry
    assert (t.outer_iterations, t.converged, t.history.size) == (1, False, 2)
    assert t.history[1] < t.history[0]
    s.close()


def test_device_pointers_give_the_host_result():
    import torch

    d = dense("jitter")  # the renumbered handle: device vectors are permuted on the way in and out
    b = d["b"]
    s = make_system("jitter")
    host = pcg.solve_refined(s, b).value()
    bd = torch.from_numpy(b.copy()).cuda()
    dev = pcg.solve_refined(s, bd).value()
    torch.cuda.synchronize()
    assert dev.solution.is_cuda and dev.solution.dtype == torch.float64
    assert_bitwise(dev.solution.cpu().numpy(), host.solution, "device-pointer x")
    assert_bitwise(dev.telemetry.history, host.telemetry.history, "device-pointer history")
    rh, nh = pcg.residual_f64(s, b, host.solution).value()
    rd, nd = pcg.residual_f64(s, bd, dev.solution).value()
    assert_bitwise(rd.cpu().numpy(), rh, "device-pointer r")
    assert nd == nh
    s.close()


# ---- 8. determinism ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [_lib.MODE_FAST, _lib.MODE_PARITY])
def test_two_refined_solves_give_identical_bits(mode):
    d = dense("block")
    s = make_system("block", mode)
    a = pcg.solve_refined(s, d["b"]).value()
    c = pcg.solve_refined(s, d["b"]).value()
    assert_bitwise(a.solution, c.solution, "x")
    assert_bitwise(a.telemetry.history, c.telemetry.history, "history")
    assert a.telemetry.inner_iterations == c.telemetry.inner_iterations
    s.close()
