"""The structured-block FAST operator (lattice.cpp / lattice.hip, k_keff_lattice; lattice_fused.hip, k_pcg_lattice)
against the pinned oracle.

A FAST handle whose mesh is a Kuhn-split box lattice (one gradient / volume set per Kuhn type) applies K_eff as
the node-pair stencil of the shared cell stiffness. Its arithmetic is the element loop's regrouped in fp32, so it
carries FAST's tolerance contract: K x within 2e-5 of the bit-exact operator relative to its scale (max |row|),
solves at tol 1e-6 within 1e-4 (relative) of the oracle's solution and its iteration count +-10%. Covered: the
detection (and its refusal of a jittered mesh), bricks cut by the block's faces in every direction, partial
Dirichlet masks, Rayleigh scalars, a randomly permuted node order (renumbered to the lattice order and back at
the boundary), Newmark steps, the fan-group path on the same mesh (CWF_LATTICE=0), and slab shards (a shard's
local order: owned planes, then ghost planes) through the LOCAL communicator."""
import numpy as np
import pytest

import oracle as O
from cwf import _lib, meshgen, pack, pcg, scenarios, shard
from cwf.stepper import Stepper
from helpers import oracle_system

pytestmark = pytest.mark.gpu

CASES = {
    "8x3x4": lambda: scenarios.block_case(8, 3, 4, h=0.1, tol=1e-6, max_iterations=600),
    "33x9x5": lambda: scenarios.block_case(33, 9, 5, h=0.1, tol=1e-6, max_iterations=800),
    "rayleigh": lambda: scenarios.block_case(6, 4, 3, h=0.1, xi=0.05, w=(10.0, 100.0), tol=1e-6,
                                             max_iterations=600),
    "rollers": lambda: scenarios.roller_case(12, 10, 7, tol=1e-6, max_iterations=1500),
    "c1": lambda: scenarios.config_case("c1"),
}


@pytest.fixture(scope="module", params=sorted(CASES))
def case(request):
    return CASES[request.param]()


def _system(case, mode=_lib.MODE_FAST, sK=None, sM=None):
    s0, m0 = case.scalars()
    return pcg.MatrixFreeSystem.from_packing(case.packing, case.materials, s0 if sK is None else sK,
                                             m0 if sM is None else sM, mode=mode)


def _kernel(s):
    return (_lib.load().cwf_hip_system_keff_kernel(s.handle()) or b"").decode()


# the structured-block stencil: the resident one-launch solve (resident.hip, the default where the block fits on chip;
# tests/test_gpu_resident.py), the fused one-launch iteration (lattice_fused.hip, where its grid is at most
# CWF_FUSED_MAXWG workgroups) or the two-kernel one (k_keff_lattice + the update pass)
LATTICE = ("k_pcg_resident", "k_pcg_lattice", "k_keff_lattice")


def _apply_err(case, s, seed=3):
    o = oracle_system(case.packing, case.materials, *case.scalars())
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.uniform(-1, 1, case.packing.dof_count).astype(np.float32)
    y = np.zeros_like(x)
    pcg.apply_keff(s, x, y).value()
    ref = o.apply_keff(x).astype(np.float64)
    return np.max(np.abs(y - ref)) / np.max(np.abs(ref))


def permuted_block(nx, ny, nz, h=0.1, **kw):
    """A Kuhn block with randomly permuted node and element order and no jitter: still a lattice."""
    tm = meshgen.jitter_and_permute(meshgen.kuhn_block(nx, ny, nz, h), h, jitter=0.0)
    mesh = pack.from_tetmesh(tm)
    cfg = scenarios.make_config(**kw)
    return scenarios.Case(f"perm{nx}x{ny}x{nz}", mesh, cfg, pack.build_packed_buffers(mesh, cfg))


def test_lattice_detected(case):
    assert _kernel(_system(case)).startswith(LATTICE)


def test_jittered_mesh_is_not_a_lattice():
    case = scenarios.block_case(7, 6, 5, h=0.1, jitter=True, tol=1e-6)
    assert _kernel(_system(case)).startswith("k_keff_groups_pipe")


def test_lattice_apply_close(case):
    assert _apply_err(case, _system(case)) <= 2e-5


def test_lattice_off_runs_the_fan_groups(case, monkeypatch):
    monkeypatch.setenv("CWF_LATTICE", "0")
    s = _system(case)
    assert _kernel(s).startswith("k_keff_groups_pipe")
    assert _apply_err(case, s) <= 2e-5


@pytest.mark.parametrize("L", ["2", "3", "64"])
def test_lattice_work_item_lengths(L, monkeypatch):
    """Planes per work item (CWF_LAT_L): chunk boundaries inside the block and one chunk over all planes (the shell
    workgroups' place in the grid follows the grid's size: lattice.cpp lattice_plan)."""
    monkeypatch.setenv("CWF_LAT_L", L)
    case = scenarios.block_case(40, 17, 9, h=0.1, tol=1e-6)
    assert _apply_err(case, _system(case), seed=11) <= 2e-5


def test_lattice_permuted_node_order():
    case = permuted_block(9, 7, 6, tol=1e-6, max_iterations=800)
    s = _system(case)
    assert _kernel(s).startswith(LATTICE)
    assert _apply_err(case, s) <= 2e-5
    o = oracle_system(case.packing, case.materials, *case.scalars())
    rhs = case.static_rhs()
    x = np.zeros_like(rhs)
    t = pcg.solve_pcg(s, rhs, pcg.PcgSettings(800, 1e-6), pcg.PcgVectors(x, np.zeros_like(rhs))).value()
    ref = o.solve_pcg(rhs, 800, 1e-6)
    assert t.converged
    assert np.linalg.norm(x - ref["x"]) <= 1e-4 * np.linalg.norm(ref["x"])


def test_lattice_solve_close(case):
    s = _system(case)
    o = oracle_system(case.packing, case.materials, *case.scalars())
    rhs = case.static_rhs()
    x = np.zeros_like(rhs)
    mi = case.cfg.solver.max_iterations
    t = pcg.solve_pcg(s, rhs, pcg.PcgSettings(mi, 1e-6), pcg.PcgVectors(x, np.zeros_like(rhs))).value()
    ref = o.solve_pcg(rhs, mi, 1e-6)
    assert t.converged and ref["telemetry"].converged
    assert np.linalg.norm(x - ref["x"]) <= 1e-4 * np.linalg.norm(ref["x"])
    assert abs(t.iterations - ref["telemetry"].iterations) <= max(3, ref["telemetry"].iterations // 10)


@pytest.mark.parametrize("variant", ["z-from-r", "z-stored", "per-node-mass"])
def test_lattice_pcg_variants_solve(variant, monkeypatch):
    """The PCG-loop bricks in their three forms solve to the oracle's solution (bricks cut by the faces in x, y and
    k): the strict interior's one lumped mass as a kernel argument with z = M^-1 r formed from r and the node
    class in the K_eff pass and no z stored by the update pass (CWF_LAT_ZR=1, the default from 2M nodes), or with z
    stored by the update pass (CWF_LAT_ZR=0, the default below), and the per-node mass through LDS (a block whose
    strict interior's lumped masses are not one value: a few perturbed, the oracle given the same masses; z stored)."""
    monkeypatch.setenv("CWF_FUSED", "0")  # the two-kernel iteration's brick variants
    monkeypatch.setenv("CWF_LAT_ZR", "1" if variant == "z-from-r" else "0")
    monkeypatch.setenv("CWF_LAT_L", "3")
    case = scenarios.block_case(40, 19, 9, h=0.1, tol=1e-6, max_iterations=1500)
    if variant == "per-node-mass":  # interior nodes (i, j, k) = (20, 9, 4) and (7, 3, 2) x 1.5 and x 0.75
        P = case.packing
        for (i, j, k), f in (((20, 9, 4), 1.5), ((7, 3, 2), 0.75)):
            n = (k * 20 + j) * 41 + i
            P.lumped_mass64[n] *= f
            P.lumped_mass[n] = np.float32(P.lumped_mass64[n])
    s = _system(case)
    # <..., mass uniform, z from r, plane bases (0 read, 1 affine, 2 affine + deep prefetch)>
    want = {"z-from-r": ["true", "true"], "z-stored": ["true", "false"], "per-node-mass": ["false", "false"]}[variant]
    assert _kernel(s).rstrip(">").split(", ")[-3:-1] == want, _kernel(s)
    assert _apply_err(case, s, seed=5) <= 2e-5
    o = oracle_system(case.packing, case.materials, *case.scalars())
    rhs = case.static_rhs()
    x = np.zeros_like(rhs)
    t = pcg.solve_pcg(s, rhs, pcg.PcgSettings(1500, 1e-6), pcg.PcgVectors(x, np.zeros_like(rhs))).value()
    ref = o.solve_pcg(rhs, 1500, 1e-6)
    assert t.converged and ref["telemetry"].converged
    assert np.linalg.norm(x - ref["x"]) <= 1e-4 * np.linalg.norm(ref["x"])
    n_ref = ref["telemetry"].iterations
    assert abs(t.iterations - n_ref) <= max(3, n_ref // 10)


def test_lattice_stepper_steps():
    case = scenarios.block_case(10, 5, 6, h=0.1, xi=0.05, w=(10.0, 100.0), tol=1e-6, max_iterations=1500)
    P = case.packing
    ref = Stepper(P, case.materials, case.rayleigh, case.cfg.solver, case.cfg.time, mode=_lib.MODE_PARITY)
    fast = Stepper(P, case.materials, case.rayleigh, case.cfg.solver, case.cfg.time, mode=_lib.MODE_FAST)
    for k in range(3):
        tr = ref.step(0.01 * k).value()
        tf = fast.step(0.01 * k).value()
        assert tf.pcg.converged and tr.pcg.converged
        assert abs(tf.pcg.iterations - tr.pcg.iterations) <= max(3, tr.pcg.iterations // 10)
    for what in (Stepper.DISPLACEMENT, Stepper.VELOCITY):
        ur, uf = ref.get_state(what), fast.get_state(what)
        assert np.linalg.norm(uf - ur) <= 1e-4 * np.linalg.norm(ur)


@pytest.mark.parametrize("nranks", [2, 3])
def test_lattice_slab_shards(nranks):
    """Slab sub-meshes (scenarios.slab_case_shape, the bench's decomposition) keep the lattice on every shard
    (local order: owned planes, then the ghost planes): before attach a shard's owned rows are the one-handle
    lattice rows (the same stencil arithmetic; its blocks come from the sub-mesh's own gradients, equal to 1e-6),
    and the attached shards' FAST solve converges to the oracle solution."""
    shape = (11, 7, 3)
    glob = scenarios.block_case(shape[0], shape[1], shape[2] * nranks, h=0.1, tol=1e-6, max_iterations=800)
    P = glob.packing
    sK, sM = glob.scalars()
    single = _system(glob)
    assert _kernel(single).startswith(LATTICE)
    rng = np.random.Generator(np.random.PCG64(7))
    x = rng.uniform(-1, 1, P.dof_count).astype(np.float32)
    y1 = np.zeros_like(x)
    pcg.apply_keff(single, x, y1).value()
    y1 = y1.reshape(-1, 3)
    comm = shard.Comm.local(nranks)
    systems, shards, rhs, xs = [], [], [], []
    for r in range(nranks):
        case, node_global, begin = scenarios.slab_case_shape(shape, nranks, r, tol=1e-6)
        src = pcg.MatrixFreeSystem.from_packing(case.packing, case.materials, sK, sM, mode=_lib.MODE_FAST)
        sh = shard.build_shard(src, begin, r, node_global)
        s = sh.system(glob.materials, sK, sM)
        assert _kernel(s).startswith(LATTICE)
        gid = sh.node_global.astype(np.int64)
        own = sh.owned_nodes
        yl = np.zeros(3 * sh.local_nodes, np.float32)
        pcg.apply_keff(s, np.ascontiguousarray(x.reshape(-1, 3)[gid].reshape(-1)), yl).value()
        d = np.abs(yl.reshape(-1, 3)[:own].astype(np.float64) - y1[gid[:own]])
        assert np.max(d) <= 1e-6 * np.max(np.abs(y1))
        comm.attach(s, sh)
        systems.append(s)
        shards.append(sh)
        rhs.append(sh.local_dofs(case.static_rhs()))
        xs.append(np.zeros(3 * sh.local_nodes, np.float32))
    tel = shard.solve_pcg_group(systems, rhs, pcg.PcgSettings(800, 1e-6), xs).value()
    xg = np.zeros((P.node_count, 3), np.float32)
    for sh, xl in zip(shards, xs):
        xg[sh.node_global[: sh.owned_nodes].astype(np.int64)] = xl.reshape(-1, 3)[: sh.owned_nodes]
    comm.close()
    ref = oracle_system(P, glob.materials, sK, sM).solve_pcg(glob.static_rhs(), 800, 1e-6)
    assert tel.converged
    assert np.linalg.norm(xg.reshape(-1) - ref["x"]) <= 1e-4 * np.linalg.norm(ref["x"])
    n_ref = ref["telemetry"].iterations
    assert abs(tel.iterations - n_ref) <= max(3, n_ref // 10)


@pytest.mark.parametrize("mesh", ["lattice", "fan-groups"])
def test_fast_solve_run_to_run_deterministic(mesh, monkeypatch):
    """Every FAST reduction is folded in a fixed order (per-workgroup shares, then the consumer's fixed-order
    fold; no atomics): two solves on one handle and one on a fresh handle give the same bits."""
    if mesh == "fan-groups":
        monkeypatch.setenv("CWF_LATTICE", "0")
    case = scenarios.block_case(33, 9, 5, h=0.1, tol=1e-6, max_iterations=800)
    rhs = case.static_rhs()

    def solve(s):
        x = np.zeros_like(rhs)
        r = np.zeros_like(rhs)
        t = pcg.solve_pcg(s, rhs, pcg.PcgSettings(800, 1e-6), pcg.PcgVectors(x, r)).value()
        return t, x, r

    s = _system(case)
    runs = [solve(s), solve(s), solve(_system(case))]
    for t, x, r in runs[1:]:
        assert t.iterations == runs[0][0].iterations and t.residual_norm == runs[0][0].residual_norm
        assert np.array_equal(x.view(np.uint32), runs[0][1].view(np.uint32))
        assert np.array_equal(r.view(np.uint32), runs[0][2].view(np.uint32))


@pytest.mark.parametrize("name", ["33x9x5", "rollers", "c1", "rayleigh", "33x9x5-persistent", "hex", "hex-persistent"])
def test_fused_iteration_matches_two_kernel_loop(name, monkeypatch):
    """The fused one-launch iteration (lattice_fused.hip: r, z, p, x formed in the launch that applies K_eff; beta's
    numerator r_(j+1).z_(j+1) expanded through r_(j+1) = r_j - alpha Ap_j from the launch's own dots) against the
    reference loop's two kernels on the same handle geometry: the same solution to 1e-4 of the oracle's and an
    iteration count within 5% (tools/cg_variants.py emulates both in FAST arithmetic on the CPU)."""
    on = "1"
    if name.endswith("-persistent"):  # a grid of 16 workgroups walking every work item (C3's shape at small scale;
        monkeypatch.setenv("CWF_FUSED_MAXWG", "16")  # forced: by default a grid below the items runs two kernels)
        name, on = name.split("-")[0], "2"
    # hex: native hex8 cells (the deeper two-plane prefetch of the 27-point stencil), checked against the fp64 solve
    # of the oracle operator at tol 1e-6, its iteration counts at tol 1e-4. At 1e-6 this static
    # stiffness-dominated solve asks for a recurrence residual where the true residual of an fp32 x floors near
    # 3e-3 |rhs|, and there finite-precision CG's count follows each path's rounding (fused 216, two-kernel 310, hex
    # tiles 168-175, fp64 163: profiles/r05zh_hex_counts.log, tools/hex_counts.py; DESIGN.md section 9, a known fp32
    # floor effect); at the reachable 1e-4 the counts are compared as for tet4
    case = (scenarios.block_case(33, 9, 5, h=0.1, element="hex8", tol=1e-6, max_iterations=800) if name == "hex"
            else CASES[name]())
    rhs = case.static_rhs()
    mi = case.cfg.solver.max_iterations

    def solve(fused, tol):
        monkeypatch.setenv("CWF_FUSED", fused)
        s = _system(case)
        assert _kernel(s).startswith("k_pcg_lattice" if fused != "0" else "k_keff_lattice"), _kernel(s)
        x = np.zeros_like(rhs)
        r = np.zeros_like(rhs)
        t = pcg.solve_pcg(s, rhs, pcg.PcgSettings(mi, tol), pcg.PcgVectors(x, r)).value()
        assert t.converged
        # the r output is the residual of x (rhs - K x, Dirichlet rows 0) to fp32 accuracy
        return t, x, r

    (tf, xf, rf), (tk, xk, _) = solve(on, 1e-6), solve("0", 1e-6)
    if name == "hex":
        (tf4, _, _), (tk4, _, _) = solve(on, 1e-4), solve("0", 1e-4)
        print(f"hex8 fused / two-kernel iterations: tol 1e-4 {tf4.iterations} / {tk4.iterations}, "
              f"tol 1e-6 {tf.iterations} / {tk.iterations}")
        assert abs(tf4.iterations - tk4.iterations) <= max(3, tk4.iterations // 20), (tf4.iterations, tk4.iterations)
        P = case.packing
        ref = {"x": O.hex8_solve64(case.mesh.coords, case.mesh.tets, P.material_index, O.make_stiffness(30.0e9, 0.2),
                                   *case.scalars(), P.lumped_mass, P.bc_mask, rhs)}
        assert np.linalg.norm(xk - ref["x"]) <= 1e-4 * np.linalg.norm(ref["x"])
    else:
        assert abs(tf.iterations - tk.iterations) <= max(3, tk.iterations // 20), (tf.iterations, tk.iterations)
        ref = oracle_system(case.packing, case.materials, *case.scalars()).solve_pcg(rhs, mi, 1e-6)
    assert np.linalg.norm(xf - ref["x"]) <= 1e-4 * np.linalg.norm(ref["x"])
    assert tf.residual_norm <= 1e-6 * np.linalg.norm(rhs.astype(np.float64)) * 1.0001
    assert abs(np.linalg.norm(rf.astype(np.float64)) - tf.residual_norm) <= 1e-3 * tf.residual_norm


@pytest.mark.parametrize("element", ["tet4", "hex8"])
@pytest.mark.parametrize("schedule", ["fused", "fused-persistent", "two-kernel"])
@pytest.mark.parametrize("nranks", [2, 3])
def test_sharded_schedules_equal_one_handle(nranks, schedule, element, monkeypatch):
    """The slab shards (LOCAL communicator) against the one-handle solve of the same block in the same schedule:
    fused (one launch and one exchange per iteration; the ghost planes' r_j / p_j formed locally from the received
    Ap_(j-1)), the fused form walking its items persistently (CWF_FUSED=2 with a 16-workgroup grid: the
    persistent and shard instantiations together), and the two-kernel loop. The shards' owned x follows the one
    handle's after 1, 2, 3 and 20 iterations (the round-5 divergence at iteration 2 was a shard whose affine planes
    skipped the ghost stores; only the scalar folds' order differs: per-workgroup shares against rank totals), and
    the full solve converges in the same iteration count to within 3 (Kuhn tets; hex8 cells, the shard
    instantiations of the 27-point stencil's two-deep prefetch, to within 10%: the note on fp32 CG counts below
    the attainable residual in test_fused_iteration_matches_two_kernel_loop)."""
    monkeypatch.setenv("CWF_FUSED", {"fused": "1", "fused-persistent": "2", "two-kernel": "0"}[schedule])
    if schedule == "fused-persistent":
        monkeypatch.setenv("CWF_FUSED_MAXWG", "16")
    shape = (11, 7, 3)
    glob = scenarios.block_case(shape[0], shape[1], shape[2] * nranks, h=0.1, element=element, tol=1e-6,
                                max_iterations=800)
    P = glob.packing
    sK, sM = glob.scalars()
    rhs = glob.static_rhs()
    single = pcg.MatrixFreeSystem.from_packing(P, glob.materials, sK, sM, mode=_lib.MODE_FAST)
    comm = shard.Comm.local(nranks)
    systems, shards, rl = [], [], []
    for r in range(nranks):
        case, node_global, begin = scenarios.slab_case_shape(shape, nranks, r, element=element, tol=1e-6)
        src = pcg.MatrixFreeSystem.from_packing(case.packing, case.materials, sK, sM, mode=_lib.MODE_FAST)
        sh = shard.build_shard(src, begin, r, node_global)
        s = sh.system(glob.materials, sK, sM)
        comm.attach(s, sh)
        systems.append(s)
        shards.append(sh)
        rl.append(sh.local_dofs(case.static_rhs()))
    want = {"fused": 1, "fused-persistent": 1, "two-kernel": 0}[schedule]
    for its, tol in ((1, 1e-30), (2, 1e-30), (3, 1e-30), (20, 1e-30), (800, 1e-6)):
        x1 = np.zeros_like(rhs)
        t1 = pcg.solve_pcg(single, rhs, pcg.PcgSettings(its, tol), pcg.PcgVectors(x1, None)).value()
        xs = [np.zeros(3 * sh.local_nodes, np.float32) for sh in shards]
        ts = shard.solve_pcg_group(systems, rl, pcg.PcgSettings(its, tol), xs).value()
        assert _lib.load().cwf_hip_system_exchange_schedule(systems[0].handle()) == want
        xg = np.zeros((P.node_count, 3), np.float32)
        for sh, xl in zip(shards, xs):
            xg[sh.node_global[: sh.owned_nodes].astype(np.int64)] = xl.reshape(-1, 3)[: sh.owned_nodes]
        slack = 0 if tol < 1e-20 else 3 if element == "tet4" else max(3, t1.iterations // 10)
        assert abs(ts.iterations - t1.iterations) <= slack, (its, ts.iterations, t1.iterations)
        d = np.linalg.norm(xg.reshape(-1).astype(np.float64) - x1) / np.linalg.norm(x1.astype(np.float64))
        assert d <= (1e-5 if tol < 1e-20 else 1e-4), (schedule, its, d)
    assert t1.converged and ts.converged
    comm.close()


@pytest.mark.parametrize("nranks", [2, 3])
def test_thin_slab_shards_take_two_kernels(nranks, monkeypatch):
    """Slabs one cell thick (ranks owning a single node plane): the schedule vote keeps the two kernels for every rank
    (the fused launch's ghost-plane forms need owned planes on both sides of a brick's end planes: fused, these shards
    did not converge in 800 iterations where the one handle takes ~220), and the solve follows the one handle's."""
    monkeypatch.delenv("CWF_FUSED", raising=False)
    shape = (13, 9, 1)
    glob = scenarios.block_case(shape[0], shape[1], shape[2] * nranks, h=0.1, tol=1e-6, max_iterations=800)
    P = glob.packing
    sK, sM = glob.scalars()
    comm = shard.Comm.local(nranks)
    systems, shards, rl, xs = [], [], [], []
    for r in range(nranks):
        case, node_global, begin = scenarios.slab_case_shape(shape, nranks, r, tol=1e-6)
        src = pcg.MatrixFreeSystem.from_packing(case.packing, case.materials, sK, sM, mode=_lib.MODE_FAST)
        sh = shard.build_shard(src, begin, r, node_global)
        s = sh.system(glob.materials, sK, sM)
        comm.attach(s, sh)
        systems.append(s)
        shards.append(sh)
        rl.append(sh.local_dofs(case.static_rhs()))
        xs.append(np.zeros(3 * sh.local_nodes, np.float32))
    ts = shard.solve_pcg_group(systems, rl, pcg.PcgSettings(800, 1e-6), xs).value()
    assert _lib.load().cwf_hip_system_exchange_schedule(systems[0].handle()) == 0
    single = pcg.MatrixFreeSystem.from_packing(P, glob.materials, sK, sM, mode=_lib.MODE_FAST)
    x1 = np.zeros_like(glob.static_rhs())
    t1 = pcg.solve_pcg(single, glob.static_rhs(), pcg.PcgSettings(800, 1e-6), pcg.PcgVectors(x1, None)).value()
    assert ts.converged and t1.converged
    # (the one handle runs the resident solve: another schedule, so the counts agree to 10%, as across schedules)
    assert abs(ts.iterations - t1.iterations) <= max(3, t1.iterations // 10), (ts.iterations, t1.iterations)
    xg = np.zeros((P.node_count, 3), np.float32)
    for sh, xl in zip(shards, xs):
        xg[sh.node_global[: sh.owned_nodes].astype(np.int64)] = xl.reshape(-1, 3)[: sh.owned_nodes]
    assert np.linalg.norm(xg.reshape(-1) - x1) <= 1e-4 * np.linalg.norm(x1)
    comm.close()
