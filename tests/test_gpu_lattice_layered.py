"""Layered structured blocks on the GPU (lattice.hip, k_keff_lattice_layered): a Kuhn tet or native hex8 block
whose material is constant within every k-layer of cells applies K_eff as a per-plane stencil table (one table per
(material below, material above) pair) and, on its surface, each cell's pair blocks from its layer's table.

The contract is the lattice's (tests/test_gpu_lattice.py): K x within 2e-5 of the oracle relative to max |row|,
solves at tol 1e-6 converged within 1e-4 (relative) of the oracle's solution and its iteration count +-10%. Layered
handles carry no class preconditioner, so they always run the two-kernel loop (never the fused or resident solve).

Cases are named by cells nx x ny x nz and the material per cell layer; the three materials are
scenarios.LAYER_MATERIALS (E = 30e9 / 3e9 / 12e9, nu = 0.2 / 0.3 / 0.25, rho = 2500 / 1800 / 2200)."""
import json
import os

import numpy as np
import pytest

import oracle as O
from cwf import _lib, meshgen, pcg, run, scenarios, shard
from cwf.stepper import Stepper
from helpers import oracle_system

pytestmark = pytest.mark.gpu

LAYERED = "k_keff_lattice_layered"
SHAPES = {
    "7x5x6": ((7, 5, 6), [0, 0, 1, 1, 2, 0]),
    "5x4x4": ((5, 4, 4), [0, 1, 0, 1]),  # every interior plane an interface
    "12x10x9": ((12, 10, 9), [0, 0, 0, 1, 1, 1, 2, 2, 2]),
    # bricks cut in x, y and k; with CWF_LAT_L = 3 the interfaces at node planes 2, 5 and 7 fall on the first, a
    # middle and the last plane of a chunk
    "40x19x9": ((40, 19, 9), [0, 0, 1, 1, 1, 2, 2, 0, 0]),
}

def _case(name, element="tet4", **kw):
    shape, layers = SHAPES[name]
    kw.setdefault("tol", 1e-6)
    kw.setdefault("max_iterations", 1500)
    return scenarios.layered_case(*shape, layers, element=element, **kw)


_cache = {}


def case_of(name, element="tet4"):
    """Each case (and its oracle solve, below) built once per session and left unchanged."""
    key = (name, element)
    if key not in _cache:
        _cache[key] = _case(name, element)
    return _cache[key]


def _system(case, mode=_lib.MODE_FAST):
    sK, sM = case.scalars()
    return pcg.MatrixFreeSystem.from_packing(case.packing, case.materials, sK, sM, mode=mode)


def _kernel(s):
    return (_lib.load().cwf_hip_system_keff_kernel(s.handle()) or b"").decode()


def _stiffness(case):
    return np.concatenate([np.asarray(m.stiffness, np.float64).reshape(-1) for m in case.materials])


def _apply_err(case, s, seed=3):
    P = case.packing
    sK, sM = case.scalars()
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.uniform(-1, 1, P.dof_count).astype(np.float32)
    y = np.zeros_like(x)
    pcg.apply_keff(s, x, y).value()
    if case.mesh.tets.shape[1] == 8:
        ref = O.hex8_apply(case.mesh.coords, case.mesh.tets, P.material_index, _stiffness(case), sK, sM,
                           P.lumped_mass, P.bc_mask, x).astype(np.float64)
    else:
        ref = oracle_system(P, case.materials, sK, sM).apply_keff(x).astype(np.float64)
    mask = np.repeat(P.bc_mask, 3) & np.tile(np.array([1, 2, 4], np.uint32), P.node_count)
    assert np.array_equal(y[mask != 0], x[mask != 0])  # Dirichlet rows pass x through
    err = float(np.max(np.abs(y - ref)) / np.max(np.abs(ref)))
    print(f"{case.name}: apply error {err:.3e} of max |row| ({_kernel(s)})")
    return err


@pytest.mark.parametrize("element", ["tet4", "hex8"])
@pytest.mark.parametrize("name", ["7x5x6", "5x4x4", "40x19x9"])
def test_layered_kernel_is_chosen(name, element):
    s = _system(case_of(name, element))
    kind = "LatHex" if element == "hex8" else "LatKuhn"
    assert _kernel(s).startswith(f"{LAYERED}<1, false, {kind},"), _kernel(s)
    # a one-material block of the same shape keeps today's kernels (the resident / fused / two-kernel stencil)
    shape = SHAPES[name][0]
    plain = _system(scenarios.block_case(*shape, h=0.1, element=element, tol=1e-6))
    assert _kernel(plain).startswith(("k_pcg_resident", "k_pcg_lattice", "k_keff_lattice<")), _kernel(plain)


@pytest.mark.parametrize("element", ["tet4", "hex8"])
@pytest.mark.parametrize("name", ["7x5x6", "5x4x4"])
def test_layered_apply_close(name, element):
    case = case_of(name, element)
    assert _apply_err(case, _system(case)) <= 2e-5


@pytest.mark.parametrize("element", ["tet4", "hex8"])
@pytest.mark.parametrize("L", ["2", "3", "64"])
def test_layered_work_item_lengths(L, element, monkeypatch):
    monkeypatch.setenv("CWF_LAT_L", L)
    case = case_of("40x19x9", element)
    s = _system(case)
    assert _kernel(s).startswith(LAYERED)
    assert _apply_err(case, s, seed=11) <= 2e-5


def test_layered_permuted_node_order():
    shape, layers = SHAPES["7x5x6"]
    case = scenarios.layered_case(*shape, layers, permute=True, tol=1e-6)
    s = _system(case)
    assert _kernel(s).startswith(LAYERED), _kernel(s)
    assert _apply_err(case, s) <= 2e-5


def test_layered_traffic_counts_the_tables():
    case = case_of("7x5x6")
    s = _system(case)
    a, b = np.zeros(1, np.uint64), np.zeros(1, np.uint64)
    assert _lib.load().cwf_hip_system_keff_traffic(s.handle(), _lib.ptr(a), _lib.ptr(b)) == 0
    N = case.packing.node_count
    classes, mats = 5, 3  # (0,0) (0,1) (1,1) (1,2) (2,0); three materials
    assert int(a[0]) == N * 52 + 36 * (classes * 15 + mats * 46) + 4 * 7


def _oracle_solve(name):
    key = ("solve", name)
    if key not in _cache:
        case = case_of(name)
        o = oracle_system(case.packing, case.materials, *case.scalars())
        _cache[key] = o.solve_pcg(case.static_rhs(), 1500, 1e-6)
    return _cache[key]


@pytest.mark.parametrize("name", ["7x5x6", "12x10x9", "40x19x9"])
def test_layered_solve_close(name):
    case = case_of(name)
    s = _system(case)
    assert _kernel(s).startswith(LAYERED)
    rhs = case.static_rhs()
    x = np.zeros_like(rhs)
    t = pcg.solve_pcg(s, rhs, pcg.PcgSettings(1500, 1e-6), pcg.PcgVectors(x, np.zeros_like(rhs))).value()
    ref = _oracle_solve(name)
    n_ref = ref["telemetry"].iterations
    err = float(np.linalg.norm(x - ref["x"]) / np.linalg.norm(ref["x"]))
    print(f"{name}: |x - x_oracle| / |x_oracle| = {err:.3e}, iterations {t.iterations} (oracle {n_ref})")
    assert t.converged and ref["telemetry"].converged
    assert err <= 1e-4
    assert abs(t.iterations - n_ref) <= max(3, n_ref // 10)


def test_layered_stepper_steps():
    """Three Newmark steps with Rayleigh damping: the beta-damping SpMV runs the layered apply form (MODE 0), the
    solves the PCG form. Against the PARITY stepper (bit-exact with the oracle's), as the one-material lattice."""
    shape, layers = SHAPES["12x10x9"]
    case = scenarios.layered_case(*shape, layers, xi=0.05, w=(10.0, 100.0), tol=1e-6, max_iterations=1500)
    P = case.packing
    ref = Stepper(P, case.materials, case.rayleigh, case.cfg.solver, case.cfg.time, mode=_lib.MODE_PARITY)
    fast = Stepper(P, case.materials, case.rayleigh, case.cfg.solver, case.cfg.time, mode=_lib.MODE_FAST)
    assert _kernel(fast.system).startswith(LAYERED)
    for k in range(3):
        tr = ref.step(0.01 * k).value()
        tf = fast.step(0.01 * k).value()
        assert tf.pcg.converged and tr.pcg.converged
        assert abs(tf.pcg.iterations - tr.pcg.iterations) <= max(3, tr.pcg.iterations // 10)
    for what in (Stepper.DISPLACEMENT, Stepper.VELOCITY):
        ur, uf = ref.get_state(what), fast.get_state(what)
        err = float(np.linalg.norm(uf - ur) / np.linalg.norm(ur))
        print(f"layered stepper state {what}: {err:.3e}")
        assert err <= 1e-4


@pytest.mark.parametrize("cut", [4, 5, 3], ids=["at-interface", "inside-layer", "one-material-shard"])
def test_layered_slab_shards(cut):
    """Two LOCAL slab shards of 12x10x9 [0,0,0,1,1,1,2,2,2]; rank 0 owns node planes [0, cut). cut = 4: the interface
    plane 3 is rank 0's last owned plane and its ghost plane lies in the next material; cut = 5: inside the middle
    layer. Each shard detects its own layers from its local desc (owned planes and the ghost plane index the local
    plane-class array) and runs the layered kernel; before attach its owned rows are the one handle's, and the
    attached solve follows the one-handle solve. cut = 3 (the interface plane is rank 1's first owned plane): rank 0's
    cells are all of material 0, so that shard is a one-material lattice and keeps today's kernels next to the layered
    rank 1."""
    shape, layers = SHAPES["12x10x9"]
    glob = case_of("12x10x9")
    P = glob.packing
    sK, sM = glob.scalars()
    single = _system(glob)
    rng = np.random.Generator(np.random.PCG64(7))
    x = rng.uniform(-1, 1, P.dof_count).astype(np.float32)
    y1 = np.zeros_like(x)
    pcg.apply_keff(single, x, y1).value()
    y1 = y1.reshape(-1, 3)
    planes = [0, cut, shape[2] + 1]
    comm = shard.Comm.local(2)
    systems, shards, rhs, xs = [], [], [], []
    for r in range(2):
        case, node_global, begin = scenarios.layered_slab_case(shape, layers, planes, r, tol=1e-6)
        src = pcg.MatrixFreeSystem.from_packing(case.packing, case.materials, sK, sM, mode=_lib.MODE_FAST)
        sh = shard.build_shard(src, begin, r, node_global)
        s = sh.system(glob.materials, sK, sM)
        want = ("k_pcg_resident", "k_pcg_lattice", "k_keff_lattice<") if (cut, r) == (3, 0) else (LAYERED,)
        assert _kernel(s).startswith(want), _kernel(s)
        gid = sh.node_global.astype(np.int64)
        own = sh.owned_nodes
        yl = np.zeros(3 * sh.local_nodes, np.float32)
        pcg.apply_keff(s, np.ascontiguousarray(x.reshape(-1, 3)[gid].reshape(-1)), yl).value()
        d = np.abs(yl.reshape(-1, 3)[:own].astype(np.float64) - y1[gid[:own]])
        assert np.max(d) <= 1e-6 * np.max(np.abs(y1))
        comm.attach(s, sh)
        assert _kernel(s).startswith(want), _kernel(s)
        systems.append(s)
        shards.append(sh)
        rhs.append(sh.local_dofs(case.static_rhs()))
        xs.append(np.zeros(3 * sh.local_nodes, np.float32))
    tel = shard.solve_pcg_group(systems, rhs, pcg.PcgSettings(1500, 1e-6), xs).value()
    xg = np.zeros((P.node_count, 3), np.float32)
    for sh, xl in zip(shards, xs):
        xg[sh.node_global[: sh.owned_nodes].astype(np.int64)] = xl.reshape(-1, 3)[: sh.owned_nodes]
    comm.close()
    x1 = np.zeros_like(x)
    t1 = pcg.solve_pcg(single, glob.static_rhs(), pcg.PcgSettings(1500, 1e-6), pcg.PcgVectors(x1, None)).value()
    assert tel.converged and t1.converged
    err = float(np.linalg.norm(xg.reshape(-1) - x1) / np.linalg.norm(x1))
    print(f"cut at plane {cut}: shards vs one handle {err:.3e}, iterations {tel.iterations} / {t1.iterations}")
    assert err <= 1e-4
    assert abs(tel.iterations - t1.iterations) <= max(3, t1.iterations // 10)


YAML = """mesh:
  path: layered.msh
materials:
  - name: concrete
    E: 3.0e10
    nu: 0.2
    rho: 2500.0
  - name: soil
    E: 3.0e9
    nu: 0.3
    rho: 1800.0
assignments:
  - group: SLAB
    material: concrete
  - group: GROUND
    material: soil
damping:
  xi: 0.02
  w1: 5.0
  w2: 50.0
time:
  dt: 0.01
  adaptive: false
solver:
  type: pcg
  preconditioner: block_jacobi
  tol_runtime: 1.0e-6
  tol_pause: 1.0e-6
  max_iters: 1500
precision:
  vectors: fp32
  reductions: fp64
loads:
  gravity: [0.0, 0.0, -9.81]
  points:
    - group: TIP
      value: [0.0, 0.0, -500.0]
dirichlet:
  fixes:
    - group: FIXED
      dof: [x, y, z]
output:
  vtu_stride: 1
  probes: [0, 5]
"""


def test_layered_scenario_from_yaml_and_gmsh(tmp_path):
    """A two-material scenario (a concrete slab on soil) from YAML plus a multi-volume Gmsh file through cwf.run in
    FAST mode: the layered kernel runs, and u after 2 steps is within 1e-4 (relative) of the PARITY run's."""
    tm, emat = meshgen.layered_block(8, 5, 5, [1, 1, 1, 0, 0], 0.1)
    meshgen.write_gmsh(tm, str(tmp_path / "layered.msh"), node_groups=["FIXED", "TIP"],
                       volumes=(["SLAB", "GROUND"], emat))
    y = str(tmp_path / "layered.yaml")
    with open(y, "w") as f:
        f.write(YAML)
    lines = []
    summary = run.run_scenario(y, 2, str(tmp_path / "out"), _lib.MODE_FAST, log=lines.append)
    assert summary["steps"] == 2 and all(json.loads(l)["converged"] for l in lines)
    assert os.path.exists(tmp_path / "out" / "vtu" / "frame_00001.vtu")
    cfg, m, P, mats = run.load_scenario(y)
    assert np.array_equal(P.material_index, emat)
    from cwf.physics import compute_rayleigh

    u = {}
    for mode in (_lib.MODE_FAST, _lib.MODE_PARITY):
        st = Stepper(P, mats, compute_rayleigh(cfg.damping), cfg.solver, cfg.time, mode=mode)
        if mode == _lib.MODE_FAST:
            assert _kernel(st.system).startswith(LAYERED), _kernel(st.system)
        t = 0.0
        for _ in range(2):
            tel = st.step(t).value()
            assert tel.pcg.converged
            t = tel.simulation_time + tel.time_step
        u[mode] = st.get_state(Stepper.DISPLACEMENT).astype(np.float64)
        st.close()
        st.system.close()
    err = float(np.linalg.norm(u[_lib.MODE_FAST] - u[_lib.MODE_PARITY]) / np.linalg.norm(u[_lib.MODE_PARITY]))
    print(f"layered scenario: |u_fast - u_parity| / |u_parity| after 2 steps = {err:.3e}")
    assert err <= 1e-4
