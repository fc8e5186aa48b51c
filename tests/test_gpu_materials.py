"""Anisotropic and mixed materials on every kernel path, against the CPU oracle (which folds the full 6 x 6 row).

Every other GPU test feeds make_stiffness_matrix(E, nu): three distinct numbers and 24 structural zeros, behind which
a swapped table slot, a transposed index map or a wrong row picked by a material id cannot be seen, and with which
the ISO = false instantiations never run. The materials and element assignments are tests/materials_common.py's:

  ortho             [ORTHO]              ISO = true kernels, every slot of the 12-entry table its own value
  rot               [ROT]                ISO = false, one material (MONO = true fan groups)
  mixed-thirds      [ISO, ORTHO, ROT]    ISO = false, MONO = false; material by thirds of the block along x
  mixed-scattered   [ISO, ORTHO, ROT]    the same, material e % 3 (almost every fan cut to one or two tets)
  many18-scattered  ROT (1 + 0.05 k)     18 materials: two lie past the 16 rows of the LDS tables

Contracts, unchanged from the files named: PARITY bit for bit (test_gpu_parity.py, test_gpu_post.py); the fp64
residual within 4096 eps64 (|K||x| + |b|) of the dense product and the refined solve to 1e-10 (test_gpu_refine.py);
FAST apply within 2e-5 of max |row| and solves at 1e-6 converged, within 1e-4 of the oracle's solution, its iteration
count +-10% (test_gpu_parity.py, test_gpu_create_paths.py, test_gpu_lattice*.py, test_hex8.py). Every test prints the
kernel the handle reports and the figure it asserts on."""
import functools
import re

import numpy as np
import pytest

import materials_common as MC
import oracle as O
import test_gpu_refine as R
from cwf import _lib, pcg, post, scenarios, shard
from cwf.stepper import Stepper
from helpers import assert_bitwise, bits, check_step_against_parity, oracle_system
from test_gpu_create_paths import CASES as CREATE_CASES, KNOBS as CREATE_KNOBS
from test_gpu_lattice_layered import LAYERED, SHAPES as LAYERED_SHAPES
from test_hex8 import hex_case

pytestmark = pytest.mark.gpu

KW = dict(xi=0.05, w=(10.0, 100.0), tol=1e-6, max_iterations=600)
MESHES = {
    # 336 nodes, 1,260 tets: two PARITY node tiles, two k_derived_nodes workgroups, several FAST tiles at every size
    "jitter": lambda: scenarios.block_case(7, 6, 5, h=0.1, jitter=True, **KW),
    "block": lambda: scenarios.block_case(8, 3, 4, h=0.1, **KW),
    "block-hex": lambda: scenarios.block_case(8, 3, 4, h=0.1, element="hex8", **KW),
    "rollers": lambda: scenarios.roller_case(12, 10, 7, **KW),
    "hex": lambda: hex_case(6, 4, 3, **KW),
}
SETS = {
    "ortho": ([MC.ORTHO], None),
    "rot": ([MC.ROT], None),
    "mixed-thirds": ([MC.ISO, MC.ORTHO, MC.ROT], "thirds"),
    "mixed-scattered": ([MC.ISO, MC.ORTHO, MC.ROT], "scattered"),
    "many18-scattered": (MC.many(18), "scattered"),
}
STRATA = [MC.ISO, MC.ROT, MC.ORTHO]
LATTICE = ("k_pcg_resident", "k_pcg_lattice", "k_keff_lattice<")
SETTINGS = pcg.PcgSettings(600, 1e-6)


# ---- cases and references, each built once per session and left unchanged --------------------------------------------
@functools.lru_cache(maxsize=None)
def base_case(mesh):
    return MESHES[mesh]()


@functools.lru_cache(maxsize=None)
def setup(mesh, sname):
    base = base_case(mesh)
    mats, how = SETS[sname]
    index = {None: lambda: None, "thirds": lambda: MC.thirds(base),
             "scattered": lambda: MC.scattered(base, len(mats))}[how]()
    return MC.MaterialCase(base, mats, index, name=f"{mesh}/{sname}")


def is_hex(c):
    return c.mesh.tets.shape[1] == 8


@functools.lru_cache(maxsize=None)
def oracle(mesh, sname):
    c = setup(mesh, sname)
    return oracle_system(c.packing, c.materials, *c.scalars())


def ref_apply(c, x, tet_oracle=None):
    P = c.packing
    if is_hex(c):
        return O.hex8_apply(c.mesh.coords, c.mesh.tets, P.material_index, c.stiffness, *c.scalars(), P.lumped_mass,
                            P.bc_mask, x).astype(np.float64)
    o = tet_oracle or oracle_system(P, c.materials, *c.scalars())
    return o.apply_keff(x).astype(np.float64)


def ref_solve(c, tet_oracle=None):
    """-> (x, iterations or None): the pinned f32 PCG on tets; the fp64 solve of the fp64 hex8 operator, whose
    iteration count (to 1e-11) is no reference for a solve to 1e-6."""
    P = c.packing
    if is_hex(c):
        return O.hex8_solve64(c.mesh.coords, c.mesh.tets, P.material_index, c.stiffness, *c.scalars(), P.lumped_mass,
                              P.bc_mask, c.static_rhs()), None
    o = tet_oracle or oracle_system(P, c.materials, *c.scalars())
    ref = o.solve_pcg(c.static_rhs(), 600, 1e-6, history=True)
    assert ref["telemetry"].converged
    return ref, int(ref["telemetry"].iterations)


@functools.lru_cache(maxsize=None)
def oracle_solve(mesh, sname):
    c = setup(mesh, sname)
    return ref_solve(c, None if is_hex(c) else oracle(mesh, sname))


def system(c, mode=_lib.MODE_FAST, keep_node_order=False, scalars=None):
    P = c.packing
    sK, sM = scalars or c.scalars()
    coords = P.position64 if getattr(P, "position64", None) is not None else P.position0
    return pcg.MatrixFreeSystem(P.connectivity, P.gradients, P.volume, P.material_index, c.materials, P.lumped_mass,
                                P.bc_mask, P.node_count, P.element_count, P.dof_count, sK, sM, P.reduction_block,
                                P.reduction_partials, (P.offsets, P.element_indices, P.local_indices), mode, 0, coords,
                                keep_node_order=keep_node_order)


def kernel(s):
    return (_lib.load().cwf_hip_system_keff_kernel(s.handle()) or b"").decode()


def same_bits(a, b, what):
    """assert_bitwise, with the count it asserts on printed first."""
    a, b = np.asarray(a), np.asarray(b)
    n = int(np.count_nonzero(bits(a) != bits(b))) if a.shape == b.shape else -1
    print(f"{what}: {n} of {a.size} words differ from the oracle")
    assert_bitwise(a, b, what)


def random_x(c, seed=3):
    return np.random.Generator(np.random.PCG64(seed)).uniform(-1, 1, c.packing.dof_count).astype(np.float32)


def fast_apply_check(c, s, ref, what):
    """max |y - ref| <= 2e-5 max |ref|; Dirichlet rows pass x through."""
    P = c.packing
    x = random_x(c)
    y = np.zeros_like(x)
    pcg.apply_keff(s, x, y).value()
    r = ref(x)
    err = float(np.max(np.abs(y - r)) / np.max(np.abs(r)))
    print(f"{what}: {kernel(s)}  apply error {err:.3e} of max |row|")
    assert err <= 2e-5
    mask = np.repeat(P.bc_mask, 3) & np.tile(np.array([1, 2, 4], np.uint32), P.node_count)
    assert np.array_equal(y[mask != 0], x[mask != 0])


def fast_solve_check(c, s, ref, what):
    """converged, |x - x_ref| <= 1e-4 |x_ref|, iterations within max(3, n_ref // 10) where there is an n_ref."""
    xr, n_ref = ref
    xr = xr["x"] if isinstance(xr, dict) else xr
    rhs = c.static_rhs()
    x = np.zeros_like(rhs)
    t = pcg.solve_pcg(s, rhs, SETTINGS, pcg.PcgVectors(x, np.zeros_like(rhs))).value()
    err = float(np.linalg.norm(x - xr) / np.linalg.norm(xr))
    print(f"{what}: {kernel(s)}  |x - x_ref| / |x_ref| = {err:.3e}, iterations {t.iterations} (reference {n_ref})")
    assert t.converged
    assert err <= 1e-4
    if n_ref is not None:
        assert abs(t.iterations - n_ref) <= max(3, n_ref // 10)


# ---- PARITY: bit for bit against the oracle --------------------------------------------------------------------------
PARITY_CASES = [("jitter", s) for s in SETS] + [("block", "rot")]


def parity_kernel_prefix(sname):
    return "k_keff_parity_tile<true," if sname == "ortho" else "k_keff_parity_tile<false,"


@pytest.mark.parametrize("mesh,sname", PARITY_CASES)
def test_parity_apply_keff_and_block_jacobi(mesh, sname):
    """k_keff_parity_tile<ISO, ...> (the apply form) and the fp64 block-Jacobi builder."""
    c, o = setup(mesh, sname), oracle(mesh, sname)
    s = system(c, _lib.MODE_PARITY)
    print(f"{c.name}: {kernel(s)}")
    assert kernel(s).startswith(parity_kernel_prefix(sname)), kernel(s)
    x = random_x(c)
    y = np.zeros_like(x)
    pcg.apply_keff(s, x, y).value()
    same_bits(y, o.apply_keff(x), f"{c.name} apply_keff")
    inv = np.zeros(9 * c.packing.node_count, np.float32)
    pcg.build_block_jacobi_inverse(s, None, inv).value()
    same_bits(inv, o.block_jacobi(), f"{c.name} block_jacobi")
    s.close()


@pytest.mark.parametrize("mesh,sname", PARITY_CASES)
def test_parity_solve(mesh, sname):
    """k_keff_parity_tile's PCG forms: x, r, the telemetry and the fp64 residual history."""
    c = setup(mesh, sname)
    ref, _ = oracle_solve(mesh, sname)
    s = system(c, _lib.MODE_PARITY)
    rhs = c.static_rhs()
    x, r = np.zeros_like(rhs), np.zeros_like(rhs)
    t = pcg.solve_pcg(s, rhs, SETTINGS, pcg.PcgVectors(x, r)).value()
    rt = ref["telemetry"]
    print(f"{c.name}: {kernel(s)}  iterations {t.iterations} (oracle {rt.iterations}), |r| {t.residual_norm!r} "
          f"(oracle {rt.residual_norm!r})")
    assert (t.iterations, t.converged) == (rt.iterations, bool(rt.converged))
    assert (t.residual_norm, t.rhs_norm, t.alpha_last, t.beta_last) == (rt.residual_norm, rt.rhs_norm, rt.alpha_last,
                                                                          rt.beta_last)
    same_bits(x, ref["x"], f"{c.name} x")
    same_bits(r, ref["r"], f"{c.name} r")
    assert np.array_equal(pcg.residual_history(s), ref["history"])
    s.close()


@pytest.mark.parametrize("mesh,sname", PARITY_CASES)
def test_parity_stepper_three_steps(mesh, sname):
    """Three Newmark steps with Rayleigh damping (xi = 0.05, w = 10, 100): the beta-damping apply and the solves."""
    c = setup(mesh, sname)
    P = c.packing
    st = Stepper(P, c.materials, c.rayleigh, c.cfg.solver, c.cfg.time)
    ray = c.rayleigh
    assert ray.beta > 0.0
    o = oracle_system(P, c.materials, *c.scalars())  # its own system: the oracle stepper rewrites the scalars
    ost = O.Stepper(o, P.external_force, P.bc_value, (ray.alpha, ray.beta), c.cfg.solver.runtime_tolerance,
                    c.cfg.solver.pause_tolerance, c.cfg.solver.max_iterations, c.cfg.time.initial_dt)
    for k in range(3):
        t = st.step(k * 0.01).value()
        rt = ost.step(k * 0.01)
        print(f"{c.name} step {k}: iterations {t.pcg.iterations} (oracle {rt.pcg.iterations})")
        assert t.pcg.converged
        assert t.pcg.iterations == rt.pcg.iterations and t.pcg.residual_norm == rt.pcg.residual_norm
    for which, ref, what in ((Stepper.DISPLACEMENT, ost.u, "u"), (Stepper.VELOCITY, ost.v, "v"),
                             (Stepper.ACCELERATION, ost.a, "a")):
        same_bits(st.get_state(which), ref, f"{c.name} {what}")
    st.close()
    st.system.close()


@pytest.mark.parametrize("mode", [_lib.MODE_PARITY, _lib.MODE_FAST], ids=["parity-handle", "fast-handle"])
@pytest.mark.parametrize("mesh,sname", PARITY_CASES)
def test_derived_fields(mesh, sname, mode):
    """k_derived_elements / k_derived_nodes<ISO, false> over both handle layouts (a FAST handle of the jittered mesh
    is renumbered), from a random u of +-1e-3."""
    c = setup(mesh, sname)
    P = c.packing
    u = np.random.Generator(np.random.PCG64(21)).uniform(-1e-3, 1e-3, P.dof_count).astype(np.float32)
    s = system(c, mode, scalars=(1.0, 0.0))
    d = post.compute_derived_fields(P, c.materials, system=s, displacement=u)
    el, nd = oracle_system(P, c.materials, 1.0, 0.0).derived_fields(u)
    print(f"{c.name}: k_derived_elements / k_derived_nodes<{'true' if sname == 'ortho' else 'false'}, false> on a "
          f"{kernel(s)} handle")
    same_bits(d.elements, el, f"{c.name} element fields")
    same_bits(d.nodes, nd, f"{c.name} node fields")
    s.close()


# ---- the fp64 residual and the refined solve (refine.hip) ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def refine_case(sname):
    """test_gpu_refine.py's jittered 12 x 3 x 4 block (260 nodes: two node tiles, the second of 4 nodes) and load."""
    base = R.mesh_case("jitter")
    mats, how = SETS[sname]
    return MC.MaterialCase(base, mats, MC.thirds(base) if how == "thirds" else None, name=f"refine-jitter/{sname}")


@functools.lru_cache(maxsize=None)
def refine_dense(sname, newmark):
    """test_gpu_refine.dense with the set's materials: K_eff assembled densely in fp64 from the packed f32 records."""
    c = refine_case(sname)
    P = c.packing
    D = P.dof_count
    packed = O.Packed(P.node_count, P.element_count, P.connectivity, P.gradients, P.volume, P.material_index,
                      P.lumped_mass64, P.lumped_mass, P.offsets, P.element_indices, P.local_indices)
    g64 = np.asarray(P.gradients).reshape(P.element_count, -1)[:, :12].astype(np.float64)
    K = O.dense_assemble(packed, c.mesh.tets, g64, P.volume.astype(np.float64), c.stiffness).reshape(D, D)
    sK, sM = R.scalars_of(c, newmark)
    K *= sK
    K[np.diag_indices(D)] += sM * np.repeat(P.lumped_mass.astype(np.float64), 3)
    free = (np.repeat(P.bc_mask, 3) & np.tile(R.DOF_BITS, P.node_count)) == 0
    b = c.static_rhs().astype(np.float64)
    for a in (K, free, b):
        a.setflags(write=False)
    return dict(K=K, free=free, b=b)


@pytest.mark.parametrize("layout", ["parity-compact", "parity-strip", "fast"])
@pytest.mark.parametrize("sname", ["rot", "mixed-thirds"])
def test_refine_residual_against_dense_product(sname, layout, monkeypatch):
    """k_refine_residual<false> as test_gpu_refine.test_residual_against_dense_product checks it (random fp64 x and b,
    Newmark scalars, 4096 eps64 (|K_eff||x| + |b|) per component), over both PARITY tile layouts and a FAST handle; on
    the PARITY handles f32(-r) of b = 0 is also the handle's own apply_keff bit for bit."""
    monkeypatch.delenv("CWF_PARITY_TILES", raising=False)
    if layout == "parity-strip":
        monkeypatch.setenv("CWF_PARITY_TILES", "strip")
    c, d = refine_case(sname), refine_dense(sname, True)
    free = d["free"]
    D = free.size
    rng = np.random.Generator(np.random.PCG64(11))
    x = rng.uniform(-1.0, 1.0, D) * 1e-3
    b = rng.uniform(-1.0, 1.0, D) * 1e6
    mode = _lib.MODE_FAST if layout == "fast" else _lib.MODE_PARITY
    s = system(c, mode, scalars=R.scalars_of(c, True))
    kern = kernel(s)
    if mode == _lib.MODE_PARITY:
        want = "k_keff_parity_tile<false, false, " + ("true, false>" if layout == "parity-strip" else "false, true>")
        assert kern == want, kern
    r_dev, norm = pcg.residual_f64(s, b, x).value()
    xm = np.where(free, x, 0.0)
    r_np = np.where(free, b - d["K"] @ xm, 0.0)
    scale = np.abs(d["K"]) @ np.abs(xm) + np.abs(b)
    ratio = float(np.max(np.abs(r_dev - r_np)[free] / (R.EPS64 * scale[free])))
    print(f"{c.name} {layout}: k_refine_residual<false> on a {kern} handle, worst |r_dev - r_np| / (eps64 (|K||x| + "
          f"|b|)) = {ratio:.2f}")
    assert np.all(r_dev[~free] == 0.0)
    assert np.all(np.abs(r_dev - r_np) <= 4096 * R.EPS64 * scale)
    assert abs(norm - np.linalg.norm(r_dev)) <= 1e-14 * norm
    if mode == _lib.MODE_PARITY:
        x32 = random_x(c, 12)
        y = np.zeros_like(x32)
        pcg.apply_keff(s, x32, y).value()
        r, _ = pcg.residual_f64(s, np.zeros(D), x32.astype(np.float64)).value()
        same_bits((-r).astype(np.float32)[free], y[free], f"{c.name} {layout} f32(-r) against apply_keff")
    s.close()


def test_refined_solve_reaches_1e_10():
    """solve_refined on the `rot` FAST handle (fan groups, ISO = false): converged at 1e-10 on its own fp64 residual,
    and the residual of the returned x evaluated by numpy within test_gpu_refine's 2e-10."""
    c, d = refine_case("rot"), refine_dense("rot", False)
    b, free = d["b"], d["free"]
    A = d["K"][np.ix_(free, free)]
    xr = np.zeros(b.size)
    xr[free] = np.linalg.solve(A, b[free])
    floor = float(np.linalg.norm(b[free] - A @ xr[free]) / np.linalg.norm(b[free]))
    s = system(c, _lib.MODE_FAST, scalars=(1.0, 0.0))
    res = pcg.solve_refined(s, b, pcg.RefineSettings(relative_tolerance=1e-10))
    assert res.has_value(), res.error()
    x, t = res.value().solution, res.value().telemetry
    true = R.true_residual(d, b, x)
    err = float(np.linalg.norm(x - xr) / np.linalg.norm(xr))
    print(f"{c.name}: {kernel(s)}  dense floor {floor:.2e}, outer {t.outer_iterations} inner {t.inner_iterations}, "
          f"device residual {t.residual_norm / t.rhs_norm:.2e}, numpy residual {true:.2e}, error {err:.2e}")
    assert kernel(s).startswith("k_keff_groups_pipe<false,"), kernel(s)
    assert t.converged and not t.stagnated
    assert t.residual_norm <= 1e-10 * t.rhs_norm
    assert true <= 2e-10
    assert np.all(x[~free] == 0.0)
    s.close()


# ---- FAST, general paths on the jittered mesh ------------------------------------------------------------------------
GROUPS_128 = ("jitter", "", {"CWF_GROUP_NT": "128"}, ("k_keff_groups_pipe",), "")
PATHS = {"fan-groups": CREATE_CASES["fan-groups"], "fan-groups-128": GROUPS_128,
         "tiles-pipe-knob": CREATE_CASES["tiles-pipe-knob"], "records-knob": CREATE_CASES["records-knob"],
         "one-tile-per-workgroup": CREATE_CASES["one-tile-per-workgroup"],
         "caller-order-flag": CREATE_CASES["caller-order-flag"]}
FOUR = ["ortho", "rot", "mixed-thirds", "mixed-scattered"]
GENERAL = ([(p, s) for p in ("fan-groups", "fan-groups-128") for s in FOUR] +
           [(p, s) for p in ("tiles-pipe-knob", "records-knob", "one-tile-per-workgroup")
            for s in FOUR + ["many18-scattered"]] + [("caller-order-flag", "mixed-thirds")])
GENERAL_KNOBS = sorted(set(CREATE_KNOBS) | {"CWF_GROUP_NT"})
# material e % 3 cuts the same-material fans (groups.cpp walk_fan) to one or two tets each: below the 3 tets per group
# fan_groups_usable asks for, create gives the mesh the pipelined per-tet tiles instead, by design (abi.cpp)
SHORT_FANS = {"mixed-scattered"}


@pytest.mark.parametrize("path,sname", GENERAL)
def test_fast_general_path(path, sname, monkeypatch):
    """k_keff_groups_pipe<ISO, false, 1, NT, MONO>, k_keff_tiles_pipe<ISO, 128 | 256>, k_keff_tiles<ISO>: the path by
    test_gpu_create_paths' knobs, the apply and the solve against the oracle. The solves on k_keff_tiles are the
    suite's only ones on that kernel: they found its PCG form storing the owner partial without the mass term."""
    mesh, variant, knobs, prefixes, _ = PATHS[path]
    assert mesh == "jitter"
    for k in GENERAL_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    c = setup(mesh, sname)
    s = system(c, _lib.MODE_FAST, keep_node_order=variant == "keep_order")
    kern = kernel(s)
    if prefixes == ("k_keff_groups_pipe",) and sname in SHORT_FANS:
        prefixes = ("k_keff_tiles_pipe",)
    assert kern.startswith(prefixes), kern
    if prefixes == ("k_keff_tiles",):
        assert not kern.startswith("k_keff_tiles_pipe"), kern
    if prefixes == ("k_keff_groups_pipe",):
        m = re.fullmatch(r"k_keff_groups_pipe<(true|false), false, 1, (\d+), (true|false)>", kern)
        assert m, kern
        assert m.group(1) == ("true" if sname == "ortho" else "false"), kern
        assert m.group(3) == ("true" if len(c.materials) == 1 else "false"), kern
        if path == "fan-groups-128":
            assert m.group(2) == "128", kern
    what = f"{path} {c.name}"
    fast_apply_check(c, s, lambda x: ref_apply(c, x, oracle(mesh, sname)), what)
    fast_solve_check(c, s, oracle_solve(mesh, sname), what)
    s.close()


# ---- FAST, hex tiles -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sname", ["ortho", "rot", "mixed-thirds"])
def test_fast_hex_tiles(sname, monkeypatch):
    """k_keff_hex_tiles<ISO, ...> (CWF_LATTICE=0 on the structured 6 x 4 x 3 hex block) against O.hex8_apply and the
    fp64 solution O.hex8_solve64 with the same stiffness array."""
    monkeypatch.setenv("CWF_LATTICE", "0")
    monkeypatch.delenv("CWF_HEX_NT", raising=False)
    c = setup("hex", sname)
    s = system(c)
    assert kernel(s).startswith("k_keff_hex_tiles"), kernel(s)
    what = f"hex-tiles {c.name}"
    fast_apply_check(c, s, lambda x: ref_apply(c, x), what)
    fast_solve_check(c, s, oracle_solve("hex", sname), what)
    s.close()


def test_fast_hex8_derived_fields_centroid_strain(monkeypatch):
    """k_derived_nodes<false, true> and the hex8 element pass on the `rot` hex-tile handle: a linear field has the
    strain sym(A) everywhere and the stress ROT sym(A) (test_hex8.test_gpu_hex8_derived_fields_centroid_strain)."""
    monkeypatch.setenv("CWF_LATTICE", "0")
    c = setup("hex", "rot")
    s = system(c, scalars=(1.0, 0.0))
    A = np.array([[1.0, 2.0, -3.0], [0.5, -1.0, 2.0], [3.0, 1.0, 0.25]]) * 1e-4
    u = (c.mesh.coords @ A.T).astype(np.float32).reshape(-1)
    ds = post.compute_derived_fields(c.packing, c.materials, system=s, displacement=u)
    ef, nf = ds.elements.astype(np.float64), ds.nodes.astype(np.float64)
    want = np.array([A[0, 0], A[1, 1], A[2, 2], A[0, 1] + A[1, 0], A[1, 2] + A[2, 1], A[0, 2] + A[2, 0]])
    sig = MC.ROT @ want
    errs = (np.abs(ef[:, :6] - want).max() / np.abs(want).max(), np.abs(ef[:, 6:12] - sig).max() / np.abs(sig).max(),
            np.abs(nf[:, :6] - want).max() / np.abs(want).max(), np.abs(nf[:, 6:12] - sig).max() / np.abs(sig).max())
    print(f"{c.name}: hex8 derived fields on a {kernel(s)} handle, element strain / stress, node strain / stress "
          f"errors {errs[0]:.2e} {errs[1]:.2e} {errs[2]:.2e} {errs[3]:.2e}")
    assert max(errs) <= 1e-5
    s.close()


# ---- FAST, the one-material lattice ----------------------------------------------------------------------------------
SCHEDULES = {"resident": ({}, LATTICE), "fused": ({"CWF_FUSED": "1"}, ("k_pcg_lattice",)),
             "two-kernel": ({"CWF_FUSED": "0"}, ("k_keff_lattice<",))}
LATTICE_CASES = ([(m, s, k) for m in ("block", "rollers") for s in ("ortho", "rot") for k in SCHEDULES] +
                 [("block-hex", s, "resident") for s in ("ortho", "rot")])


@pytest.mark.parametrize("mesh,sname,schedule", LATTICE_CASES)
def test_fast_lattice(mesh, sname, schedule, monkeypatch):
    """The stencil tables lattice.cpp derives from a full D, in the three PCG schedules, tet4 and hex8."""
    for k in ("CWF_FUSED", "CWF_RESIDENT", "CWF_LATTICE", "CWF_FUSED_MAXWG"):
        monkeypatch.delenv(k, raising=False)
    env, prefixes = SCHEDULES[schedule]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c = setup(mesh, sname)
    s = system(c)
    kern = kernel(s)
    assert kern.startswith(prefixes) and ("LatHex" if is_hex(c) else "LatKuhn") in kern, kern
    what = f"lattice-{schedule} {c.name}"
    tet = None if is_hex(c) else oracle(mesh, sname)
    fast_apply_check(c, s, lambda x: ref_apply(c, x, tet), what)
    fast_solve_check(c, s, oracle_solve(mesh, sname), what)
    s.close()


# ---- FAST, the layered lattice ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def layered(name, element="tet4"):
    shape, layers = LAYERED_SHAPES[name]
    base = scenarios.layered_case(*shape, layers, element=element, **KW)
    return MC.MaterialCase(base, STRATA, name=f"{name}-{element}/strata")


@pytest.mark.parametrize("element", ["tet4", "hex8"])
@pytest.mark.parametrize("name", ["7x5x6", "12x10x9"])
def test_fast_layered_apply(name, element):
    c = layered(name, element)
    s = system(c)
    kind = "LatHex" if element == "hex8" else "LatKuhn"
    assert kernel(s).startswith(f"{LAYERED}<1, false, {kind},"), kernel(s)
    fast_apply_check(c, s, lambda x: ref_apply(c, x), f"layered {c.name}")
    s.close()


@functools.lru_cache(maxsize=None)
def layered_solve(name):
    return ref_solve(layered(name))


@pytest.mark.parametrize("name", ["7x5x6", "12x10x9"])
def test_fast_layered_solve(name):
    c = layered(name)
    s = system(c)
    assert kernel(s).startswith(LAYERED), kernel(s)
    fast_solve_check(c, s, layered_solve(name), f"layered {c.name}")
    s.close()


# ---- FAST steppers against the PARITY stepper ------------------------------------------------------------------------
@pytest.mark.parametrize("mesh,sname", [("jitter", "mixed-thirds"), ("block", "rot")])
def test_fast_stepper_against_parity(mesh, sname):
    """Three FAST Newmark steps (Rayleigh damping on: the beta-damping apply form runs next to the PCG form) against
    the PARITY stepper's, which test_parity_stepper_three_steps pins to the oracle: helpers.STEP_REL_TOL."""
    prefixes = LATTICE if mesh == "block" else ("k_keff_groups_pipe<false,",)
    c = setup(mesh, sname)
    P = c.packing
    ref = Stepper(P, c.materials, c.rayleigh, c.cfg.solver, c.cfg.time, mode=_lib.MODE_PARITY)
    fast = Stepper(P, c.materials, c.rayleigh, c.cfg.solver, c.cfg.time, mode=_lib.MODE_FAST)
    assert kernel(fast.system).startswith(prefixes), kernel(fast.system)
    for k in range(3):
        tr = ref.step(0.01 * k).value()
        tf = fast.step(0.01 * k).value()
        print(f"{c.name} step {k}: {kernel(fast.system)}  iterations {tf.pcg.iterations} (PARITY {tr.pcg.iterations})")
        assert tf.pcg.converged and tr.pcg.converged
        assert abs(tf.pcg.iterations - tr.pcg.iterations) <= max(3, tr.pcg.iterations // 10)
    check_step_against_parity(fast.get_state(Stepper.SOLUTION), ref.get_state(Stepper.SOLUTION),
                              fast.get_state(Stepper.DISPLACEMENT), ref.get_state(Stepper.DISPLACEMENT),
                              f"{c.name} after 3 steps")
    for st in (ref, fast):
        st.close()
        st.system.close()


# ---- two LOCAL shards ------------------------------------------------------------------------------------------------
def test_sharded_parity_solve_bitwise_equals_single_handle():
    """mixed-thirds on the jittered mesh over two PARITY shards cut at node 256 (test_gpu_shard's construction): x,
    r, the telemetry and the histories are the one-handle solve's, which test_parity_solve pins to the oracle."""
    c = setup("jitter", "mixed-thirds")
    P = c.packing
    sK, sM = c.scalars()
    ranges = shard.slab_ranges(P.node_count, 2, align=256)
    assert ranges.tolist() == [0, 256, P.node_count]
    comm = shard.Comm.local(2)
    systems, shards, rhs, xs, rs = [], [], [], [], []
    for k in range(2):
        sh = shard.build_shard(system(c, _lib.MODE_PARITY), ranges, k)
        assert sorted(set(sh.material_index.tolist())) == [0, 1, 2]
        s = sh.system(c.materials, sK, sM, mode=_lib.MODE_PARITY)
        comm.attach(s, sh)
        systems.append(s)
        shards.append(sh)
        rhs.append(sh.local_dofs(c.static_rhs()))
        xs.append(np.zeros(3 * sh.local_nodes, np.float32))
        rs.append(np.zeros(3 * sh.local_nodes, np.float32))
    tel = shard.solve_pcg_group(systems, rhs, SETTINGS, xs, residuals=rs).value()
    x, r = np.zeros((P.node_count, 3), np.float32), np.zeros((P.node_count, 3), np.float32)
    for sh, xl, rl in zip(shards, xs, rs):
        g = sh.node_global[: sh.owned_nodes].astype(np.int64)
        x[g], r[g] = xl.reshape(-1, 3)[: sh.owned_nodes], rl.reshape(-1, 3)[: sh.owned_nodes]
    hists = [pcg.residual_history(s) for s in systems]
    comm.close()
    single = system(c, _lib.MODE_PARITY)
    x1, r1 = np.zeros(P.dof_count, np.float32), np.zeros(P.dof_count, np.float32)
    t1 = pcg.solve_pcg(single, c.static_rhs(), SETTINGS, pcg.PcgVectors(x1, r1)).value()
    print(f"{c.name}: two PARITY shards, iterations {tel.iterations} (one handle {t1.iterations})")
    assert tel.converged and (tel.iterations, tel.residual_norm, tel.rhs_norm, tel.alpha_last, tel.beta_last) == (
        t1.iterations, t1.residual_norm, t1.rhs_norm, t1.alpha_last, t1.beta_last)
    same_bits(x.reshape(-1), x1, f"{c.name} sharded x")
    same_bits(r.reshape(-1), r1, f"{c.name} sharded r")
    h1 = pcg.residual_history(single)
    for h in hists:
        assert np.array_equal(h, h1)
    single.close()


def test_sharded_layered_solve_follows_single_handle():
    """The layered 12 x 10 x 9 block with the strata [ISO, ROT, ORTHO] over two FAST slab shards cut at node plane 4
    (test_gpu_lattice_layered.test_layered_slab_shards' construction): both run the layered kernel, and the attached
    solve follows the one-handle solve to 1e-4 in its iteration count +-10%."""
    shape, layers = LAYERED_SHAPES["12x10x9"]
    glob = layered("12x10x9")
    P = glob.packing
    sK, sM = glob.scalars()
    planes = [0, 4, shape[2] + 1]
    comm = shard.Comm.local(2)
    systems, shards, rhs, xs = [], [], [], []
    for k in range(2):
        sub, node_global, begin = scenarios.layered_slab_case(shape, layers, planes, k, **KW)
        src = pcg.MatrixFreeSystem.from_packing(sub.packing, glob.materials, sK, sM, mode=_lib.MODE_FAST)
        sh = shard.build_shard(src, begin, k, node_global)
        s = sh.system(glob.materials, sK, sM)
        comm.attach(s, sh)
        assert kernel(s).startswith(LAYERED), kernel(s)
        systems.append(s)
        shards.append(sh)
        rhs.append(sh.local_dofs(sub.static_rhs()))
        xs.append(np.zeros(3 * sh.local_nodes, np.float32))
    tel = shard.solve_pcg_group(systems, rhs, SETTINGS, xs).value()
    xg = np.zeros((P.node_count, 3), np.float32)
    for sh, xl in zip(shards, xs):
        xg[sh.node_global[: sh.owned_nodes].astype(np.int64)] = xl.reshape(-1, 3)[: sh.owned_nodes]
    comm.close()
    single = system(glob)
    x1 = np.zeros(P.dof_count, np.float32)
    t1 = pcg.solve_pcg(single, glob.static_rhs(), SETTINGS, pcg.PcgVectors(x1, None)).value()
    err = float(np.linalg.norm(xg.reshape(-1) - x1) / np.linalg.norm(x1))
    print(f"{glob.name}: two FAST shards cut at plane 4 ({kernel(single)}), |x - x_single| / |x_single| = {err:.3e}, "
          f"iterations {tel.iterations} / {t1.iterations}")
    assert tel.converged and t1.converged
    assert err <= 1e-4
    assert abs(tel.iterations - t1.iterations) <= max(3, t1.iterations // 10)
    single.close()
