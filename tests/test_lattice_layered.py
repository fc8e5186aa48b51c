"""Layered structured blocks (one material per k-layer of cells) on the CPU: the detection and the per-plane
stencil tables it derives (lattice.cpp), through the C-ABI introspection entry cwf_lattice_describe_layers (no
device needed).

The tables are applied here in numpy (fp64 over the f32 tables) with the kernel's algorithm (lattice.hip,
k_keff_lattice_layered): a strict-interior node of plane k takes the 14 off-centre stencil blocks of its plane's
class, the (material below, material above) pair, on the differences u_(n+d) - u_n; a surface node takes each
existing cell's pair blocks from the table of that cell's material. That must reproduce the pinned oracle's
apply_keff (the reference's element loop over the per-element materials) to the f32 rounding of the tables: 1e-6
of the operator scale (max |row|), the bound tests/test_lattice.py sets for the one-material tables."""
import ctypes as C

import numpy as np
import pytest

from cwf import _lib, mesh as cwf_mesh, meshgen, pack, pcg, scenarios
from helpers import oracle_system

OFF = np.array([[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [1, 1, 0],
                [-1, -1, 0], [1, 0, 1], [-1, 0, -1], [0, 1, 1], [0, -1, -1], [1, 1, 1], [-1, -1, -1]])
KUHN = [[0, 1, 3, 7], [0, 1, 5, 7], [0, 2, 3, 7], [0, 2, 6, 7], [0, 4, 5, 7], [0, 4, 6, 7]]
PAIRS = [(c, c2) for c in range(8) for c2 in range(8) if c == c2 or any(c in t and c2 in t for t in KUHN)]

CASES = {"7x5x6": ((7, 5, 6), [0, 0, 1, 1, 2, 0]), "5x4x4": ((5, 4, 4), [0, 1, 0, 1])}


def fast_system(case):
    sK, sM = case.scalars()
    return pcg.MatrixFreeSystem.from_packing(case.packing, case.materials, sK, sM, mode=_lib.MODE_FAST)


def describe_layers(system, renumber=True):
    """cwf_lattice_describe_layers -> None (no lattice) or a dict of its outputs."""
    L = _lib.load()
    desc = system.desc()
    dims, info = (C.c_uint32 * 3)(), (C.c_uint32 * 4)()
    pcap, ccap, mcap = 1 << 12, 16, 8
    plane, pcls, lmat = (np.zeros(pcap, np.uint32) for _ in range(3))
    cpair, ccoef = np.zeros(2 * ccap, np.uint32), np.zeros(ccap * 27 * 9, np.float32)
    mids, pcoef = np.zeros(mcap, np.uint32), np.zeros(mcap * 64 * 9, np.float32)
    p = _lib.ptr
    st = L.cwf_lattice_describe_layers(C.byref(desc), int(renumber), dims, info, pcap, p(plane), p(pcls), p(lmat), ccap,
                                       p(cpair), p(ccoef), mcap, p(mids), p(pcoef))
    assert st in (0, 1), st
    if st != 1:
        return None
    nmat, ncls, hex8, sym = (int(v) for v in info)
    noff, npair = (27, 64) if hex8 else (15, 46)
    nz = int(dims[2])
    return dict(dims=(int(dims[0]), int(dims[1]), nz), hex=bool(hex8), sym=bool(sym), plane=plane[:nz].copy(),
                plane_class=pcls[:nz].copy(), layer_material=lmat[:nz - 1].copy(),
                class_pair=cpair[:2 * ncls].reshape(ncls, 2).copy(),
                class_coef=ccoef[:ncls * noff * 9].reshape(ncls, noff, 3, 3).copy(), material_ids=mids[:nmat].copy(),
                pair_coef=pcoef[:nmat * npair * 9].reshape(nmat, npair, 3, 3).copy())


def describe_plain(system, renumber=True):
    L = _lib.load()
    desc = system.desc()
    dims = (C.c_uint32 * 3)()
    coef = np.zeros(549, np.float32)
    st = L.cwf_lattice_describe(C.byref(desc), int(renumber), dims, coef.ctypes.data, None)
    assert st in (0, 1), st
    return coef if st == 1 else None


def layered_apply(d, x3, sK):
    """K x (no mass, no Dirichlet) on the lattice in lexicographic order, the layered kernel's algorithm."""
    nx, ny, nz = d["dims"]
    u = np.pad(x3.reshape(nz, ny, nx, 3), ((1, 1), (1, 1), (1, 1), (0, 0)), mode="edge")
    S = d["class_coef"].astype(np.float64)[d["plane_class"]]  # [nz, 15, 3, 3]: each plane's table
    slot_of = {int(m): s for s, m in enumerate(d["material_ids"])}
    layer_slot = np.array([slot_of[int(m)] for m in d["layer_material"]])
    Kp = d["pair_coef"].astype(np.float64)
    u0 = u[1:nz + 1, 1:ny + 1, 1:nx + 1]

    def nb(dd):
        dx, dy, dz = dd
        return u[1 + dz:nz + 1 + dz, 1 + dy:ny + 1 + dy, 1 + dx:nx + 1 + dx] - u0

    y = np.zeros((nz, ny, nx, 3))
    for o in range(1, 15):
        y += np.einsum("kjic,krc->kjir", nb(OFF[o]), S[:, o])
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    surface = (i == 0) | (i == nx - 1) | (j == 0) | (j == ny - 1) | (k == 0) | (k == nz - 1)
    ys = np.zeros_like(y)
    for c in range(8):
        cx, cy, cz = c & 1, (c >> 1) & 1, (c >> 2) & 1
        has = ((i >= 1) if cx else (i + 1 < nx)) & ((j >= 1) if cy else (j + 1 < ny)) & \
              ((k >= 1) if cz else (k + 1 < nz))
        Kc = Kp[layer_slot[np.clip(np.arange(nz) - cz, 0, nz - 2)]]  # [nz, 46, 3, 3]: the cell's layer (k - cz)
        t = np.zeros_like(y)
        for p, (a, b) in enumerate(PAIRS):
            if a == c and b != c:
                dd = ((b & 1) - cx, ((b >> 1) & 1) - cy, ((b >> 2) & 1) - cz)
                t += np.einsum("kjic,krc->kjir", nb(dd), Kc[:, p])
        ys += np.where(has[..., None], t, 0.0)
    y = np.where(surface[..., None], ys, y)
    return sK * y.reshape(-1, 3)


@pytest.fixture(scope="module", params=sorted(CASES))
def layered(request):
    shape, layers = CASES[request.param]
    case = scenarios.layered_case(*shape, layers)
    return case, shape, layers, describe_layers(fast_system(case))


def test_layered_block_is_described(layered):
    case, shape, layers, d = layered
    assert d is not None and not d["hex"] and not d["sym"]
    assert d["dims"] == tuple(n + 1 for n in shape)
    assert np.array_equal(d["plane"], np.arange(d["dims"][2]) * d["dims"][0] * d["dims"][1])
    assert np.array_equal(d["layer_material"], layers)
    # one class per distinct (below, above) pair; the end planes take their one layer twice
    nz = shape[2]
    pairs = [(layers[max(k - 1, 0)], layers[min(k, nz - 1)]) for k in range(nz + 1)]
    assert [tuple(int(v) for v in d["class_pair"][c]) for c in d["plane_class"]] == pairs
    assert len(d["class_pair"]) == len(set(pairs))
    assert sorted(d["material_ids"].tolist()) == sorted(set(layers))
    # cwf_lattice_describe keeps refusing a layered block
    assert describe_plain(fast_system(case)) is None


def test_layered_tables_reproduce_the_oracle_operator(layered, materials=None):
    """materials (tests/test_materials_host.py): other strata stiffnesses than the case's; the tables are then
    described from them, not taken from the fixture."""
    case, shape, layers, d = layered
    P = case.packing
    sK, sM = case.scalars()
    if materials is not None:
        d = describe_layers(pcg.MatrixFreeSystem.from_packing(P, materials, sK, sM, mode=_lib.MODE_FAST))
        assert d is not None and not d["hex"]
    else:
        materials = case.materials
    rng = np.random.Generator(np.random.PCG64(1))
    x = rng.uniform(-1, 1, P.dof_count).astype(np.float32)
    mask = (np.repeat(P.bc_mask, 3) & np.tile(np.array([1, 2, 4], np.uint32), P.node_count)) != 0
    xs = np.where(mask, 0.0, x.astype(np.float64))
    y = layered_apply(d, xs, sK).reshape(-1) + sM * np.repeat(P.lumped_mass.astype(np.float64), 3) * xs
    y = np.where(mask, x, y)
    ref = oracle_system(P, materials, sK, sM).apply_keff(x).astype(np.float64)
    err = np.max(np.abs(y - ref)) / np.max(np.abs(ref))
    print(f"layered tables vs oracle: {err:.3e} of max |row|")
    assert err <= 1e-6


def test_interface_planes_are_not_symmetric(layered):
    """S_(-d) = S_d (the paired form) holds between equal layers only: exactly there, not on interface planes."""
    _, _, _, d = layered
    for c, (below, above) in enumerate(d["class_pair"]):
        S = d["class_coef"][c]
        paired = all(np.array_equal(S[o], S[o + 1]) for o in range(1, 15, 2))
        assert paired == (below == above), (c, below, above)


def test_material_varying_inside_a_layer_is_refused():
    tm, emat = meshgen.layered_block(6, 5, 4, [0, 1, 1, 2], 0.1)
    emat = emat.copy()
    cell = (2 * 5 + 3) * 6 + 2  # cell (2, 3, 2) of layer 2: its six tets to another material
    emat[6 * cell:6 * cell + 6] = 0
    mesh, mats, asg = scenarios.layered_mesh(tm, emat)
    cfg = scenarios.layered_config(mats, asg)
    case = scenarios.Case("mixed-layer", mesh, cfg, pack.build_packed_buffers(mesh, cfg))
    s = fast_system(case)
    assert describe_layers(s) is None and describe_plain(s) is None


def test_one_material_block_has_one_class_with_todays_tables():
    s = fast_system(scenarios.block_case(6, 5, 4, h=0.1))
    d, coef = describe_layers(s), describe_plain(s)
    assert d is not None and coef is not None and d["sym"]
    assert d["class_coef"].shape[0] == 1 and not d["plane_class"].any() and d["material_ids"].tolist() == [0]
    assert np.array_equal(d["class_coef"].reshape(-1).view(np.uint32), coef[:135].view(np.uint32))
    assert np.array_equal(d["pair_coef"].reshape(-1).view(np.uint32), coef[135:].view(np.uint32))


def test_layered_hex8_block_is_described():
    case = scenarios.layered_case(5, 4, 4, [0, 1, 0, 1], element="hex8")
    d = describe_layers(fast_system(case))
    assert d is not None and d["hex"] and d["class_coef"].shape[1:] == (27, 3, 3)
    assert np.array_equal(d["layer_material"], [0, 1, 0, 1]) and len(d["class_pair"]) == 4


def test_too_many_plane_classes_are_refused():
    """The cap (cwf_hip.h CWF_LATTICE_MAX_PLANE_CLASSES = 16): 5 materials in every order give 20 interface pairs."""
    mats = tuple(scenarios.Material(f"m{i}", (1.0 + i) * 1e9, 0.2, 2000.0) for i in range(5))
    layers = [0, 1, 0, 2, 0, 3, 0, 4, 1, 2, 1, 3, 1, 4, 2, 3, 2, 4, 3, 4, 0]
    case = scenarios.layered_case(3, 3, len(layers), layers, materials=mats)
    assert describe_layers(fast_system(case)) is None


def test_gmsh_round_trip_keeps_the_materials(tmp_path):
    shape, layers = CASES["7x5x6"]
    case = scenarios.layered_case(*shape, layers)
    tm, emat = meshgen.layered_block(*shape, layers, 0.1)
    names = [f"SOLID{s}" for s in range(3)]
    path = tmp_path / "layered.msh"
    meshgen.write_gmsh(tm, str(path), volumes=(names, emat))
    back = cwf_mesh.load_gmsh_file(path).value().to_tet_mesh()
    assert np.array_equal(back.tets, case.mesh.tets) and np.array_equal(back.coords, case.mesh.coords)
    packed = pack.build_packed_buffers(back, case.cfg)
    assert np.array_equal(packed.material_index, case.packing.material_index)
    assert np.array_equal(packed.material_index, emat)
