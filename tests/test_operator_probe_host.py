"""The entry-wise probe's own reference and checks on the CPU (tests/operator_probe_common.py), so that the GPU tests
built on them (test_gpu_operator_probe.py, test_gpu_pcg_identities.py) can neither fail nor pass because of their
reference:

  * the numpy K_ref equals the oracle's dense assembly (tet4) and the oracle's fp64 hex8 operator column by column, to
    1e-13 of the row scale R_I;
  * coloured probes recover a known banded matrix exactly;
  * the host's lattice tables (cwf_lattice_describe) applied as test_lattice.lattice_apply does, with every operation
    rounded to fp32, stay inside the lattice caps c_e = 16, c_v = 128 (u = 2^-24; here 2.6 to 3.4 u per entry, the
    MI355X's figures to the digit, and 3.0 to 3.2 u on a random vector), give structural zeros and translations
    exactly 0, and a stencil entry perturbed by 1e-5 of its row maximum is caught;
  * the oracle's PARITY apply_keff (fp64 accumulation, one rounding per row) probed the same way stays inside them.
"""
import functools

import numpy as np
import pytest

import oracle as O
import operator_probe_common as OP
from cwf import _lib, pcg, scenarios
from helpers import oracle_system
from test_hex8 import hex_case
from test_lattice import OFF, PAIRS, describe

LATTICE_CE, LATTICE_CV = 16.0, 128.0

LATTICE_CASES = {
    "8x3x4": lambda: scenarios.block_case(8, 3, 4, h=0.1),
    "rayleigh": lambda: scenarios.block_case(6, 4, 3, h=0.1, xi=0.05, w=(10.0, 100.0)),
    "rollers": lambda: scenarios.roller_case(7, 5, 4),
}


@functools.lru_cache(maxsize=None)
def lattice_case(name):
    return LATTICE_CASES[name]()


# ---- the reference against the oracle --------------------------------------------------------------------------------
def test_tet4_reference_equals_the_oracle_dense_assembly():
    case = scenarios.block_case(4, 3, 2, h=0.1, jitter=True)
    P = case.packing
    D = P.dof_count
    ref = OP.tet4_reference(P, case.materials, 1.0, 0.0, bc_mask=np.zeros(P.node_count, np.uint32))
    packed = O.Packed(P.node_count, P.element_count, P.connectivity, P.gradients, P.volume, P.material_index,
                      P.lumped_mass64, P.lumped_mass, P.offsets, P.element_indices, P.local_indices)
    stiff = np.concatenate([np.asarray(m.stiffness, np.float64).reshape(-1) for m in case.materials])
    g64 = np.asarray(P.gradients).reshape(P.element_count, -1)[:, :12].astype(np.float64)
    K = O.dense_assemble(packed, case.mesh.tets, g64, P.volume.astype(np.float64), stiff).reshape(D, D)
    got = ref.dense()
    err = float(np.max(np.abs(got - K) / ref.row_scale[:, None]))
    print(f"tet4 K_ref against orc_dense_assemble: {err:.2e} of R_I")
    assert err <= 1e-13
    # the absolute assembly and its diagonal, against the same dense matrix element by element
    assert np.all(ref.apply_abs(np.eye(D)) >= np.abs(K) * (1 - 1e-13))
    assert np.allclose(np.diag(ref.apply_abs(np.eye(D))), ref.diag_abs, rtol=1e-13, atol=0.0)
    # the Dirichlet rule and the scalars, against the oracle's apply_keff (f32 out: half an ulp of the row)
    sK, sM = case.scalars()
    full = OP.reference_of(case)
    x = np.random.Generator(np.random.PCG64(2)).uniform(-1, 1, D).astype(np.float32)
    y = oracle_system(P, case.materials, sK, sM).apply_keff(x)
    want = full.apply(x)
    assert np.array_equal(y[full.fixed], x[full.fixed]) and np.array_equal(want[full.fixed], x[full.fixed])
    assert np.all(np.abs(y - want) <= 0.5 * np.spacing(np.abs(want).astype(np.float32)) + 1e-13 * full.row_scale)


def test_hex8_reference_equals_the_oracle_operator():
    case = hex_case(6, 4, 3, xi=0.05, w=(10.0, 100.0))
    P = case.packing
    D = P.dof_count
    sK, sM = case.scalars()
    assert sM != 0.0
    ref = OP.reference_of(case)
    stiff = np.concatenate([np.asarray(m.stiffness, np.float64).reshape(-1) for m in case.materials])
    coords = np.ascontiguousarray(case.mesh.coords, np.float64)
    hexes = np.ascontiguousarray(case.mesh.tets, np.uint32).reshape(-1, 8)
    mat = np.ascontiguousarray(P.material_index, np.uint32)
    mass = np.ascontiguousarray(P.lumped_mass, np.float32)
    mask = np.ascontiguousarray(P.bc_mask, np.uint32)
    K = np.zeros((D, D))
    out = np.zeros(D)
    for j in range(D):
        e = np.zeros(D)
        e[j] = 1.0
        assert O.lib().orc_hex8_apply64(P.node_count, hexes.shape[0], O._p(coords), O._p(hexes), O._p(mat),
                                        O._p(stiff), sK, sM, O._p(mass), O._p(mask), O._p(e), O._p(out)) == 0
        K[:, j] = out
    got = ref.dense()
    err = float(np.max(np.abs(got - K) / ref.row_scale[:, None]))
    print(f"hex8 K_ref against orc_hex8_apply64: {err:.2e} of R_I")
    assert err <= 1e-13
    assert np.array_equal(got[ref.fixed], np.eye(D)[ref.fixed])


def test_coloured_probes_recover_a_banded_matrix():
    rng = np.random.Generator(np.random.PCG64(4))
    D, hb = 37, 3
    i, j = np.meshgrid(np.arange(D), np.arange(D), indexing="ij")
    M = np.where(np.abs(i - j) <= hb, rng.integers(-8, 9, (D, D)).astype(np.float64), 0.0)
    V = OP.banded_probes(D, hb)
    assert V.shape == (D, 2 * hb + 1)
    assert np.array_equal(OP.read_banded(M @ V, hb), M)


def test_lattice_probes_put_one_probe_node_in_every_row():
    case = lattice_case("8x3x4")
    ref = OP.reference_of(case)
    V, nodes, comp = OP.lattice_probes(case.mesh.coords)
    assert V.shape == (ref.D, 81) and np.array_equal(V.sum(1), np.ones(ref.D))
    adj = ref.reach(np.eye(ref.N, dtype=bool))  # node adjacency by shared elements
    assert int((adj.astype(np.int64) @ nodes.astype(np.int64)).max()) == 1
    # so a coloured product is the matrix entry itself
    K = ref.dense()
    Y = ref.apply(V)
    I = 57  # interior; node 58 is its +x neighbour
    c = int(np.nonzero(nodes[I + 1] & (comp == 1))[0][0])
    J = np.nonzero(adj[I] & nodes[:, c])[0]
    assert J.tolist() == [I + 1] and np.any(K[3 * I:3 * I + 3, 3 * J[0] + 1] != 0)
    assert np.array_equal(Y[3 * I:3 * I + 3, c], K[3 * I:3 * I + 3, 3 * J[0] + 1])


# ---- the lattice tables, every operation rounded to fp32 -------------------------------------------------------------
def lattice_apply_f32(dims, coef, X, sK, mass_sM):
    """test_lattice.lattice_apply on a block of sanitised f32 vectors X [D, m] with every product, difference and sum
    rounded to fp32 (numpy float32 arithmetic, no fused operations), the mass term included."""
    nx, ny, nz = dims
    m = X.shape[1]
    f32 = np.float32
    u = np.pad(X.astype(f32).reshape(nz, ny, nx, 3, m), ((1, 1), (1, 1), (1, 1), (0, 0), (0, 0)), mode="edge")
    S = coef[:135].astype(f32).reshape(15, 3, 3)
    Kp = coef[135:549].astype(f32).reshape(46, 3, 3)
    u0 = u[1:nz + 1, 1:ny + 1, 1:nx + 1]

    def nb(d):
        dx, dy, dz = d
        return u[1 + dz:nz + 1 + dz, 1 + dy:ny + 1 + dy, 1 + dx:nx + 1 + dx] - u0

    def fold(acc, B, w):  # acc[r] = acc[r] + B[r, c] * w[c], c ascending
        for c in range(3):
            acc += B[:, c][:, None] * w[..., c:c + 1, :]

    y = np.zeros((nz, ny, nx, 3, m), f32)
    for o in range(1, 15):
        fold(y, S[o], nb(OFF[o]))
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    surface = (i == 0) | (i == nx - 1) | (j == 0) | (j == ny - 1) | (k == 0) | (k == nz - 1)
    ys = np.zeros_like(y)
    for c in range(8):
        cx, cy, cz = c & 1, (c >> 1) & 1, (c >> 2) & 1
        has = ((i >= 1) if cx else (i + 1 < nx)) & ((j >= 1) if cy else (j + 1 < ny)) & \
              ((k >= 1) if cz else (k + 1 < nz))
        t = np.zeros_like(y)
        for p, (a, b) in enumerate(PAIRS):
            if a == c and b != c:
                fold(t, Kp[p], nb(((b & 1) - cx, ((b >> 1) & 1) - cy, ((b >> 2) & 1) - cz)))
        ys += np.where(has[..., None, None], t, f32(0.0))
    y = np.where(surface[..., None, None], ys, y)
    assert y.dtype == f32
    y = f32(sK) * y.reshape(-1, m)
    return y + mass_sM.astype(f32)[:, None] * X.astype(f32)


def emulated_operator(case, coef_edit=None, bc_mask=None, scalars=None):
    """V f32 [D, m] -> the f32 emulation of the case's lattice operator with the oracle's Dirichlet rule."""
    P = case.packing
    sK, sM = case.scalars() if scalars is None else scalars
    out = describe(pcg.MatrixFreeSystem.from_packing(P, case.materials, sK, sM, mode=_lib.MODE_FAST))
    assert out is not None
    dims, coef, _, _ = out
    if coef_edit is not None:
        coef = coef_edit(coef.copy())
    mask = P.bc_mask if bc_mask is None else bc_mask
    fixed = (np.repeat(mask, 3) & np.tile(OP.DOF_BITS, P.node_count)) != 0
    mass_sM = np.repeat((P.lumped_mass.astype(np.float64) * sM).astype(np.float32), 3)

    def apply(V):
        V = np.asarray(V, np.float32).reshape(P.dof_count, -1)
        Y = lattice_apply_f32(dims, coef, np.where(fixed[:, None], np.float32(0.0), V), sK, mass_sM)
        return np.where(fixed[:, None], V, Y)

    return apply, coef


def random_vector(D, seed=3):
    return np.random.Generator(np.random.PCG64(seed)).uniform(-1, 1, D).astype(np.float32)


@pytest.mark.parametrize("probes", ["coloured", "unit"])
@pytest.mark.parametrize("name", sorted(LATTICE_CASES))
def test_fp32_emulation_of_the_lattice_tables_is_inside_the_caps(name, probes):
    case = lattice_case(name)
    ref = OP.reference_of(case)
    apply, _ = emulated_operator(case)
    V, nodes, comp = OP.lattice_probes(case.mesh.coords) if probes == "coloured" else OP.unit_probes(ref.N)
    rep = OP.probe_report(ref, V, nodes, comp, apply(V))
    x = random_vector(ref.D)
    ratio, off_scale = OP.vector_ratio(ref, x, apply(x)[:, 0])
    print(f"{name} ({probes}, {V.shape[1]} probes): entry {rep['entry']:.2f} u R_I (cap {LATTICE_CE:g}), random vector "
          f"{ratio:.2f} u A|x| (cap {LATTICE_CV:g})")
    assert (rep["structural"], rep["passthrough"], rep["leaked"]) == (0, 0, 0), rep
    assert rep["entry"] <= LATTICE_CE
    assert ratio <= LATTICE_CV and off_scale == 0


@pytest.mark.parametrize("name", sorted(LATTICE_CASES))
def test_fp32_emulation_maps_translations_to_zero(name):
    case = lattice_case(name)
    P = case.packing
    sK, _ = case.scalars()
    apply, _ = emulated_operator(case, bc_mask=np.zeros(P.node_count, np.uint32), scalars=(sK, 0.0))
    T = np.tile(np.eye(3, dtype=np.float32) * np.float32(0.7), (P.node_count, 1))
    assert np.all(apply(T) == 0.0)


def test_a_perturbed_stencil_entry_is_caught():
    """One interior stencil entry (offset +x, row 0, column 0) moved by 1e-5 of the row's largest entry, 168 u: the
    entry-wise check must fail, on the coloured probes and on the unit probes alike, while max |y - ref| <= 2e-5
    max |ref| on a random vector (what the suite asserted so far) still passes."""
    case = lattice_case("8x3x4")
    ref = OP.reference_of(case)
    sK, _ = case.scalars()

    def edit(coef):
        S = coef[:135].reshape(15, 3, 3)
        S[1, 0, 0] += np.float32(1e-5 * np.abs(S[:, 0, :]).max())
        return coef

    good, coef = emulated_operator(case)
    bad, _ = emulated_operator(case, edit)
    # R_I of an interior node is the largest diagonal entry of A: at least the row maximum of the tables times s_K
    assert ref.node_scale.max() >= sK * np.abs(coef[:135].reshape(15, 3, 3)[1:, 0, :]).max()
    for V, nodes, comp in (OP.lattice_probes(case.mesh.coords), OP.unit_probes(ref.N)):
        assert OP.probe_report(ref, V, nodes, comp, good(V))["entry"] <= LATTICE_CE
        rep = OP.probe_report(ref, V, nodes, comp, bad(V))
        print(f"perturbed entry, {V.shape[1]} probes: {rep['entry']:.1f} u R_I")
        assert rep["entry"] > LATTICE_CE
    x = random_vector(ref.D)
    want = ref.apply(x)
    assert np.max(np.abs(bad(x)[:, 0] - want)) <= 2e-5 * np.max(np.abs(want))
    # a scaled row of the reference is caught the same way
    scaled = ref.apply(V)
    row = 3 * 57
    scaled[row] *= 1.0 + 1e-5
    assert OP.probe_report(ref, V, nodes, comp, good(V), scaled)["entry"] > LATTICE_CE


# ---- the bit-exact restatement, probed the same way ------------------------------------------------------------------
@pytest.mark.parametrize("name", ["block-8x3x4", "jitter-7x6x5"])
def test_oracle_parity_operator_is_inside_the_caps(name):
    case = lattice_case("8x3x4") if name.startswith("block") else scenarios.block_case(7, 6, 5, h=0.1, jitter=True)
    ref = OP.reference_of(case)
    o = oracle_system(case.packing, case.materials, *case.scalars())
    V, nodes, comp = OP.unit_probes(ref.N)
    Y = np.stack([o.apply_keff(V[:, c]) for c in range(V.shape[1])], 1)
    rep = OP.probe_report(ref, V, nodes, comp, Y)
    x = random_vector(ref.D)
    ratio, off_scale = OP.vector_ratio(ref, x, o.apply_keff(x))
    print(f"{name}: oracle apply_keff entry {rep['entry']:.2f} u R_I, random vector {ratio:.2f} u A|x|")
    assert (rep["structural"], rep["passthrough"], rep["leaked"]) == (0, 0, 0), rep
    assert rep["entry"] <= LATTICE_CE
    assert ratio <= LATTICE_CV and off_scale == 0
