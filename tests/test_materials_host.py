"""Anisotropic materials on the CPU: the builders of tests/materials_common.py, and the host table code
(lattice.cpp: the one-material stencil, the layered per-plane tables) and the hex8 oracle with a full 6 x 6 stiffness.

The checks are the existing host tests' own, called with another material: test_lattice's stencil check, test_hex8's
oracle physics checks, test_lattice_layered's table check. Their bounds are unchanged."""
import numpy as np
import pytest

import materials_common as MC
import test_hex8 as H
import test_lattice as TL
import test_lattice_layered as TLL
from cwf import scenarios

MATERIALS = {"ortho": MC.ORTHO, "rot": MC.ROT}


def test_builders():
    for name, D, lo, hi in (("ortho", MC.ORTHO, 3.0e9, 3.2e10), ("rot", MC.ROT, 3.05e9, 2.87e10)):
        top = np.abs(D).max()
        assert np.abs(D - D.T).max() <= 1e-12 * top
        w = np.linalg.eigvalsh(0.5 * (D + D.T))
        print(f"{name}: eigenvalues {w.min():.4e} ... {w.max():.4e}, smallest |entry| / largest "
              f"{np.abs(D).min() / top:.3e}")
        assert w.min() > 0.0
        assert abs(w.min() - lo) <= 0.01 * lo and abs(w.max() - hi) <= 0.01 * hi
    # ORTHO: the isotropic zero pattern, nine distinct values
    nz = MC.ORTHO != 0.0
    assert np.array_equal(nz, np.asarray(MC.ISO) != 0.0) and int(nz.sum()) == 12
    assert np.unique(MC.ORTHO[nz]).size == 9
    # ROT: full, and ORTHO again when turned back
    assert np.abs(MC.ROT).min() >= 1e-6 * np.abs(MC.ROT).max()
    assert np.abs(MC.rotate(MC.ROT, MC.R_ROT.T) - MC.ORTHO).max() <= 1e-12 * np.abs(MC.ORTHO).max()
    # rotation leaves the eigenvalues of the 6 x 6 Kelvin (Mandel) form, not of the engineering-shear Voigt form;
    # the trace of the tensor contraction C_ijij is one invariant both forms share
    tr = lambda D: np.einsum("ijij", MC.tensor_of(D))
    assert abs(tr(MC.ROT) - tr(MC.ORTHO)) <= 1e-12 * tr(MC.ORTHO)
    # many(n): distinct, and props() carries the 36 numbers unchanged
    assert len({m.tobytes() for m in MC.many(18)}) == 18
    assert np.array_equal(np.asarray(MC.props(MC.ROT).stiffness).reshape(6, 6), MC.ROT)


def test_assignments():
    case = scenarios.block_case(7, 6, 5, h=0.1, jitter=True)
    t = MC.thirds(case)
    counts = np.bincount(t, minlength=3)
    print(f"thirds on the jittered 7x6x5: {counts.tolist()} tets")
    assert counts.sum() == 1260 and counts.min() >= 400
    assert np.array_equal(np.bincount(MC.scattered(case, 3)), [420, 420, 420])
    assert MC.scattered(case, 18).max() == 17
    P = MC.with_materials(case, t)
    assert P.material_index.dtype == np.uint32 and P.volume is case.packing.volume


@pytest.mark.parametrize("mat", sorted(MATERIALS))
@pytest.mark.parametrize("name", ["8x3x4", "rollers"])
def test_lattice_stencil(name, mat):
    TL.test_stencil_reproduces_the_oracle_operator(name, materials=[MC.props(MATERIALS[mat])])


@pytest.mark.parametrize("mat", sorted(MATERIALS))
def test_hex8_oracle_physics(mat):
    H.test_hex8_oracle_rigid_modes_and_patch_test(D=MATERIALS[mat].reshape(-1))
    H.test_hex8_oracle_symmetric_positive_and_diag_blocks(D=MATERIALS[mat].reshape(-1))


@pytest.mark.parametrize("name", ["5x4x4", "7x5x6"])
def test_layered_tables(name):
    shape, layers = TLL.CASES[name]
    case = scenarios.layered_case(*shape, layers)
    strata = [MC.props(D) for D in (MC.ISO, MC.ROT, MC.ORTHO)]
    TLL.test_layered_tables_reproduce_the_oracle_operator((case, shape, layers, None), materials=strata)


def test_no_stiffness_clears_the_paired_stencil_flag():
    """cwf_lattice_describe's sym flag (S_(-d) = S_d) on a one-material block: the Kuhn cell and the stiffness tensor
    are both unchanged by the point reflection x -> -x, so the flag holds for every D, a non-symmetric one included
    (DESIGN.md section 3)."""
    rng = np.random.Generator(np.random.PCG64(9))
    A = rng.uniform(-1.0, 1.0, (6, 6))
    full = 1.0e10 * (A @ A.T + 6.0 * np.eye(6))
    skew = full + 1.0e9 * (A - A.T)
    case = scenarios.block_case(5, 4, 3, h=0.1)
    for name, D in (("ortho", MC.ORTHO), ("rot", MC.ROT), ("random-spd", full), ("non-symmetric", skew)):
        out = TL.describe(TL.pcg.MatrixFreeSystem.from_packing(case.packing, [D.reshape(-1)], 1.0, 0.0,
                                                               mode=TL._lib.MODE_FAST))
        assert out is not None
        print(f"{name}: sym = {out[3]}")
        assert out[3]
