"""The block kernels of the modal analysis on the GPU (csrc/modal.hip): k_block_gram (G = A^T W B, fp64 on the f64
MFMA) and k_block_rotate (X' = X Q, Y' = M X').

Exact data pins the MFMA lane map: with small-integer entries (and small-integer masses) every product and partial
sum is an integer far below 2^53, so the Gram matrix must equal the integer one bit for bit whatever the summation
order. A wrong C/D row formula scrambles rows and cannot pass; a tolerance test on random data could."""
import functools

import numpy as np
import pytest

from cwf import _lib, modal, pcg, scenarios
from helpers import assert_bitwise

pytestmark = pytest.mark.gpu

DOF_BITS = np.array([1, 2, 4], np.uint32)


@functools.lru_cache(maxsize=None)
def small_system(mode):
    """block_case(12, 3, 4): 260 nodes, D = 780 (no multiple of 16 or 64; one row chunk), with integer lumped masses
    1..4. FAST renumbers its nodes internally (the public block calls weight caller-order vectors), PARITY does not."""
    case = scenarios.block_case(12, 3, 4, h=0.25)
    P = case.packing
    assert (P.node_count, P.dof_count) == (260, 780)
    s = pcg.MatrixFreeSystem.from_packing(P, case.materials, 1.0, 0.0, mode=mode)
    s.lumped_mass = (1 + (np.arange(P.node_count) * 7) % 4).astype(np.float32)
    return s


def weights(s):
    """W's diagonal: the lumped mass on free DOFs, 0 on constrained ones."""
    free = (np.repeat(s.bc_mask, 3) & np.tile(DOF_BITS, s.node_count)) == 0
    return np.repeat(s.lumped_mass.astype(np.float64), 3) * free


def int_block(rng, q, D):
    return rng.integers(-3, 4, (q, D)).astype(np.float32)


@pytest.mark.parametrize("mode", [_lib.MODE_FAST, _lib.MODE_PARITY], ids=["fast", "parity"])
@pytest.mark.parametrize("q", [1, 5, 16, 17, 32])
def test_block_gram_of_integer_data_is_exact(q, mode):
    s = small_system(mode)
    D = s.dof_count
    rng = np.random.Generator(np.random.PCG64(100 + q))
    A = int_block(rng, q, D)
    w = weights(s)
    assert np.count_nonzero(w == 0) > 0 and set(np.unique(w[w > 0])) == {1.0, 2.0, 3.0, 4.0}
    others = [qb for qb in (1, 5, 16, 17, 32) if qb != q][:2] + [q]
    for weighted in (False, True):
        ww = w if weighted else np.ones(D)
        A64 = A.astype(np.float64)
        G = modal.block_gram(s, A, None, weighted).value()  # A == B: only the upper tiles are computed
        assert_bitwise(G, (A64 * ww) @ A64.T, f"A^T W A q={q} weighted={weighted}")
        for qb in others:  # A != B, other column counts on the B side (every tile-count pair)
            B = int_block(rng, qb, D)
            G = modal.block_gram(s, A, B, weighted).value()
            assert G.shape == (q, qb)
            assert_bitwise(G, (A64 * ww) @ B.astype(np.float64).T, f"A^T W B q={q},{qb} weighted={weighted}")


@pytest.mark.parametrize("mode", [_lib.MODE_FAST, _lib.MODE_PARITY], ids=["fast", "parity"])
@pytest.mark.parametrize("q_in,q_out", [(1, 1), (5, 3), (16, 16), (17, 32), (32, 7)])
def test_block_rotate_by_an_integer_matrix_is_exact(q_in, q_out, mode):
    s = small_system(mode)
    D = s.dof_count
    rng = np.random.Generator(np.random.PCG64(7 * q_in + q_out))
    X = int_block(rng, q_in, D)
    Q = rng.integers(-2, 3, (q_in, q_out)).astype(np.float64)
    Xo, MXo = modal.block_rotate(s, X, Q).value()
    ref = (Q.T @ X.astype(np.float64))  # |entries| <= 32 * 3 * 2: exact in f32
    assert_bitwise(Xo, ref.astype(np.float32), "X Q")
    w = weights(s)
    assert_bitwise(MXo, (ref * w).astype(np.float32), "M (X Q)")
    assert np.all(MXo[:, w == 0] == 0) and np.count_nonzero(w == 0) == 3 * np.count_nonzero(s.bc_mask == 7)
    Xo2, none = modal.block_rotate(s, X, Q, with_mass=False).value()
    assert none is None
    assert_bitwise(Xo2, Xo, "X Q without M")


def test_block_calls_on_device_tensors_equal_the_host_calls():
    import torch

    s = small_system(_lib.MODE_FAST)
    D = s.dof_count
    rng = np.random.Generator(np.random.PCG64(5))
    A, B = int_block(rng, 17, D), int_block(rng, 5, D)
    dA, dB = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    assert_bitwise(modal.block_gram(s, dA, dB, True).value(), modal.block_gram(s, A, B, True).value(), "gram")
    Q = rng.integers(-2, 3, (17, 5)).astype(np.float64)
    Xo, MXo = torch.zeros(5, D, device="cuda"), torch.zeros(5, D, device="cuda")
    assert modal.block_rotate(s, dA, Q, Xo, MXo).has_value()
    hX, hM = modal.block_rotate(s, A, Q).value()
    assert_bitwise(Xo.cpu().numpy(), hX, "rotate X")
    assert_bitwise(MXo.cpu().numpy(), hM, "rotate MX")
    # in place is refused, not computed
    e = modal.block_rotate(s, dA, np.eye(17), dA, None)
    assert not e.has_value() and e.error().message == "block rotation is out of place"


def test_block_argument_errors():
    s = small_system(_lib.MODE_FAST)
    D = s.dof_count
    big = np.zeros((33, D), np.float32)
    e = modal.block_gram(s, big)
    assert not e.has_value() and e.error().message == "qa must be in [1, 32]" and e.error().context == ["qa=33"]
    e = modal.block_gram(s, big[:2], big)
    assert not e.has_value() and e.error().context == ["qb=33"]
    e = modal.block_rotate(s, big[:2], np.zeros((2, 33)))
    assert not e.has_value() and e.error().context == ["q_out=33"]
    L = _lib.load()
    G = np.zeros(4)
    assert L.cwf_hip_block_gram(s.handle(), None, 2, _lib.ptr(big), 2, 0, _lib.ptr(G), 0) == -11  # CWF_ERR_ARGUMENT
    assert _lib.last_error(s.handle()) == ("null pointer", ["A"])


@functools.lru_cache(maxsize=None)
def chunked_system():
    """block_case(24, 24, 24): D = 46,875 = 11 full row chunks of 4,096 and a tail of 1,819 rows (odd: the last
    16-row slab is partial and most columns start off a 16-B boundary)."""
    case = scenarios.block_case(24, 24, 24, h=0.1)
    assert case.packing.dof_count == 46875
    return pcg.MatrixFreeSystem.from_packing(case.packing, case.materials, 1.0, 0.0, mode=_lib.MODE_FAST)


@pytest.mark.parametrize("weighted", [False, True])
def test_block_gram_over_several_chunks_meets_the_summation_bound_and_repeats(weighted):
    s = chunked_system()
    D = s.dof_count
    rng = np.random.Generator(np.random.PCG64(11))
    A = rng.uniform(-1, 1, (17, D)).astype(np.float32)
    B = rng.uniform(-1, 1, (32, D)).astype(np.float32)
    w = weights(s) if weighted else np.ones(D)
    A64, B64 = A.astype(np.float64), B.astype(np.float64)
    # Every product a (w b) is formed from exact f32 operands (w b is exact in fp64: 24 + 24 bits) and rounded at
    # most once on its way into the sum, and the D terms are added in fp64 in some fixed order: the standard bound
    # for a length-D sum, |err| <= D u sum |terms| (u = 2^-53), with one more u for the weighted products.
    terms = D + (1 if weighted else 0)
    for X, Y in ((A, B), (B, None)):
        X64 = X.astype(np.float64)
        Y64 = X64 if Y is None else Y.astype(np.float64)
        G = modal.block_gram(s, X, Y, weighted).value()
        ref = (X64 * w) @ Y64.T
        bound = terms * 2.0 ** -53 * ((np.abs(X64) * w) @ np.abs(Y64).T)
        err = np.abs(G - ref)
        print(f"weighted={weighted} q={X.shape[0]}x{Y64.shape[0]}: worst err/bound {np.max(err / bound):.3e}")
        assert np.all(err <= bound)
        assert_bitwise(modal.block_gram(s, X, Y, weighted).value(), G, "second call")
    assert A64.shape == (17, D) and B64.shape == (32, D)
