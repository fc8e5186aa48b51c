"""The restatement of the explicit step pinned on the host (no GPU, no library): explicit_common.scheme_steps against
the words recorded in tests/golden/data/explicit_restatement.npz, bit for bit.

The fixture holds the inputs and the expected u, v of two synthetic problems, one of 120 nodes and one of 300 (the tie
groups of 2, 8, 9, 64, 65 and 129 members, one on each side of every threshold of gather_sum, need 277). The operator
is elementwise numpy -- a diagonal and two rolled neighbours in float64, rounded to float32 -- and the load and the
correction force are one product and one sum per DOF: no BLAS, no np.sum, no transcendental function, so every word is
determined by IEEE arithmetic. The expected words were written by the five separate restatements this module's
scheme_steps replaced, which agreed with one another wherever two of them covered a case."""
import os

import numpy as np
import pytest

import explicit_common as xc
from helpers import assert_bitwise

FIXTURE = np.load(os.path.join(xc.ROOT, "tests", "golden", "data", "explicit_restatement.npz"))
CASES = {
    # problem, alpha_R, beta_R, first_step, steps, dashpots, ties, correction force
    "plain": ("small", 0.0, 0.0, 0, 7, False, False, False),
    "beta": ("small", 0.0, 2e-5, 0, 7, False, False, False),  # the w = u + beta_R v path
    "alpha": ("small", 5.0, 0.0, 0, 7, False, False, False),
    "dashpots": ("small", 5.0, 2e-5, 0, 7, True, False, False),  # 17 nodes in a permuted order
    "correction": ("small", 5.0, 0.0, 0, 7, True, False, True),
    "first_step": ("small", 5.0, 2e-5, 4, 5, True, False, False),
    "ties": ("tied", 5.0, 2e-5, 0, 7, True, True, False),
    "ties_correction": ("tied", 5.0, 0.0, 2, 5, True, True, True),
}


def scheme_arguments(name):
    """-> (the positional arguments of scheme_steps up to v0, the keyword arguments) of a case."""
    problem, alpha, beta, _, _, dashpots, ties, correction = CASES[name]
    Z = {k[len(problem) + 1:]: FIXTURE[k] for k in FIXTURE.files if k.startswith(problem + "_")}
    diag, off, cp = (Z[k].astype(np.float64) for k in ("diag", "off", "cp"))
    base, pattern = Z["base"].astype(np.float64), Z["pattern"].astype(np.float64)

    def apply(w):
        w = w.astype(np.float64)
        return ((diag * w + off * np.roll(w, 1)) + off * np.roll(w, -1)).astype(np.float32)

    kw = {}
    if dashpots:
        kw["dash"] = (Z["dash_ids"], Z["dash_P"], Z["dash_Q"])
    if ties:
        groups = [Z["tie_ids"][a:b] for a, b in zip(Z["tie_offsets"][:-1], Z["tie_offsets"][1:])]
        assert [len(g) for g in groups] == [2, 8, 9, 64, 65, 129]
        assert np.intersect1d(groups[2], Z["dash_ids"]).size == 1  # a dashpot node inside a group
        assert Z["fixed"].reshape(-1, 3)[groups[4]].any()  # a member with a constrained component
        kw["tie"] = (groups, Z["tie_M"], Z["tie_P"], Z["tie_Q"])
    if correction:
        kw["p_at"] = lambda n, u: (cp * u.astype(np.float64)).astype(np.float32)
    return (apply, Z["mass"], Z["fixed"], Z["bcv"], lambda n: (base + Z["curve"][n] * pattern).astype(np.float32),
            alpha, beta, float(Z["dt"]), Z["u0"], Z["v0"]), kw


@pytest.mark.parametrize("name", list(CASES))
def test_scheme_steps_reproduces_the_recorded_words(name):
    args, kw = scheme_arguments(name)
    first, steps = CASES[name][3:5]
    record = list(xc.scheme_steps(*args, first, steps, **kw))
    assert [s.n for s in record] == list(range(first, first + steps))
    assert_bitwise(record[-1].un, FIXTURE[name + "_u"], f"{name}: u")
    assert_bitwise(record[-1].vn, FIXTURE[name + "_v"], f"{name}: v")
    # a step hands on what it stored, and host_scheme is the generator run to its end
    for a, b in zip(record, record[1:]):
        assert a.un is b.u and a.vn is b.v
    assert (record[-1].p is None) == ("p_at" not in kw)
    u, v, p = xc.host_scheme(*args, first, steps, **kw, with_p=True)
    assert_bitwise(u, record[-1].un, f"{name}: host_scheme's u")
    assert_bitwise(v, record[-1].vn, f"{name}: host_scheme's v")
    assert_bitwise(p, np.zeros_like(u) if record[-1].p is None else record[-1].p, f"{name}: host_scheme's p")


@pytest.mark.parametrize("name", ["dashpots", "ties"])
def test_a_split_run_is_the_whole_run(name):
    """3 steps, then 4 from the state they left: the 7 steps' recorded words."""
    args, kw = scheme_arguments(name)
    u, v = xc.host_scheme(*args, 0, 3, **kw)
    u, v = xc.host_scheme(*args[:-2], u, v, 3, 4, **kw)
    assert_bitwise(u, FIXTURE[name + "_u"], f"{name}: u of 3 + 4 steps")
    assert_bitwise(v, FIXTURE[name + "_v"], f"{name}: v of 3 + 4 steps")
