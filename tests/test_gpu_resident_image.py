"""The resident solve's per-box LDS image strides (csrc/resident_image.hpp, chosen in csrc/resident.cpp).

Padding a box's image moves addresses only: the lists' order, every operand and every sum stay what they were. So every
comparison here is of bytes, CWF_RESIDENT_IMAGE=0 (the dense strides) against the default on fresh handles (the knob is
read when the plan is made): the same x and r, the same fp64 residual history and the same iteration count after 1, 2,
3 and 20 iterations and as a full solve. The plans: block faces on every axis with the reducer role on and off, uneven
and one-cell-thin boxes, hex8, the 4-node LDS-state instantiation (the smallest shape tests/test_gpu_resident.py runs it
at), the forced second ring pass, warm-started Stepper steps, and one run through the trace file, whose header must show
padded strides.

The last two tests are of a box's wait for the reducer's decision granule on the padded plans, compared the same way
against CWF_RESIDENT_REDUCER=0 (every box folds the shares itself: a path that wait is no part of) on one handle: 1 and
2 iterations, a zero right-hand side, and twelve solves back to back whose iteration counts alternate odd and even, so
both parity slots of the decision granule hold stale tags of earlier solves.

Not tested, on purpose: the timeout / failed paths (they need a workgroup that misses its phase)."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_resident_golden",
                                               os.path.join(ROOT, "tools", "record_resident_golden.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

IMAGE, REDUCER = "CWF_RESIDENT_IMAGE", "CWF_RESIDENT_REDUCER"
KNOBS = ("CWF_FUSED", "CWF_RESIDENT_REREAD", "CWF_RESIDENT_TRACE", "CWF_FUSED_TRACE_IT", IMAGE, REDUCER)

# name: (the case, the full solve's iteration cap, CWF_RESIDENT_REDUCER or None for the default)
PLANS = {
    "40x17x9-reducer": (rec.CASES["40x17x9"][0], 1500, "1"),
    "40x17x9-all-fold": (rec.CASES["40x17x9"][0], 1500, "0"),
    "rollers-12x10x7-reducer": (rec.CASES["rollers-12x10x7"][0], 1500, "1"),
    "rollers-12x10x7-all-fold": (rec.CASES["rollers-12x10x7"][0], 1500, "0"),
    # 34 x 10 x 6 nodes: boxes of uneven sizes; 4 x 4 x 61: boxes one cell thin
    "uneven-33x9x5": (lambda S: S.block_case(33, 9, 5, h=0.1, tol=1e-6, max_iterations=800), 800, None),
    "thin-3x3x60": (lambda S: S.block_case(3, 3, 60, h=0.1, tol=1e-6, max_iterations=2000), 2000, None),
    "hex8-33x9x5": (rec.CASES["hex8-33x9x5"][0], 800, None),
    # the C3 / 8 slab's size: k_pcg_resident<.., 4, 3, false>, r, Ap, x in LDS and little room to pad the image in
    "lds-state-149x149x19": (lambda S: S.block_case(149, 149, 19, h=0.1, tol=1e-30, max_iterations=20), 1200, None),
}


def _system(case, monkeypatch, image, reducer=None, expect=None):
    from cwf import _lib, pcg

    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    if image is not None:
        monkeypatch.setenv(IMAGE, image)
    if reducer is not None:
        monkeypatch.setenv(REDUCER, reducer)
    s = pcg.MatrixFreeSystem.from_packing(case.packing, case.materials, *case.scalars(), mode=_lib.MODE_FAST)
    # (the schedule, and with it the plan, is made at the first ask: under this environment)
    kernel = (_lib.load().cwf_hip_system_keff_kernel(s.handle()) or b"").decode()
    assert kernel.startswith(expect or "k_pcg_resident"), kernel
    return s


def _same(a, b, what):
    assert a["iterations"] == b["iterations"], what
    assert a["converged"] == b["converged"], what
    assert a["hist"] == b["hist"], what
    assert (a["x"], a["r"]) == (b["x"], b["r"]), what


@pytest.mark.parametrize("name", sorted(PLANS))
def test_padded_image_same_bits(name, monkeypatch):
    from cwf import scenarios

    make, cap, reducer = PLANS[name]
    case = make(scenarios)
    rhs = case.static_rhs()
    expect = "k_pcg_resident<true, LatKuhn, 4, 3, false>" if name.startswith("lds-state") else None
    runs = {}
    for image in ("0", None):
        s = _system(case, monkeypatch, image, reducer, expect)
        runs[image] = [rec.solve(s, rhs, its, tol) for its, tol in ((1, 1e-30), (2, 1e-30), (3, 1e-30), (20, 1e-30), (cap, 1e-6))]
        s.close()
    for dense, padded, its in zip(runs["0"], runs[None], (1, 2, 3, 20, cap)):
        print(f"{name} {its}: {dense['iterations']} / {padded['iterations']} iterations, x {dense['x'][:12]} / "
              f"{padded['x'][:12]}, res {dense['hist'][-1]} / {padded['hist'][-1]}")
        if its != cap:
            assert dense["iterations"] == its
        _same(dense, padded, (name, its))
    assert runs["0"][-1]["iterations"] > 20


def test_padded_image_with_the_forced_second_ring_pass(monkeypatch):
    from cwf import scenarios

    case = rec.CASES["40x17x9"][0](scenarios)
    rhs = case.static_rhs()
    runs = {}
    for image in ("0", None):
        s = _system(case, monkeypatch, image)
        monkeypatch.setenv("CWF_RESIDENT_REREAD", "1")  # (read at every launch)
        runs[image] = rec.solve(s, rhs, 20, 1e-30)
        s.close()
    s = _system(case, monkeypatch, None)
    plain = rec.solve(s, rhs, 20, 1e-30)
    s.close()
    assert plain["iterations"] == 20
    _same(runs["0"], runs[None], "reread, dense against padded")
    _same(plain, runs[None], "padded, one ring pass against two")


def test_padded_image_through_the_stepper(monkeypatch):
    """Two FAST Newmark steps of a small block (the second solve warm-started, x_0 != 0): the same state bytes."""
    from cwf import _lib, scenarios
    from cwf.stepper import Stepper

    case = scenarios.block_case(10, 5, 6, h=0.1, xi=0.05, w=(10.0, 100.0), tol=1e-6, max_iterations=1500)
    state = {}
    for image in ("0", None):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        if image is not None:
            monkeypatch.setenv(IMAGE, image)
        st = Stepper(case.packing, case.materials, case.rayleigh, case.cfg.solver, case.cfg.time, mode=_lib.MODE_FAST)
        assert (_lib.load().cwf_hip_system_keff_kernel(st.system.handle()) or b"").decode().startswith("k_pcg_resident")
        its = []
        for k in range(2):
            tel = st.step(0.01 * k).value()
            assert tel.pcg.converged
            its.append(tel.pcg.iterations)
        state[image] = (its, [st.get_state(w).tobytes() for w in
                              (Stepper.DISPLACEMENT, Stepper.VELOCITY, Stepper.ACCELERATION)])
    assert state["0"][0] == state[None][0] and min(state["0"][0]) > 0
    assert state["0"][1] == state[None][1]


def _image_of(header):
    """(PX, PXY, LDS bytes) of a trace header '# resident ... image PX,PXY lds BYTES boxes GXxGYxGZ'."""
    words = header.split()
    px, pxy = (int(v) for v in words[words.index("image") + 1].split(","))
    return px, pxy, int(words[words.index("lds") + 1])


def test_padded_strides_were_really_chosen(monkeypatch, tmp_path):
    """40 x 17 x 9 cells on 256 CUs (84 boxes and the reducer): the trace header of the default plan shows other strides
    for box 0 and a larger image than the header of a CWF_RESIDENT_IMAGE=0 plan, whose strides are the dense ones, and
    both solves give the same bytes."""
    from cwf import scenarios

    cus = rec.cu_count()
    if cus != 256:
        pytest.skip(f"the box plan depends on the CU count: the case is stated for 256 CUs, this device has {cus}")
    case = rec.CASES["40x17x9"][0](scenarios)
    rhs = case.static_rhs()
    seen = {}
    for image in ("0", None):
        s = _system(case, monkeypatch, image)
        path = tmp_path / f"trace_{image}.txt"
        monkeypatch.setenv("CWF_RESIDENT_TRACE", str(path))
        monkeypatch.setenv("CWF_FUSED_TRACE_IT", "2")
        out = rec.solve(s, rhs, 3, 1e-30)
        s.close()
        with open(path) as f:
            headers = [line.strip() for line in f if line.startswith("#")]
        assert len(headers) == 1 and "grid 85 " in headers[0] and headers[0].split()[-2] == "boxes", headers
        seen[image] = (_image_of(headers[0]), out)
        print(image, headers[0])
    (px0, pxy0, lds0), dense = seen["0"]
    (px1, pxy1, lds1), padded = seen[None]
    assert pxy0 % px0 == 0 and lds0 % (16 * pxy0) == 0  # dense: PXY = PX (sy + 2), the image PXY (sz + 2) slots
    assert px1 >= px0 and pxy1 >= pxy0 and (px1, pxy1) != (px0, pxy0) and lds1 > lds0
    _same(dense, padded, "traced")


# ---- a box's wait for the decision granule (the reducer role) against the all-fold path ----

def test_decision_wait_one_and_two_iterations_and_a_zero_rhs(monkeypatch):
    from cwf import pcg, scenarios

    case = rec.CASES["40x17x9"][0](scenarios)
    s = _system(case, monkeypatch, None)
    rhs = case.static_rhs()
    for its in (1, 2):
        monkeypatch.setenv(REDUCER, "0")
        off = rec.solve(s, rhs, its, 1e-30)
        monkeypatch.setenv(REDUCER, "1")
        on = rec.solve(s, rhs, its, 1e-30)
        assert off["iterations"] == its
        _same(off, on, its)
    for knob in ("0", "1"):
        monkeypatch.setenv(REDUCER, knob)
        x0 = np.zeros_like(rhs)
        t = pcg.solve_pcg(s, np.zeros_like(rhs), pcg.PcgSettings(50, 1e-6), pcg.PcgVectors(x0, None)).value()
        assert t.iterations == 0 and not x0.any()
    s.close()


def test_decision_wait_twelve_solves_of_alternating_parity(monkeypatch):
    from cwf import scenarios

    case = rec.CASES["rollers-12x10x7"][0](scenarios)
    s = _system(case, monkeypatch, None)
    rhs = case.static_rhs()
    counts = (5, 8, 3, 20, 1, 2, 7, 6, 9, 4, 11, 12)
    seq = {}
    for knob in ("1", "0"):
        monkeypatch.setenv(REDUCER, knob)
        seq[knob] = [rec.solve(s, rhs, n, 1e-30) for n in counts]
    s.close()
    for a, b, n in zip(seq["0"], seq["1"], counts):
        assert a["iterations"] == n
        _same(a, b, n)
