"""The resident solve's reducer role (csrc/resident.hip, CWF_RESIDENT_REDUCER): one extra workgroup on a spare CU polls
every box's five share granules, folds them with the boxes' own block_sum_lds, runs fused_decide once and publishes one
decision granule {alpha, beta, state, tag} that every box polls in place of sweeping, folding and deciding itself. The
claim is the same bits, so every comparison here is of bytes: knob 0 (every box folds) against knob 1 (the role wherever
the plan is eligible) on ONE handle, the knob being read at every launch.

Box counts on 256 CUs (the planner's cost function): block_case(40, 17, 9) 84 boxes (a full fold wave + 20 lanes),
roller_case(12, 10, 7) 56 (one partial wave, Dirichlet-masked components), hex8 block_case(33, 9, 5) 68 (a full wave +
4 lanes), block_case(30, 24, 24) 200 (four waves, the last with 8 lanes), block_case(55, 55, 55) 256 (no spare CU: the
role must not run). The bit comparisons hold on any device; the tests that read a plan's size from the trace skip on a
device without 256 CUs.

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

KNOB = "CWF_RESIDENT_REDUCER"
BITS_CASES = {
    "40x17x9": rec.CASES["40x17x9"][0],
    "rollers-12x10x7": rec.CASES["rollers-12x10x7"][0],
    "hex8-33x9x5": rec.CASES["hex8-33x9x5"][0],
    "30x24x24": lambda S: S.block_case(30, 24, 24, h=0.1, tol=1e-6, max_iterations=1500),
}


def _system(case, monkeypatch):
    from cwf import _lib, pcg

    for k in ("CWF_FUSED", "CWF_RESIDENT_REREAD", "CWF_RESIDENT_TRACE", KNOB):
        monkeypatch.delenv(k, raising=False)
    s = pcg.MatrixFreeSystem.from_packing(case.packing, case.materials, *case.scalars(), mode=_lib.MODE_FAST)
    assert (_lib.load().cwf_hip_system_keff_kernel(s.handle()) or b"").decode().startswith("k_pcg_resident")
    return s


def _same(a, b, what):
    assert a["iterations"] == b["iterations"], what
    assert a["converged"] == b["converged"], what
    assert a["hist"] == b["hist"], what
    assert (a["x"], a["r"]) == (b["x"], b["r"]), what


def _traces(path):
    """[(header line, rows)] of a CWF_RESIDENT_TRACE file."""
    out = []
    with open(path) as f:
        for line in f:
            if line.startswith("#"):
                out.append((line.strip(), []))
            elif line.strip():
                out[-1][1].append([int(v) for v in line.split()])
    return out


def _need_256():
    cus = rec.cu_count()
    if cus != 256:
        pytest.skip(f"the box plan depends on the CU count: the case is stated for 256 CUs, this device has {cus}")


@pytest.mark.parametrize("name", sorted(BITS_CASES))
def test_same_bits_with_and_without_the_role(name, monkeypatch):
    from cwf import scenarios

    case = BITS_CASES[name](scenarios)
    s = _system(case, monkeypatch)
    rhs = case.static_rhs()
    for its, tol in ((1, 1e-30), (2, 1e-30), (3, 1e-30), (20, 1e-30), (case.cfg.solver.max_iterations, 1e-6)):
        monkeypatch.setenv(KNOB, "0")
        off = rec.solve(s, rhs, its, tol)
        monkeypatch.setenv(KNOB, "1")
        on = rec.solve(s, rhs, its, tol)
        print(f"{name} {its} @ {tol}: {off['iterations']} / {on['iterations']} iterations, x {off['x'][:12]} / "
              f"{on['x'][:12]}, res {off['hist'][-1]} / {on['hist'][-1]}")
        if tol == 1e-30:
            assert off["iterations"] == its
        else:
            assert off["converged"]
        _same(off, on, (name, its, tol))
    s.close()


def test_the_role_really_ran(monkeypatch, tmp_path):
    from cwf import scenarios

    _need_256()
    case = BITS_CASES["40x17x9"](scenarios)
    s = _system(case, monkeypatch)
    rhs = case.static_rhs()
    path = tmp_path / "trace.txt"
    monkeypatch.setenv("CWF_RESIDENT_TRACE", str(path))
    monkeypatch.setenv("CWF_FUSED_TRACE_IT", "2")
    monkeypatch.setenv(KNOB, "1")
    rec.solve(s, rhs, 3, 1e-30)
    monkeypatch.setenv(KNOB, "0")
    rec.solve(s, rhs, 3, 1e-30)
    s.close()
    (h1, r1), (h0, r0) = _traces(path)
    print(h1, len(r1), "|", h0, len(r0))
    assert "grid 85 " in h1 and "reducer 1 " in h1 and len(r1) == 85
    assert "grid 84 " in h0 and "reducer 0 " in h0 and len(r0) == 84
    # the reducer's row: its five stamps of the traced phase, in order; a box's row has its decision-seen stamp
    red = r1[84]
    assert red[0] == 84 and 0 < red[1] <= red[2] <= red[3] <= red[4] and red[3] <= red[5]
    assert all(0 < row[1] <= row[2] <= row[3] for row in r1[:84])


def test_no_spare_cu_keeps_every_box_folding(monkeypatch, tmp_path):
    from cwf import scenarios

    _need_256()
    case = rec.CASES["55x55x55"][0](scenarios)
    s = _system(case, monkeypatch)
    rhs = case.static_rhs()
    monkeypatch.setenv(KNOB, "0")
    off = {n: rec.solve(s, rhs, n, 1e-30) for n in (3, 20)}
    path = tmp_path / "trace.txt"
    monkeypatch.setenv("CWF_RESIDENT_TRACE", str(path))
    monkeypatch.setenv(KNOB, "1")
    on = {n: rec.solve(s, rhs, n, 1e-30) for n in (3, 20)}
    s.close()
    for hdr, rows in _traces(path):
        print(hdr, len(rows))
        assert "grid 256 " in hdr and "reducer 0 " in hdr and len(rows) == 256
    for n in (3, 20):
        assert on[n]["iterations"] == n
        _same(off[n], on[n], n)


def test_stops_through_the_reducer(monkeypatch):
    from cwf import pcg, scenarios

    case = BITS_CASES["40x17x9"](scenarios)
    s = _system(case, monkeypatch)
    rhs = case.static_rhs()
    monkeypatch.setenv(KNOB, "1")
    x, r = np.zeros_like(rhs), np.zeros_like(rhs)
    t = pcg.solve_pcg(s, rhs, pcg.PcgSettings(7, 1e-12), pcg.PcgVectors(x, r)).value()
    assert (t.iterations, t.converged) == (7, False)
    h = pcg.residual_history(s)
    assert len(h) - 1 == 7 and np.all(np.isfinite(h)) and h[-1] == t.residual_norm
    # a zero right-hand side: the solve returns at once, x as it was
    x0 = np.zeros_like(rhs)
    t = pcg.solve_pcg(s, np.zeros_like(rhs), pcg.PcgSettings(50, 1e-6), pcg.PcgVectors(x0, None)).value()
    assert t.iterations == 0 and not x0.any()
    # three solves back to back: the tag base advances across them, the decision granules of an earlier solve never match
    seq = {}
    for knob in ("1", "0"):
        monkeypatch.setenv(KNOB, knob)
        seq[knob] = [rec.solve(s, rhs, n, 1e-30) for n in (5, 20, 5)]
    s.close()
    for a, b, n in zip(seq["0"], seq["1"], (5, 20, 5)):
        assert a["iterations"] == n
        _same(a, b, n)
    _same(seq["1"][0], seq["1"][2], "the first and the third solve")


def test_with_the_forced_second_ring_pass(monkeypatch):
    from cwf import scenarios

    case = BITS_CASES["40x17x9"](scenarios)
    s = _system(case, monkeypatch)
    rhs = case.static_rhs()
    monkeypatch.setenv(KNOB, "1")
    plain = rec.solve(s, rhs, 20, 1e-30)
    monkeypatch.setenv("CWF_RESIDENT_REREAD", "1")
    twice = rec.solve(s, rhs, 20, 1e-30)
    s.close()
    assert plain["iterations"] == 20
    _same(plain, twice, "reread")


def test_through_the_stepper(monkeypatch):
    """Two FAST Newmark steps of a small block (the second solve warm-started, x_0 != 0): the same state bytes."""
    from cwf import _lib, scenarios
    from cwf.stepper import Stepper

    for k in ("CWF_FUSED", "CWF_RESIDENT_REREAD", "CWF_RESIDENT_TRACE"):
        monkeypatch.delenv(k, raising=False)
    case = scenarios.block_case(10, 5, 6, h=0.1, xi=0.05, w=(10.0, 100.0), tol=1e-6, max_iterations=1500)
    state = {}
    for knob in ("0", "1"):
        monkeypatch.setenv(KNOB, knob)
        st = Stepper(case.packing, case.materials, case.rayleigh, case.cfg.solver, case.cfg.time, mode=_lib.MODE_FAST)
        assert (_lib.load().cwf_hip_system_keff_kernel(st.system.handle()) or b"").decode().startswith("k_pcg_resident")
        its = []
        for k in range(2):
            tel = st.step(0.01 * k).value()
            assert tel.pcg.converged
            its.append(tel.pcg.iterations)
        state[knob] = (its, [st.get_state(w).tobytes() for w in
                             (Stepper.DISPLACEMENT, Stepper.VELOCITY, Stepper.ACCELERATION)])
    assert state["0"][0] == state["1"][0] and min(state["0"][0]) > 0
    assert state["0"][1] == state["1"][1]
