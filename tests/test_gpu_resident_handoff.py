"""The resident solve's hand-off (csrc/resident.hip): a published box-surface node stores one granule {Ap, tag} per
phase, and each ring entry's r and p stay with the box that reads it, formed there by fused_form from the owner's own
inputs. The claim is identical bits, so these tests ask for identical bits.

test_bits_equal_the_recorded_build: x, r (SHA-256 of their bytes), the iteration count and the fp64 residual history
equal tests/golden/resident_handoff.json, recorded (tools/record_resident_golden.py) on a 256-CU MI355X with the build
that still published {r, tag} {Ap, tag} {p, tag} per node. Static solves from x = 0 at tol 1e-30 after 1, 2, 3 and 20
iterations of block_case(40, 17, 9), roller_case(12, 10, 7) (Dirichlet-masked components among the ring entries) and the
hex8 block_case(33, 9, 5), each also as a full solve at tol 1e-6; and after 3 and 20 iterations of block_case(55, 55,
55): 56^3 nodes, whose plan on 256 CUs (4 x 8 x 8 boxes) printed max_halo 548 while recording (CWF_VERBOSE), more than
the 512 threads, so both ring slots of a thread are live there. The box plan depends on the CU count, so the comparison skips on a device with another count
than the recorded one (256: it runs on an MI355X).

test_reread_path_same_bits: CWF_RESIDENT_REREAD=1 makes every phase take its first ring vote as failed, so every ring
granule is requested and every ring entry formed twice; the kept r and p must have taken alpha once: 20 iterations of
the four cases give the bits of the same build without the knob."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_resident_golden",
                                               os.path.join(ROOT, "tools", "record_resident_golden.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


@pytest.fixture(scope="module")
def golden():
    with open(rec.GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", sorted(rec.CASES))
def test_bits_equal_the_recorded_build(name, golden, monkeypatch):
    monkeypatch.delenv("CWF_RESIDENT_REREAD", raising=False)
    cus = rec.cu_count()
    if cus != golden["cus"]:
        pytest.skip(f"the box plan depends on the CU count: recorded on {golden['cus']} CUs, this device has {cus}")
    want, got = golden["cases"][name], rec.run_case(name)
    assert got["kernel"] == want["kernel"]
    assert sorted(got["fixed"]) == sorted(want["fixed"]) == sorted(str(n) for n in rec.CASES[name][1])
    for n in want["fixed"]:
        g, w = got["fixed"][n], want["fixed"][n]
        print(f"{name} after {n}: x {g['x'][:12]} / {w['x'][:12]}, r {g['r'][:12]} / {w['r'][:12]}, "
              f"res {g['hist'][-1]} / {w['hist'][-1]}")
        assert g["iterations"] == w["iterations"] == int(n)
        assert g["hist"] == w["hist"], (name, n)
        assert (g["x"], g["r"]) == (w["x"], w["r"]), (name, n)
    assert (got["full"] is None) == (want["full"] is None) == (not rec.CASES[name][2])
    if want["full"]:
        g, w = got["full"], want["full"]
        print(f"{name} full solve: {g['iterations']} / {w['iterations']} iterations")
        assert w["converged"] and g["converged"]
        assert g["iterations"] == w["iterations"]
        assert g["hist"] == w["hist"]
        assert (g["x"], g["r"]) == (w["x"], w["r"])


@pytest.mark.parametrize("name", sorted(rec.CASES))
def test_reread_path_same_bits(name, monkeypatch):
    from cwf import _lib, pcg, scenarios

    monkeypatch.delenv("CWF_FUSED", raising=False)
    case = rec.CASES[name][0](scenarios)
    s = pcg.MatrixFreeSystem.from_packing(case.packing, case.materials, *case.scalars(), mode=_lib.MODE_FAST)
    assert (_lib.load().cwf_hip_system_keff_kernel(s.handle()) or b"").decode().startswith("k_pcg_resident")
    rhs = case.static_rhs()
    monkeypatch.delenv("CWF_RESIDENT_REREAD", raising=False)
    plain = rec.solve(s, rhs, 20, 1e-30)
    monkeypatch.setenv("CWF_RESIDENT_REREAD", "1")  # (read at every launch)
    twice = rec.solve(s, rhs, 20, 1e-30)
    s.close()
    assert plain["iterations"] == twice["iterations"] == 20
    assert twice["hist"] == plain["hist"]
    assert (twice["x"], twice["r"]) == (plain["x"], plain["r"])
