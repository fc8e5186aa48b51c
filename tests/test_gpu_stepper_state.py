"""The state core the Newmark stepper and the explicit stepper share (csrc/abi_transient.cpp; cwf.transient): the
same C entry points on both, their refusals with the messages they have always returned, what stays with each
stepper, and the one load-pattern rounding both go through. The 8 x 3 x 4 block, on a renumbered FAST handle (the
spans cross the handle's node permutation both ways) and on a PARITY handle."""
import ctypes as C

import numpy as np
import pytest

from cwf import _lib, pcg, scenarios
from cwf.explicit import ExplicitStepper
from cwf.physics import RayleighCoefficients
from cwf.stepper import Stepper

pytestmark = pytest.mark.gpu

ERR_SIZE, ERR_ARGUMENT, ERR_UNSUPPORTED = -1, -11, -13
PREFIX = {"newmark": "cwf_hip_stepper", "explicit": "cwf_hip_explicit"}
_case = []


def block():
    if not _case:
        _case.append(scenarios.block_case(8, 3, 4, h=0.1))
    return _case[0]


def new_system(handle_kind, monkeypatch):
    """A handle of its own per stepper: a FAST one that renumbers (the fan-group layout: Morton order), or PARITY."""
    case = block()
    if handle_kind == "fast-renumbered":
        monkeypatch.setenv("CWF_LATTICE", "0")
    s = pcg.MatrixFreeSystem.from_packing(case.packing, case.materials, 1.0, 0.0,
                                          mode=_lib.MODE_FAST if handle_kind == "fast-renumbered" else _lib.MODE_PARITY)
    if handle_kind == "fast-renumbered":  # only a renumbered handle refuses PARITY (test_gpu_renumber)
        assert _lib.load().cwf_hip_system_set_mode(s.handle(), _lib.MODE_PARITY) == ERR_UNSUPPORTED
    return s


def new_stepper(which, s):
    case = block()
    if which == "newmark":
        return Stepper(case.packing, case.materials, case.rayleigh, case.cfg.solver, case.cfg.time, mode=s.mode,
                       system=s)
    return ExplicitStepper(case.packing, case.materials, RayleighCoefficients(0.0, 0.0), mode=s.mode, system=s)


def call(t, name, *args):
    """(status, message, context) of <prefix>_<name>(handle, *args)."""
    rc = getattr(_lib.load(), f"{t._PREFIX}_{name}")(t._raw(), *args)
    msg, ctx = _lib.last_error(t.system._h)
    return rc, msg, ctx


@pytest.mark.parametrize("handle_kind", ["fast-renumbered", "parity"])
@pytest.mark.parametrize("which", ["newmark", "explicit"])
def test_state_entry_points(which, handle_kind, monkeypatch):
    s = new_system(handle_kind, monkeypatch)
    t = new_stepper(which, s)
    assert t._PREFIX == PREFIX[which]
    D = t.dof_count
    rng = np.random.Generator(np.random.PCG64(11))
    f32 = np.zeros(D + 3, np.float32)
    f64 = np.zeros(D + 3, np.float64)
    H = _lib.PTR_HOST

    # a wrong span length: CWF_ERR_SIZE and the message each call has always returned
    for n in (D - 3, D + 3):
        assert call(t, "get_state", 0, _lib.ptr(f32), n, H)[:2] == (ERR_SIZE, "state span size mismatch")
        assert call(t, "set_state", 0, _lib.ptr(f32), n, H)[:2] == (ERR_SIZE, "state span size mismatch")
        assert call(t, "set_external_force", _lib.ptr(f32), n, H)[:2] == (ERR_SIZE,
                                                                          "external force span size mismatch")
        assert call(t, "set_load_pattern", _lib.ptr(f64), _lib.ptr(f64), n) == (
            ERR_SIZE, "load pattern span size mismatch", [f"input={n}", f"dofs={D}"])
    # the span is checked before the field: a wrong length with an unknown field is still a size error
    assert call(t, "get_state", 7, _lib.ptr(f32), D - 3, H)[0] == ERR_SIZE
    # an unknown field
    assert call(t, "get_state", 7, _lib.ptr(f32), D, H)[:2] == (ERR_ARGUMENT, "unknown state field")
    assert call(t, "set_state", 7, _lib.ptr(f32), D, H)[:2] == (ERR_ARGUMENT, "unknown state field")
    # NULL spans and NULL handles never reach a handle's record
    assert call(t, "get_state", 0, None, D, H)[0] == ERR_ARGUMENT
    assert getattr(_lib.load(), f"{t._PREFIX}_get_state")(None, 0, _lib.ptr(f32), D, H) == ERR_ARGUMENT
    assert _lib.last_error(None)[0] == "null pointer"

    # u and v come back bit for bit through the handle's node order
    for field in (t.DISPLACEMENT, t.VELOCITY):
        x = (1e-3 * rng.standard_normal(D)).astype(np.float32)
        t.set_state(field, x)
        assert np.array_equal(t.get_state(field).view(np.uint32), x.view(np.uint32))

    f = (1e2 * rng.standard_normal(D)).astype(np.float32)
    t.set_external_force(f)
    assert np.array_equal(t.get_state(t.EXTERNAL_FORCE).view(np.uint32), f.view(np.uint32))

    if which == "explicit":
        # the force is a field to read, not one to set as state; the scheme keeps no acceleration
        assert call(t, "set_state", 4, _lib.ptr(f32), D, H)[:2] == (ERR_ARGUMENT, "unknown state field")
        assert call(t, "get_state", 2, _lib.ptr(f32), D, H)[:2] == (ERR_ARGUMENT, "unknown state field")
        assert call(t, "get_state", 4, _lib.ptr(f32), D, H)[0] == 0
    else:
        # field 3 is the handle's own x: what a solve on the handle left there
        a = (1e-3 * rng.standard_normal(D)).astype(np.float32)
        t.set_state(Stepper.ACCELERATION, a)
        assert np.array_equal(t.get_state(Stepper.ACCELERATION).view(np.uint32), a.view(np.uint32))
        case = block()
        rhs = case.static_rhs()
        x, r = np.zeros(D, np.float32), np.zeros(D, np.float32)
        pcg.solve_pcg(s, rhs, pcg.PcgSettings(400, 1e-6, False), pcg.PcgVectors(x, r)).value()
        assert np.any(x != 0)
        assert np.array_equal(t.get_state(Stepper.SOLUTION).view(np.uint32), x.view(np.uint32))
        y = (1e-3 * rng.standard_normal(D)).astype(np.float32)
        t.set_state(Stepper.SOLUTION, y)
        assert np.array_equal(t.get_state(Stepper.SOLUTION).view(np.uint32), y.view(np.uint32))

    ct, dt = t._times()
    assert (t.current_time(), t.time_step()) == (ct, dt) and dt > 0.0
    t.close()
    t.close()  # a second close is a no-op
    s.close()


@pytest.mark.parametrize("handle_kind", ["fast-renumbered", "parity"])
def test_load_pattern_rounds_the_same_on_both_steppers(handle_kind, monkeypatch):
    """Newmark set_load_scale(c) and the explicit stepper after one step under the constant curve c both form
    f32(base + c pattern) with stepper_scaled_load: get_state(4) agrees bit for bit (and with numpy's fp64)."""
    D = block().packing.dof_count
    rng = np.random.Generator(np.random.PCG64(5))
    base = 10.0 * rng.standard_normal(D)
    pattern = 3.0 * rng.standard_normal(D)
    c = 0.7321
    got = {}
    for which in ("newmark", "explicit"):
        s = new_system(handle_kind, monkeypatch)
        t = new_stepper(which, s)
        t.set_load_pattern(base, pattern)
        if which == "newmark":
            t.set_load_scale(c)
        else:
            t.set_load_curve([(0.0, c), (1.0, c)])
            assert t.advance(1).value().steps == 1
        got[which] = t.get_state(4)
        t.close()
        s.close()
    assert np.array_equal(got["newmark"].view(np.uint32), got["explicit"].view(np.uint32))
    # base + c * pattern in fp64, rounded once: a contracted fp64 multiply-add may differ in the last f32 bit
    want = (base + c * pattern).astype(np.float32)
    assert np.all(np.abs(got["newmark"] - want) <= np.spacing(np.abs(want)))
