"""The explicit stepper, host side (no GPU): the exported entry points, the struct layouts, the damped critical step
and the load curve's evaluation."""
import ctypes as C
import math

import numpy as np
import pytest

from cwf import _lib, explicit, scenarios
from cwf.physics import Curve, evaluate_curve
from explicit_common import header_struct_size

SYMBOLS = {
    "cwf_hip_explicit_create", "cwf_hip_explicit_destroy", "cwf_hip_explicit_advance", "cwf_hip_explicit_get_state",
    "cwf_hip_explicit_set_state", "cwf_hip_explicit_set_external_force", "cwf_hip_explicit_set_load_pattern",
    "cwf_hip_explicit_set_load_curve", "cwf_hip_explicit_time", "cwf_hip_lambda_max", "cwf_explicit_critical_dt",
    "cwf_explicit_curve_value",
}


def bits(x):
    return np.float64(x).view(np.uint64)


def test_library_declares_and_exports_the_entry_points():
    L = _lib.load()
    assert SYMBOLS <= set(_lib.declared_symbols())
    for n in SYMBOLS:
        assert hasattr(L, n), n
    assert L.cwf_hip_abi_version() == 1


def test_struct_sizes_match_the_header():
    assert C.sizeof(_lib.ExplicitDescC) == header_struct_size("cwf_explicit_desc") == 4 * 8 + 2 * 4 + 2 * 8 == 56
    assert C.sizeof(_lib.ExplicitTelemetryC) == header_struct_size("cwf_explicit_telemetry") == 4 * 8 + 8 + 2 * 4 == 48
    assert _lib.ExplicitDescC.external_force.offset == 40
    assert _lib.ExplicitTelemetryC.steps.offset == 32 and _lib.ExplicitTelemetryC.finite.offset == 40


@pytest.mark.parametrize("lam", [1.0, 1.9e9, 1e12])
def test_undamped_critical_step(lam):
    assert explicit.critical_dt(lam, 0.0) == 2.0 / math.sqrt(lam)
    assert explicit.critical_dt(lam) == 2.0 / math.sqrt(lam)


@pytest.mark.parametrize("lam", [1.0, 1.9e9, 1e12])
@pytest.mark.parametrize("beta", [0.0, 1e-6, 2e-5])
def test_damped_critical_step(lam, beta):
    w = math.sqrt(lam)
    xi = beta * w / 2.0
    want = (2.0 / w) * (math.sqrt(1.0 + xi * xi) - xi)
    got = explicit.critical_dt(lam, beta)
    assert abs(got - want) <= 1e-15 * want, (got, want)
    assert got <= 2.0 / w


def test_critical_step_of_no_stiffness_is_zero():
    assert explicit.critical_dt(0.0, 0.0) == 0.0
    assert explicit.critical_dt(-1.0, 1e-6) == 0.0


def test_curve_value_is_the_packers_curve_evaluation():
    curve = scenarios.harmonic_curve(5.0)
    knots = [p[0] for p in curve.points]
    rng = np.random.Generator(np.random.PCG64(11))
    times = knots + list(rng.uniform(knots[0], knots[-1], 200 - len(knots)))
    assert len(times) == 200
    for t in times:
        assert bits(explicit.curve_value(curve, t)) == bits(evaluate_curve(curve, t)), t
    for t in (-1.0, knots[0] - 1e-12, knots[-1] + 1e-12, 10.0):
        assert bits(explicit.curve_value(curve, t)) == bits(evaluate_curve(curve, t)), t
    assert explicit.curve_value(curve, -1.0) == curve.points[0][1]
    assert explicit.curve_value(curve, 10.0) == curve.points[-1][1]


def test_curve_value_edge_cases():
    # no points: 1; one point: its value; a repeated time (a jump): the earlier segment's end value
    assert explicit.curve_value([], 0.3) == 1.0 == evaluate_curve(Curve([]), 0.3)
    assert explicit.curve_value([(0.5, 2.5)], 0.3) == 2.5 == explicit.curve_value([(0.5, 2.5)], 0.7)
    jump = Curve([(0.0, 1.0), (1.0, -3.0), (1.0, 4.0), (2.0, 5.0)])
    for t in (0.25, 0.999, 1.0, 1.0 + 1e-9, 1.5, 2.0):
        assert bits(explicit.curve_value(jump, t)) == bits(evaluate_curve(jump, t)), t
    # same-sign and opposite-sign ends take different branches of the interpolation
    same = Curve([(0.0, 0.1), (0.3, 0.7)])
    for t in np.linspace(0.0, 0.3, 37):
        assert bits(explicit.curve_value(same, float(t))) == bits(evaluate_curve(same, float(t)))


def test_null_handles_are_refused_before_any_device_call():
    L = _lib.load()
    lam = C.c_double()
    assert L.cwf_hip_lambda_max(None, 60, C.byref(lam), None) == -11
    assert L.cwf_hip_explicit_advance(None, 1, None) == -11
    assert L.cwf_hip_last_error(None).decode() == "null handle"
    d = _lib.ExplicitDescC()
    out = C.c_void_p()
    assert L.cwf_hip_explicit_create(None, C.byref(d), C.byref(out)) == -11
