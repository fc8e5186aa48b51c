"""The refined solve, host side (no GPU): the exported entry points, the Python settings' defaults and the
power-of-two scale."""
import ctypes as C

import numpy as np
import pytest

from cwf import _lib, pcg

TINY = 5e-324  # the smallest subnormal


def test_library_exports_the_entry_points_and_the_scale_helper():
    L = _lib.load()
    names = {"cwf_hip_solve_refined", "cwf_hip_residual_f64", "cwf_refine_scale_exponent"}
    assert names <= set(_lib.declared_symbols())
    for n in names:
        assert hasattr(L, n)
    # the ctypes mirrors have the header's layout: u32 (+ pad) + 2 f64 + cwf_pcg_settings + 2 i32;
    # u32 (+ pad) + u64 + 2 f64 + 2 i32 + 32 f64 + 2 f64
    assert C.sizeof(_lib.RefineSettingsC) == 8 + 16 + C.sizeof(_lib.PcgSettingsC) + 8 == 56
    assert C.sizeof(_lib.RefineTelemetryC) == 8 + 8 + 16 + 8 + 32 * 8 + 16 == 312
    assert _lib.RefineTelemetryC.history.offset == 40


def test_refine_settings_defaults_are_the_documented_ones():
    s = pcg.RefineSettings()
    assert (s.max_outer, s.relative_tolerance, s.stagnation_ratio, s.warm_start) == (12, 1.0e-10, 0.5, False)
    assert (s.inner.max_iterations, s.inner.relative_tolerance) == (20000, 1.0e-4)
    header = open(_lib.HEADER_PATH).read()
    for text in ("0 -> 12", "0 -> 1e-10", "0 -> 0.5", "0 -> 1e-4", "0 -> 20000"):
        assert text in header, text


@pytest.mark.parametrize("bnorm", [4.5e4, 1.0, 3.0e-7, 2.0 ** 40])
@pytest.mark.parametrize("rel", [1.0, 1e-3, 1e-12, "subnormal", 0.0])
def test_scale_brings_the_residual_to_the_right_hand_sides_binade(bnorm, rel):
    rnorm = TINY * 3 if rel == "subnormal" else rel * bnorm
    e = pcg.refine_scale_exponent(rnorm, bnorm)
    if rnorm == 0.0:
        assert e == 0
        return
    scaled = float(np.ldexp(np.float64(rnorm), e))  # exact: a power of two, no overflow at these sizes
    assert bnorm / 2 <= scaled <= 2 * bnorm, (rnorm, bnorm, e, scaled)
    # a vector of that norm scaled by 2^e and back is the identity bit for bit, entries far below the norm included
    rng = np.random.Generator(np.random.PCG64(5))
    v = rng.uniform(-1.0, 1.0, 64) * rnorm
    v[:8] *= 2.0 ** -40
    back = np.ldexp(np.ldexp(v, e), -e)
    assert np.array_equal(back.view(np.uint64), v.view(np.uint64))


def test_scale_without_a_right_hand_side_norm():
    # |b| = 0 with non-zero prescribed values: the residual goes to the binade of 1
    for rnorm in (3.0e-9, 7.0e5, TINY):
        e = pcg.refine_scale_exponent(rnorm, 0.0)
        assert 0.5 <= float(np.ldexp(np.float64(rnorm), e)) <= 2.0
    assert pcg.refine_scale_exponent(0.0, 0.0) == 0
    assert pcg.refine_scale_exponent(float("nan"), 1.0) == 0
    assert pcg.refine_scale_exponent(float("inf"), 1.0) == 0


def test_null_arguments_are_refused_before_any_device_call():
    L = _lib.load()
    x = np.zeros(3)
    assert L.cwf_hip_solve_refined(None, _lib.ptr(x), None, _lib.ptr(x), 3, 0, None) == -11
    assert L.cwf_hip_residual_f64(None, _lib.ptr(x), _lib.ptr(x), None, 3, 0, None) == -11
    assert L.cwf_hip_last_error(None).decode() == "null handle"
