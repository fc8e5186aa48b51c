"""Modal analysis, host side (no GPU): the Rayleigh-Ritz step's C++ test program, the Python settings and the
Rayleigh helper."""
import ctypes as C
import os
import subprocess

import pytest

from cwf import _lib, modal, physics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "civiwave-fem_amd", "csrc")
TEST_CPP = os.path.join(ROOT, "tests", "cpp", "modal_host_test.cpp")


def test_ritz_host_program_against_the_library(tmp_path):
    """tests/cpp/modal_host_test.cpp over the functions libcwf_hip.so ships (Cholesky of the scaled Mr + cyclic
    Jacobi): a 12 x 12 pair with known eigenvalues, a pair with repeated ones and a nearly singular Mr; eigenvalues,
    Q^T Mr Q = I and Q^T Kr Q = Theta to 1e-12."""
    libdir = os.path.join(ROOT, "civiwave-fem_amd", "lib")
    exe = str(tmp_path / "modal_host_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I" + CSRC, TEST_CPP, "-o", exe, f"-L{libdir}", "-lcwf_hip",
                    f"-Wl,-rpath,{libdir}"], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True)
    print(out.stdout)
    assert out.stdout.strip().endswith("ok")


def test_ritz_host_program_stand_alone_with_host_sanitizers(tmp_path):
    """The same program built stand-alone with csrc/modal_ritz.cpp (plain C++, no device code) under the host
    compiler's address and undefined-behaviour sanitizers (their runtimes linked into the program)."""
    exe = str(tmp_path / "modal_host_test_san")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I" + CSRC, TEST_CPP,
                    os.path.join(CSRC, "modal_ritz.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    out = subprocess.run([exe], env=env, check=True, capture_output=True, text=True)
    assert out.stdout.strip().endswith("ok"), out.stdout + out.stderr


@pytest.mark.parametrize("xi,wi,wj", [(0.02, 5.0, 50.0), (0.05, 12.5, 13.0), (0.001, 311.7, 2950.25)])
def test_rayleigh_from_modes_equals_compute_rayleigh(xi, wi, wj):
    got = modal.rayleigh_from_modes(xi, wi, wj)
    ref = physics.compute_rayleigh(physics.Damping(xi, wi, wj))
    assert (got.alpha, got.beta) == (ref.alpha, ref.beta)
    # the damping ratio alpha / (2 w) + beta w / 2 is xi at both frequencies
    for w in (wi, wj):
        assert abs(got.alpha / (2 * w) + got.beta * w / 2 - xi) <= 1e-15 + 1e-12 * xi


def test_modal_settings_defaults_are_the_documented_ones():
    s = modal.ModalSettings()
    assert (s.block, s.max_outer, s.tolerance, s.shift) == (0, 40, 1.0e-6, 0.0)
    assert (s.pcg.max_iterations, s.pcg.relative_tolerance) == (20000, 1.0e-6)
    # q = min(2 k, k + 8), capped at the 32 columns a block holds
    assert [modal.default_block(k) for k in (1, 3, 6, 8, 9, 16, 24, 28, 32)] == [2, 6, 12, 16, 17, 24, 32, 32, 32]
    # the ctypes mirrors have the header's layout: 4 u32 + 2 f64 + cwf_pcg_settings; 4 u32 + u64 + 3 f64
    assert C.sizeof(_lib.ModalSettingsC) == 16 + 16 + C.sizeof(_lib.PcgSettingsC) == 56
    assert C.sizeof(_lib.ModalTelemetryC) == 48
    header = open(_lib.HEADER_PATH).read()
    assert "#define CWF_MODAL_MAX_BLOCK 32" in header and modal.MAX_BLOCK == 32
    assert {"cwf_hip_modal_solve", "cwf_hip_block_gram", "cwf_hip_block_rotate"} <= set(_lib.declared_symbols())
