"""The resident box image's LDS bank-conflict model and per-box stride chooser (csrc/resident_image.hpp, a host-only
header) through their C++ test program. No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "civiwave-fem_amd", "csrc")
TEST_CPP = os.path.join(ROOT, "tests", "cpp", "resident_image_test.cpp")


def _run(exe, *args, env=None):
    out = subprocess.run([exe, *args], env=env, capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().splitlines()[-1] == "ok", (out.stdout, out.stderr)


def test_image_model_and_chooser(tmp_path):
    """tests/cpp/resident_image_test.cpp: the lane groups; on the lists of 14 x 10 x 10 boxes of a 70^3 lattice 2464
    read cycles for an interior box and 4774 for an x-face box with strides (16, 192), the chooser at the floor of 1232
    for the interior box and within 1.35 x of it for the six kinds of box; over small box shapes (Kuhn and hex8, boxes
    inside the block, on a face of each axis and in a corner) never dearer than the dense strides, inside the caps,
    every slot distinct and inside the image."""
    exe = str(tmp_path / "resident_image_test")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I" + CSRC, TEST_CPP, "-o", exe], check=True)
    _run(exe)


def test_image_model_and_chooser_with_host_sanitizers(tmp_path):
    """The same program under the host compiler's address and undefined-behaviour sanitizers (their runtimes linked
    into the program), over every fourth sx of the shape sweep."""
    exe = str(tmp_path / "resident_image_test_san")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I" + CSRC, TEST_CPP,
                    "-o", exe], check=True)
    _run(exe, "4", env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
