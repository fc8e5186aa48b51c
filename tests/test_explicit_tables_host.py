"""The explicit stepper's host table builders (csrc/explicit_tables.cpp: the load sources' CSR, plasticity's slots and
node-major corner positions) through their C++ test program. No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "civiwave-fem_amd", "csrc")
TEST_CPP = os.path.join(ROOT, "tests", "cpp", "explicit_tables_test.cpp")


def test_tables_host_program_against_the_library(tmp_path):
    """tests/cpp/explicit_tables_test.cpp over the functions libcwf_hip.so ships: two sources over five nodes with a
    shared node and a permuted node order, one source of one node, two tets sharing a face with one and with both
    materials plastic, a dropped corner (refused) and a mesh without a plastic element (empty tables)."""
    libdir = os.path.join(ROOT, "civiwave-fem_amd", "lib")
    exe = str(tmp_path / "explicit_tables_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I" + CSRC, TEST_CPP, "-o", exe, f"-L{libdir}", "-lcwf_hip",
                    f"-Wl,-rpath,{libdir}"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout, out.stderr)


def test_tables_host_program_stand_alone_with_host_sanitizers(tmp_path):
    """The same program built stand-alone with csrc/explicit_tables.cpp (plain C++, no device code) under the host
    compiler's address and undefined-behaviour sanitizers (their runtimes linked into the program)."""
    exe = str(tmp_path / "explicit_tables_test_san")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I" + CSRC, TEST_CPP,
                    os.path.join(CSRC, "explicit_tables.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    out = subprocess.run([exe], env=env, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout, out.stderr)
