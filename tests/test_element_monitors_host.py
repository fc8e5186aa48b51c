"""The host side of the explicit stepper's element monitors (include/cwf_hip.h "Element monitors"): the effective
shear strain against the principal strains, the envelopes' update rule, the soil column of the physical check decided
with the all-float64 dense run, the C structs' layout and the driver's refusal. No GPU."""
import ctypes as C

import numpy as np
import pytest

import element_monitors_common as ec
from cwf import _lib, explicit, run


def random_strains(n=1000, seed=11):
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.standard_normal((n, 6)) * 10.0 ** rng.uniform(-6.0, -2.0, (n, 1))


def test_effective_shear_strain_is_two_sqrt_j2():
    e = random_strains()
    got, want = ec.effective_shear(e), ec.two_sqrt_j2(e)
    rel = np.abs(got - want) / want
    print(f"1,000 random symmetric tensors: worst relative difference {rel.max():.2e}")
    assert np.all(rel <= 1e-12)
    # the package's helper is the same statement order: same bits
    assert np.array_equal(explicit.effective_shear_strain(e).view(np.uint64), got.view(np.uint64))


def test_effective_shear_strain_is_gamma_in_pure_shear():
    gammas = np.array([1e-6, -3.5e-4, 2.0e-3, -1.0])
    for k in (3, 4, 5):
        e = np.zeros((gammas.size, 6))
        e[:, k] = gammas
        assert np.array_equal(ec.effective_shear(e), np.abs(gammas))
    # a volumetric strain has none
    assert np.array_equal(ec.effective_shear(np.array([[2e-4, 2e-4, 2e-4, 0.0, 0.0, 0.0]])), [0.0])


def test_update_rule_keeps_extrema_and_ignores_nan():
    ref = ec.EnvelopeReference(3)
    assert np.all(ref.von_mises == 0.0) and not np.signbit(ref.von_mises).any()
    assert np.all(ref.stress_min == np.inf) and np.all(ref.stress_max == -np.inf)
    f = np.zeros((3, 13), np.float32)
    f[:, 6:12] = [[-1.0] * 6, [2.0] * 6, [np.nan] * 6]
    f[:, 12] = [1.0, 2.0, np.nan]
    ref.add(f, np.array([0.5, np.nan, 0.25], np.float32))
    g = f.copy()
    g[:, 6:12] = [[3.0] * 6, [-4.0] * 6, [0.0] * 6]
    g[:, 12] = [0.5, 3.0, 0.0]
    ref.add(g, np.array([0.25, 1.0, np.nan], np.float32))
    assert ref.von_mises.tolist() == [1.0, 3.0, 0.0] and ref.shear_strain.tolist() == [0.5, 1.0, 0.25]
    assert ref.stress_min[:, 0].tolist() == [-1.0, -4.0, 0.0] and ref.stress_max[:, 0].tolist() == [3.0, 2.0, 0.0]
    assert ref.samples == 2


def test_strain_restatement_on_a_rigid_rotation_and_a_uniform_shear():
    """A displacement field linear in x has the same strain in every element: the restatement returns it."""
    from cwf import scenarios

    for element in ("tet4", "hex8"):
        case = scenarios.block_case(3, 2, 2, h=0.1, element=element)
        X = case.mesh.coords
        H = np.array([[1e-4, 3e-4, 0.0], [-1e-4, 2e-4, 5e-5], [2e-4, 0.0, -3e-4]])
        u = (X @ H.T).reshape(-1)
        e = ec.element_strain64(case.packing, u)
        want = np.array([H[0, 0], H[1, 1], H[2, 2], H[0, 1] + H[1, 0], H[1, 2] + H[2, 1], H[0, 2] + H[2, 0]])
        assert e.shape == (case.packing.element_count, 6)
        assert np.abs(e - want).max() <= 1e-6 * np.abs(want).max(), element  # f32 gradients


def test_the_24_cell_column_has_no_overlap_free_element_and_the_48_cell_one_has():
    """The decision the GPU check rests on (test_gpu_element_monitors.test_soil_column_peak_shear_strain), with the
    all-float64 dense run: absorbing_common's 24-cell column is shorter than the pulse, so the up-going and the
    reflected pulse overlap in every element; in the lower half of a 48-cell column (441 nodes) they do not, and there
    the fp64 run's own peak effective shear strain is max |v_inc| / V_s within the discretisation error of a pulse
    with sigma = 6 h on linear tets. Measured: 5.5e-3 relative (the bound below is a sanity bound, not the figure)."""
    assert not ec.column_clear_elements(ec.column_case(24), 24).any()
    case = ec.column_case()
    clear = ec.column_clear_elements(case, ec.COLUMN_NZ)
    assert case.packing.node_count == 441 and clear.sum() == case.packing.element_count // 2
    env, R = ec.column_envelope_f64(ec.column_dt_estimate())
    target = ec.column_target(R)
    dev = float(np.abs(env[clear] - target).max() / target)
    print(f"48-cell column, fp64 dense run, {R['steps'] + 1} steps: max |v_inc| / V_s = {target:.6e}; peak effective "
          f"shear strain of the {int(clear.sum())} overlap-free elements deviates by at most {dev:.3e} relative")
    assert 0.0 < dev < 0.05
    # where the pulses meet (under the free surface) the envelope is nowhere near: the choice of elements matters
    assert np.abs(env[~clear] - target).max() / target > 0.5


def test_struct_layout_and_entry_points():
    assert C.sizeof(_lib.ExplicitElementMonitorDescC) == 48 and C.sizeof(_lib.ExplicitElementMonitorInfoC) == 64
    assert (_lib.ENVELOPE_VON_MISES, _lib.ENVELOPE_SHEAR_STRAIN, _lib.ENVELOPE_STRESS_RANGE) == (1, 2, 4)
    header = open(_lib.HEADER_PATH).read()
    for name in ("set_element_monitors", "reset_element_monitors", "element_monitor_info", "read_gauges",
                 "read_envelopes"):
        assert f"int cwf_hip_explicit_{name}(" in header
    L = _lib.load()
    d = _lib.ExplicitElementMonitorDescC()
    assert L.cwf_hip_explicit_set_element_monitors(None, C.byref(d)) == -11  # CWF_ERR_ARGUMENT
    assert _lib.last_error(None)[0] == "null handle"
    assert L.cwf_hip_explicit_read_envelopes(None, None, None, None, None, 0, _lib.PTR_HOST) == -11


def test_refusals_on_the_host(tmp_path):
    """tests/cpp/element_monitor_refusal_test.cpp: every refusal of cwf_hip_explicit_set_element_monitors with its
    message and context, the order of the checks and the descs that pass, through element_monitor_refusal
    (abi_internal.hpp) on descs the program builds. No GPU call; built the way test_host's create_host_test is."""
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.dirname(_lib.LIB_PATH)
    exe = str(tmp_path / "element_monitor_refusal_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    "-I" + os.path.join(root, "civiwave-fem_amd", "csrc"),
                    os.path.join(root, "tests", "cpp", "element_monitor_refusal_test.cpp"), "-o", exe, f"-L{libdir}",
                    "-lcwf_hip", f"-Wl,-rpath,{libdir}"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout, out.stderr)


def test_newmark_refuses_the_element_monitor_flags(capsys):
    import os

    yaml = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data", "cantilever.yaml")
    for flag in (["--envelope-every", "2"], ["--gauges", "0,5"], ["--gauge-every", "3"]):
        assert run.main([yaml, "--steps", "1", *flag]) == 1
        assert "belong to the explicit integrator" in capsys.readouterr().err
    assert run.main([yaml, "--integrator", "explicit", "--steps", "1", "--gauges", "0,x"]) == 1
    assert "--gauges takes element numbers" in capsys.readouterr().err
