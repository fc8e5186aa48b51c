"""Every layout cwf_hip_system_create can build (abi.cpp choose_fast_path), reached by its input or by its knob:
the kernel the handle reports, its FAST apply_keff against the CPU oracle, and the layout counters
(cwf_hip_system_memory, cwf_hip_system_keff_traffic) against tests/golden/create_layout.json
(tests/golden/make_create_layout.py wrote it from these same cases)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import oracle as O
from cwf import _lib, pcg, scenarios
from helpers import oracle_system
from test_hex8 import D_STEEL, hex_case

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "create_layout.json")
LATTICE = ("k_pcg_resident", "k_pcg_lattice", "k_keff_lattice")

# name -> (mesh, variant, knobs, kernel-name prefixes, substring the name must also hold)
# The jittered 7x6x5 block (336 nodes, 1,260 tets) is several tiles at every tile size in use.
CASES = {
    "lattice-tet4": ("block", "", {}, LATTICE, "LatKuhn"),
    "lattice-hex8": ("hex", "", {}, LATTICE, "LatHex"),
    "fan-groups": ("jitter", "", {}, ("k_keff_groups_pipe",), ""),
    "tiles-pipe-17-materials": ("jitter", "materials17", {}, ("k_keff_tiles_pipe",), ""),
    "tiles-pipe-knob": ("jitter", "", {"CWF_GROUPS": "0"}, ("k_keff_tiles_pipe",), ""),
    "records-no-coords": ("jitter", "no_coords", {}, ("k_keff_tiles",), ""),
    "records-knob": ("jitter", "", {"CWF_GEO": "0"}, ("k_keff_tiles",), ""),
    "one-tile-per-workgroup": ("jitter", "", {"CWF_GROUPS": "0", "CWF_TILE_PIPE": "0"}, ("k_keff_tiles",), ""),
    "hex-tiles": ("hex", "", {"CWF_LATTICE": "0"}, ("k_keff_hex_tiles",), ""),
    "caller-order-flag": ("jitter", "keep_order", {}, ("k_keff_groups_pipe",), ""),
    "caller-order-knob": ("jitter", "", {"CWF_RENUMBER": "0"}, ("k_keff_groups_pipe",), ""),
}
KNOBS = sorted({k for c in CASES.values() for k in c[2]})

_meshes = {}


def mesh_case(kind):
    if kind not in _meshes:
        _meshes[kind] = {"block": lambda: scenarios.block_case(8, 3, 4, h=0.1),
                         "hex": lambda: hex_case(6, 4, 3),
                         "jitter": lambda: scenarios.block_case(7, 6, 5, h=0.1, jitter=True)}[kind]()
    return _meshes[kind]


def build(name):
    """(FAST system, oracle apply_keff) of a case; the case's knobs must already be in the environment."""
    kind, variant, _, _, _ = CASES[name]
    case = mesh_case(kind)
    P = case.packing
    sK, sM = case.scalars()
    materials, mat = case.materials, P.material_index
    if variant == "materials17":  # 17 copies of the one stiffness: the same operator, past the 16 the groups hold
        materials, mat = materials * 17, (np.arange(P.element_count) % 17).astype(np.uint32)
    coords = P.position64 if getattr(P, "position64", None) is not None else P.position0
    s = pcg.MatrixFreeSystem(P.connectivity, P.gradients, P.volume, mat, materials, P.lumped_mass, P.bc_mask,
                             P.node_count, P.element_count, P.dof_count, sK, sM, P.reduction_block,
                             P.reduction_partials, (P.offsets, P.element_indices, P.local_indices), _lib.MODE_FAST, 0,
                             None if variant == "no_coords" else coords,
                             keep_node_order=variant == "keep_order")
    if kind == "hex":
        return s, lambda x: O.hex8_apply(case.mesh.coords, case.mesh.tets, mat, D_STEEL, sK, sM, P.lumped_mass,
                                         P.bc_mask, x)
    packed = O.Packed(P.node_count, P.element_count, P.connectivity, P.gradients, P.volume, mat, P.lumped_mass64,
                      P.lumped_mass, P.offsets, P.element_indices, P.local_indices)
    stiff = np.concatenate([np.asarray(m.stiffness, np.float64).reshape(-1) for m in materials])
    return s, O.System(packed, stiff, P.bc_mask, sK, sM, 256).apply_keff


def kernel_name(s):
    return (_lib.load().cwf_hip_system_keff_kernel(s.handle()) or b"").decode()


def layout_counters(s):
    """The integers create's host layout code decides: device bytes and the K_eff pass's modelled traffic."""
    L = _lib.load()
    mem, lay, ref = C.c_uint64(), C.c_uint64(), C.c_uint64()
    assert L.cwf_hip_system_memory(s.handle(), C.byref(mem)) == 0
    assert L.cwf_hip_system_keff_traffic(s.handle(), C.byref(lay), C.byref(ref)) == 0
    return {"memory": mem.value, "traffic": lay.value, "reference_traffic": ref.value}


@pytest.mark.parametrize("name", sorted(CASES))
def test_create_path(name, monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in CASES[name][2].items():
        monkeypatch.setenv(k, v)
    s, ref_apply = build(name)
    kern = kernel_name(s)
    prefixes, holds = CASES[name][3], CASES[name][4]
    assert kern.startswith(prefixes) and holds in kern, kern
    if prefixes == ("k_keff_tiles",):
        assert not kern.startswith("k_keff_tiles_pipe"), kern
    counters = layout_counters(s)
    x = np.random.Generator(np.random.PCG64(3)).uniform(-1, 1, s.dof_count).astype(np.float32)
    y = np.zeros_like(x)
    pcg.apply_keff(s, x, y).value()
    ref = ref_apply(x).astype(np.float64)
    err, scale = float(np.max(np.abs(y - ref))), float(np.max(np.abs(ref)))
    print(f"{name}: {kern}  max|y - ref| / max|ref| = {err / scale:.3e}  {counters}")
    # fp32 element math vs fp64, relative to the operator scale (test_fast_mode_apply_keff_close; test_hex8's bound)
    assert err <= 2e-5 * scale
    with open(GOLDEN) as f:
        assert counters == json.load(f)[name]
    s.close()
