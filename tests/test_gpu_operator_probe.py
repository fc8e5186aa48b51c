"""FAST apply_keff entry by entry against the fp64 reference of tests/operator_probe_common.py, on every layout
cwf_hip_system_create can build (test_gpu_create_paths.CASES) and the lattice's variants.

Per case (u = 2^-24, R_I the largest diagonal entry of A = sum_e |Ke| over node I's rows):

  1. structural zeros: +-0.0 on every row of a node that shares no element with the probe node;
  2. the Dirichlet rule: constrained rows return x bit for bit, a probe on a constrained DOF changes no free row;
  3. |K_fast[i, j] - K_ref[i, j]| <= c_e u R_I;
  4. rigid translations on a handle with no Dirichlet node and s_M = 0: exactly 0 on the lattice (difference form),
     within item 5's bound elsewhere;
  5. one random vector: |y - K_ref x|_i <= c_v u (A |x|)_i; and one smooth vector under the same bound, the static
     load over the row scale R_I (what the first PCG iterate looks like): a row's rounding errors average out over
     random signs and add up over equal ones, so the random vector alone understates c_v (fan groups: 5.3 against 66).

Meshes of at most 2,048 DOF are probed with every unit vector; the larger lattices with the 81 coloured probes.

Caps. The lattice families (plain and layered, Kuhn and hex8) carry c_e = 16, c_v = 128 from rounding counts: a unit
probe makes every product exact, which leaves the table's rounding, the diagonal block's sum of at most 14 terms and the
s_K and mass roundings per entry, and about 90 fp32 operations per row of a full vector (the fp32 emulation of the host
tables gives 3.4 and 3.2, tests/test_operator_probe_host.py). The families that form their geometry in fp32 carry
4 x the worst ratio measured on the MI355X, rounded up to a power of two: profiles/operator_probe_accuracy.txt holds
the measured ratios and the caps per family. Every c_e is 32 or less, a tenth of the 335 u of the largest row that
2e-5 max |ref| allows. One finding: the fan groups' c_v comes out at 512 (66.2 u of the row's own A|x| on the smooth
vector with 256-node tiles, 29.2 with 128-node ones; the per-tet tiles of the same mesh stay at 12.0). Its unit is
the row's own scale, not the largest row of the vector that the 2e-5 contract is written in, so the two numbers do
not compare directly; but it is above 335 by the rounding rule and several times what the other fp32-geometry
families need, and is recorded as a finding, not tuned away. Every worst ratio is printed."""
import dataclasses
import functools

import numpy as np
import pytest

import materials_common as MC
import operator_probe_common as OP
from cwf import _lib, pcg, scenarios
from test_gpu_create_paths import CASES as CREATE_CASES, KNOBS as CREATE_KNOBS
from test_gpu_lattice import permuted_block
from test_gpu_lattice_layered import SHAPES as LAYERED_SHAPES
from test_hex8 import hex_case

pytestmark = pytest.mark.gpu

# family -> (c_e, c_v); the lattice's derived, the others 4 x the worst ratio measured, rounded up to a power of two
# (profiles/operator_probe_accuracy.txt: entry 7.79 / 5.37 / 4.76 / 5.17, vector 66.2 / 12.0 / 7.84 / 6.11)
CAPS = {
    "lattice": (16.0, 128.0),
    "fan-groups": (32.0, 512.0),
    "tiles-pipe": (32.0, 64.0),
    "records": (32.0, 32.0),
    "hex-tiles": (32.0, 32.0),
}
FAMILY_OF = (("k_keff_groups_pipe", "fan-groups"), ("k_keff_tiles_pipe", "tiles-pipe"), ("k_keff_tiles", "records"),
             ("k_keff_hex_tiles", "hex-tiles"), ("k_keff_lattice", "lattice"), ("k_pcg_lattice", "lattice"),
             ("k_pcg_resident", "lattice"))
LATTICE_KERNELS = ("k_pcg_resident", "k_pcg_lattice", "k_keff_lattice")
KNOBS = sorted(set(CREATE_KNOBS) | {"CWF_GROUP_NT", "CWF_FUSED", "CWF_LAT_L", "CWF_LAT_ZR", "CWF_RESIDENT",
                                    "CWF_FUSED_MAXWG", "CWF_HEX_NT"})
FULL_PROBE_DOFS = 2048
STRATA = [MC.ISO, MC.ROT, MC.ORTHO]


def family_of(kern):
    for prefix, fam in FAMILY_OF:
        if kern.startswith(prefix):
            return fam
    raise AssertionError(kern)


@dataclasses.dataclass(frozen=True)
class Spec:
    mesh: str
    variant: str = ""
    knobs: tuple = ()
    kernels: tuple = ()
    materials: str = ""


MESHES = {
    "block": lambda: scenarios.block_case(8, 3, 4, h=0.1),
    "hex": lambda: hex_case(6, 4, 3),
    "jitter": lambda: scenarios.block_case(7, 6, 5, h=0.1, jitter=True),
    "layered-5x4x4-tet4": lambda: scenarios.layered_case(*LAYERED_SHAPES["5x4x4"][0], LAYERED_SHAPES["5x4x4"][1]),
    "layered-5x4x4-hex8": lambda: scenarios.layered_case(*LAYERED_SHAPES["5x4x4"][0], LAYERED_SHAPES["5x4x4"][1],
                                                         element="hex8"),
    "rollers-7x5x4": lambda: scenarios.roller_case(7, 5, 4),
    "rayleigh-6x4x3": lambda: scenarios.block_case(6, 4, 3, h=0.1, xi=0.05, w=(10.0, 100.0)),
    "permuted-9x7x6": lambda: permuted_block(9, 7, 6),
    "block-40x17x9": lambda: scenarios.block_case(40, 17, 9, h=0.1),
    "layered-40x19x9": lambda: scenarios.layered_case(*LAYERED_SHAPES["40x19x9"][0], LAYERED_SHAPES["40x19x9"][1]),
}
SPECS = {f"create/{name}": Spec(c[0], c[1], tuple(sorted(c[2].items())), c[3]) for name, c in CREATE_CASES.items()}
SPECS.update({
    "fan-groups-128": Spec("jitter", knobs=(("CWF_GROUP_NT", "128"),), kernels=("k_keff_groups_pipe",)),
    "layered-5x4x4-tet4": Spec("layered-5x4x4-tet4", kernels=("k_keff_lattice_layered",)),
    "layered-5x4x4-hex8": Spec("layered-5x4x4-hex8", kernels=("k_keff_lattice_layered",)),
    "rollers-7x5x4": Spec("rollers-7x5x4", kernels=LATTICE_KERNELS),
    "rayleigh-6x4x3": Spec("rayleigh-6x4x3", kernels=LATTICE_KERNELS),
    "permuted-9x7x6": Spec("permuted-9x7x6", kernels=LATTICE_KERNELS),
    "fan-groups/rot": Spec("jitter", kernels=("k_keff_groups_pipe",), materials="rot"),
    "fan-groups/mixed-thirds": Spec("jitter", kernels=("k_keff_groups_pipe",), materials="mixed-thirds"),
    "lattice-tet4/rot": Spec("block", kernels=LATTICE_KERNELS, materials="rot"),
    "layered-5x4x4-tet4/strata": Spec("layered-5x4x4-tet4", kernels=("k_keff_lattice_layered",), materials="strata"),
    "40x17x9-two-kernel-L3": Spec("block-40x17x9", knobs=(("CWF_FUSED", "0"), ("CWF_LAT_L", "3")),
                                  kernels=("k_keff_lattice<",)),
    "40x17x9-two-kernel": Spec("block-40x17x9", knobs=(("CWF_FUSED", "0"),), kernels=("k_keff_lattice<",)),
    "layered-40x19x9-L3": Spec("layered-40x19x9", knobs=(("CWF_LAT_L", "3"),), kernels=("k_keff_lattice_layered",)),
})


@functools.lru_cache(maxsize=None)
def mesh_case(name):
    return MESHES[name]()


@functools.lru_cache(maxsize=None)
def material_case(mesh, variant, materials):
    """The case with the spec's materials: (materials, material index per element)."""
    case = mesh_case(mesh)
    P = case.packing
    if variant == "materials17":
        return case.materials * 17, (np.arange(P.element_count) % 17).astype(np.uint32)
    if materials == "rot":
        return [MC.props(MC.ROT)], P.material_index
    if materials == "mixed-thirds":
        return [MC.props(D) for D in (MC.ISO, MC.ORTHO, MC.ROT)], MC.thirds(case)
    if materials == "strata":
        return [MC.props(D) for D in STRATA], P.material_index
    return case.materials, P.material_index


def make_system(spec, scalars, bc_mask=None):
    case = mesh_case(spec.mesh)
    P = case.packing
    materials, mat = material_case(spec.mesh, spec.variant, spec.materials)
    coords = P.position64 if getattr(P, "position64", None) is not None else P.position0
    return pcg.MatrixFreeSystem(P.connectivity, P.gradients, P.volume, mat, materials, P.lumped_mass,
                                P.bc_mask if bc_mask is None else bc_mask, P.node_count, P.element_count, P.dof_count,
                                scalars[0], scalars[1], P.reduction_block, P.reduction_partials,
                                (P.offsets, P.element_indices, P.local_indices), _lib.MODE_FAST, 0,
                                None if spec.variant == "no_coords" else coords,
                                keep_node_order=spec.variant == "keep_order")


@functools.lru_cache(maxsize=None)
def reference(mesh, variant, materials, free_body=False):
    """The fp64 reference of a spec's operator (free_body: no Dirichlet node, s_M = 0), built once and shared."""
    case = mesh_case(mesh)
    mats, mat = material_case(mesh, variant, materials)
    sK, sM = case.scalars()
    if free_body:
        return OP.reference_of(case, mats, (sK, 0.0), mat, np.zeros(case.packing.node_count, np.uint32))
    return OP.reference_of(case, mats, (sK, sM), mat)


def kernel_name(s):
    return (_lib.load().cwf_hip_system_keff_kernel(s.handle()) or b"").decode()


def apply_block(s, V):
    """K_fast V, one apply_keff per column."""
    V = np.asarray(V, np.float32).reshape(s.dof_count, -1)
    Y = np.zeros_like(V)
    y = np.zeros(s.dof_count, np.float32)
    for c in range(V.shape[1]):
        pcg.apply_keff(s, np.ascontiguousarray(V[:, c]), y).value()
        Y[:, c] = y
    return Y


@pytest.mark.parametrize("name", sorted(SPECS))
def test_apply_keff_entry_by_entry(name, monkeypatch):
    spec = SPECS[name]
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in spec.knobs:
        monkeypatch.setenv(k, v)
    case = mesh_case(spec.mesh)
    sK, sM = case.scalars()
    ref = reference(spec.mesh, spec.variant, spec.materials)
    s = make_system(spec, (sK, sM))
    kern = kernel_name(s)
    assert kern.startswith(spec.kernels), kern
    if spec.kernels == ("k_keff_tiles",):
        assert not kern.startswith("k_keff_tiles_pipe"), kern
    family = family_of(kern)
    c_e, c_v = CAPS[family]
    if ref.D <= FULL_PROBE_DOFS:
        V, nodes, comp = OP.unit_probes(ref.N)
    else:
        assert family == "lattice"
        V, nodes, comp = OP.lattice_probes(case.mesh.coords)
    rep = OP.probe_report(ref, V, nodes, comp, apply_block(s, V))
    x = np.random.Generator(np.random.PCG64(3)).uniform(-1, 1, ref.D).astype(np.float32)
    ratio, off_scale = OP.vector_ratio(ref, x, apply_block(s, x)[:, 0])
    # and a smooth one, the static load over the row scale (a Jacobi-preconditioned load, what a PCG iterate looks
    # like): the rounding errors of a row, which average out over random signs, add up over equal ones
    xs = (case.static_rhs().astype(np.float64) / ref.row_scale).astype(np.float32)
    smooth, off_smooth = OP.vector_ratio(ref, xs, apply_block(s, xs)[:, 0])
    s.close()
    # rigid translations of the free body
    body = reference(spec.mesh, spec.variant, spec.materials, True)
    sb = make_system(spec, (sK, 0.0), np.zeros(case.packing.node_count, np.uint32))
    assert family_of(kernel_name(sb)) == family, kernel_name(sb)
    T = np.tile(np.eye(3, dtype=np.float32) * np.float32(0.7), (ref.N, 1))
    YT = apply_block(sb, T)
    sb.close()
    t_nonzero = int(np.count_nonzero(YT))
    t_ratio = float(np.max(np.abs(YT.astype(np.float64) - body.apply(T)) / (OP.U * body.apply_abs(T))))
    print(f"{name}: {kern} [{family}] {V.shape[1]} probes: entry {rep['entry']:.2f} u R_I (cap {c_e:g}), random vector "
          f"{ratio:.2f} u A|x| (cap {c_v:g}), smooth vector {smooth:.2f} u A|x|, translations {t_ratio:.2f} u A|x| "
          f"({t_nonzero} non-zero), structural "
          f"{rep['structural']}, passthrough {rep['passthrough']}, leaked {rep['leaked']}")
    assert rep["structural"] == 0
    assert rep["passthrough"] == 0 and rep["leaked"] == 0
    assert rep["entry"] <= c_e
    if family == "lattice":
        assert t_nonzero == 0
    else:
        assert t_ratio <= c_v
    assert ratio <= c_v and off_scale == 0
    assert smooth <= c_v and off_smooth == 0
