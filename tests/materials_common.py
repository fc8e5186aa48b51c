"""Anisotropic test materials and per-element material assignments, shared by tests/test_materials_host.py and
tests/test_gpu_materials.py (CPU only, numpy).

Voigt order is the project's: xx, yy, zz, xy, yz, xz with engineering shear (physics.make_stiffness_matrix), so a
Voigt entry is the tensor entry itself, D[I, J] = C[i, j, k, l] with (i, j) = PAIR[I], (k, l) = PAIR[J].

  ISO    the project's steel: three distinct numbers and 24 structural zeros.
  ORTHO  orthotropic along the axes: the isotropic zero pattern (twelve non-zeros) with nine distinct values, so a
         handle of it runs the ISO = true kernels and every slot of their 12-entry table holds its own number.
  ROT    ORTHO rotated by Rz(30 deg) Rx(20 deg): all 36 entries non-zero, so a handle of it runs ISO = false.
"""
import dataclasses

import numpy as np

from cwf.physics import Material, make_properties, make_stiffness_matrix

STEEL = Material("steel", 30.0e9, 0.2, 2500.0)
PAIR = ((0, 0), (1, 1), (2, 2), (0, 1), (1, 2), (0, 2))


def orthotropic(E, nu12, nu23, nu13, G_xy, G_yz, G_xz):
    """The inverse of the compliance S with S01 = -nu12 / E1, S12 = -nu23 / E2, S02 = -nu13 / E1."""
    S = np.zeros((6, 6))
    S[0, 0], S[1, 1], S[2, 2] = 1.0 / E[0], 1.0 / E[1], 1.0 / E[2]
    S[0, 1] = S[1, 0] = -nu12 / E[0]
    S[1, 2] = S[2, 1] = -nu23 / E[1]
    S[0, 2] = S[2, 0] = -nu13 / E[0]
    S[3, 3], S[4, 4], S[5, 5] = 1.0 / G_xy, 1.0 / G_yz, 1.0 / G_xz
    return np.linalg.inv(S)


def tensor_of(D):
    C = np.zeros((3, 3, 3, 3))
    for I, (i, j) in enumerate(PAIR):
        for J, (k, l) in enumerate(PAIR):
            C[i, j, k, l] = C[j, i, k, l] = C[i, j, l, k] = C[j, i, l, k] = D[I, J]
    return C


def voigt_of(C):
    return np.array([[C[i, j, k, l] for (k, l) in PAIR] for (i, j) in PAIR])


def rotate(D, R):
    """The stiffness of the material turned by R: C'_abcd = R_ai R_bj R_ck R_dl C_ijkl."""
    return voigt_of(np.einsum("ai,bj,ck,dl,ijkl", R, R, R, R, tensor_of(D)))


def _rz(deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def _rx(deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    return np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])


R_ROT = _rz(30.0) @ _rx(20.0)
ISO = np.array(make_stiffness_matrix(30.0e9, 0.2)).reshape(6, 6)
ORTHO = orthotropic((30.0e9, 12.0e9, 6.0e9), 0.2, 0.25, 0.3, 5.0e9, 3.0e9, 4.0e9)
ROT = rotate(ORTHO, R_ROT)
for _D in (ISO, ORTHO, ROT):
    _D.setflags(write=False)


def many(n):
    """n distinct materials ROT (1 + 0.05 k); for n = 18 two of them lie past the 16-row LDS tables."""
    return [ROT * (1.0 + 0.05 * k) for k in range(n)]


def props(D):
    """An ElasticProperties record carrying D, for every entry point that takes `materials`."""
    return dataclasses.replace(make_properties(STEEL), stiffness=list(np.asarray(D, np.float64).reshape(-1)))


def stiffness_array(materials):
    """The concatenated 36-vectors the oracle entry points take."""
    return np.concatenate([np.asarray(m.stiffness if hasattr(m, "stiffness") else m, np.float64).reshape(-1)
                           for m in materials])


def centroids(case):
    return case.mesh.coords[np.asarray(case.mesh.tets, np.int64)].mean(1)


def thirds(case):
    """material = floor(3 x / L) of the element centroid: three large regions, fans cut at two interfaces."""
    x = centroids(case)[:, 0]
    lo, hi = case.mesh.coords[:, 0].min(), case.mesh.coords[:, 0].max()
    return np.clip(np.floor(3.0 * (x - lo) / (hi - lo)), 0, 2).astype(np.uint32)


def scattered(case, M):
    """material = e % M: almost every fan is cut to one or two elements."""
    return (np.arange(case.packing.element_count) % M).astype(np.uint32)


class MaterialCase:
    """A scenarios.Case seen with a material list of the test's own (Case.materials is derived from the config) and,
    optionally, another material per element. Everything else is the case's."""

    def __init__(self, case, stiffnesses, material_index=None, name=None):
        self.case = case
        self.name = name or case.name
        self.materials = [props(D) for D in stiffnesses]
        self.packing = case.packing if material_index is None else with_materials(case, material_index)

    def __getattr__(self, attr):  # mesh, cfg, rayleigh, scalars, static_rhs
        return getattr(self.case, attr)

    @property
    def stiffness(self):
        return stiffness_array(self.materials)


def with_materials(case, material_index):
    """The case's packing with another material per element (the density, so the mass, is the steel's throughout)."""
    return dataclasses.replace(case.packing, material_index=np.ascontiguousarray(material_index, np.uint32))
