"""Helpers of the explicit stepper's soil plasticity (include/cwf_hip.h "Soil plasticity"): Drucker-Prager parameters
from Mohr-Coulomb ones, the geostatic stress of a horizontally layered deposit, and a check of that stress against the
cone. Host only; the arithmetic is the library's."""
from __future__ import annotations

import math

import numpy as np

from . import _lib

MATCHES = {"compression": 0, "extension": 1, "plane_strain": 2}


def _check(rc: int, what: str):
    if rc:
        msg, ctx = _lib.last_error(None)
        raise ValueError(f"{what}: {msg} {ctx}")


def from_mohr_coulomb(c: float, phi_deg: float, psi_deg: float = 0.0, match: str = "compression"):
    """-> (alpha, kappa, beta) of ExplicitStepper.set_soil_plasticity from a cohesion c (Pa), a friction angle and a
    dilation angle in degrees. match: the cone through the Mohr-Coulomb hexagon's compression corners, through its
    extension corners, or the plane-strain fit."""
    if match not in MATCHES:
        raise ValueError(f"match must be one of {sorted(MATCHES)}")
    out = np.zeros(3, np.float64)
    _check(_lib.load().cwf_soil_dp_from_mohr_coulomb(float(c), math.radians(phi_deg), math.radians(psi_deg),
                                                     MATCHES[match], _lib.ptr(out)), "from_mohr_coulomb")
    return float(out[0]), float(out[1]), float(out[2])


def centroids(packing) -> np.ndarray:
    """f64 [E,3]: the mean of each tet4 element's corner positions (the packing's float64 ones when it has them)."""
    X = packing.position64 if packing.position64 is not None else packing.position0
    X = np.asarray(X, np.float64).reshape(-1, 3)
    conn = np.asarray(packing.connectivity, np.uint32).reshape(-1, 8)[:, :4].astype(np.int64)
    return np.ascontiguousarray(X[conn].mean(axis=1))


def geostatic_stress(packing, materials, gravity: float = 9.81, k0=0.5, axis: int = 2, surface=None,
                     density=None) -> np.ndarray:
    """The stress at rest [E,6] of a horizontally layered deposit under its own weight: sigma_v = -g x the integral of
    the density from the free surface down to the element's centroid along `axis` (pointing up), sigma_h = K0 sigma_v,
    no shears. materials: records with a ``density`` (the scenario's), or pass ``density`` per material. k0: a scalar
    or one per material. surface: the free surface's elevation (None: the highest node). For horizontally layered
    deposits only: an elevation at which two materials meet side by side is refused (ValueError)."""
    M = len(materials)
    rho = np.asarray([m.density for m in materials] if density is None else density, np.float64)
    rho = np.ascontiguousarray(np.broadcast_to(rho, (M,)) if rho.ndim == 0 else rho.reshape(-1))
    k = np.asarray(k0, np.float64)
    k = np.ascontiguousarray(np.broadcast_to(k, (M,)) if k.ndim == 0 else k.reshape(-1))
    if rho.size != M or k.size != M:
        raise ValueError("one density and one K0 per material")
    cen = centroids(packing)
    E = cen.shape[0]
    mat = np.ascontiguousarray(packing.material_index, np.uint32)
    X = packing.position64 if packing.position64 is not None else packing.position0
    X = np.ascontiguousarray(np.asarray(X, np.float64).reshape(-1, 3))
    top = None if surface is None else np.array([surface], np.float64)
    out = np.zeros((E, 6), np.float64)
    _check(_lib.load().cwf_soil_geostatic_stress(E, _lib.ptr(cen), _lib.ptr(mat), M, _lib.ptr(rho), _lib.ptr(k),
                                                 float(gravity), int(axis), _lib.ptr(top), X.shape[0], _lib.ptr(X),
                                                 _lib.ptr(out)), "geostatic_stress")
    return out


def overstressed(initial_stress, alpha, kappa, material_index=None) -> np.ndarray:
    """The elements whose stress at rest already lies outside the cone, f = J + 3 alpha pm - kappa > 0: a K0 too far
    from 1 for the friction angle. alpha, kappa: scalars, or per material with material_index [E]."""
    s0 = np.asarray(initial_stress, np.float64).reshape(-1, 6)
    al, ka = np.asarray(alpha, np.float64), np.asarray(kappa, np.float64)
    if material_index is not None:
        idx = np.asarray(material_index, np.int64)
        al = al[idx] if al.ndim else al
        ka = ka[idx] if ka.ndim else ka
    pm = ((s0[:, 0] + s0[:, 1]) + s0[:, 2]) / 3.0
    s = s0[:, :3] - pm[:, None]
    j2 = 0.5 * ((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2]) + \
        ((s0[:, 3] * s0[:, 3] + s0[:, 4] * s0[:, 4]) + s0[:, 5] * s0[:, 5])
    f = (np.sqrt(np.maximum(j2, 0.0)) + (3.0 * al) * pm) - ka
    return np.flatnonzero(f > 0.0)
