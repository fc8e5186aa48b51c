"""Shared by the element-monitor tests (include/cwf_hip.h "Element monitors"): the element strain of csrc/post.hip
restated in numpy float64 in its statement order (numpy fuses nothing, so every term has the device's bits), the
effective shear strain, the envelopes' update rule from their start values, and the soil column of the physical check."""
import functools
import math

import numpy as np

import absorbing_common as ac

INVALID = 0xFFFFFFFF
COLUMN_NZ = 48  # the physical check's column: 441 nodes, 1,152 tets


def corners(P):
    """-> (connectivity [E, K] int64, f32 gradients [E, K, 3]) of a packing, K = 4 (tet4) or 8 (hex8)."""
    conn = np.asarray(P.connectivity, np.uint32).reshape(-1, 8)
    K = 4 if P.element_count and conn[0, 4] == INVALID else 8
    grad = np.asarray(P.gradients, np.float32).reshape(-1, 24)[:, :3 * K].reshape(-1, K, 3)
    return conn[:, :K].astype(np.int64), grad


def element_strain64(P, u):
    """element_tensors' fp64 strain [E, 6] from the packing's f32 gradients and u (f32 or f64 [3N]): per corner, in
    ascending corner order from +0.0, e0 += gx ux; e1 += gy uy; e2 += gz uz; e3 += gy ux + gx uy; e4 += gz uy + gy uz;
    e5 += gz ux + gx uz (each shear pair summed before it is added)."""
    conn, grad = corners(P)
    u3 = np.asarray(u).astype(np.float64).reshape(-1, 3)
    e = np.zeros((conn.shape[0], 6), np.float64)
    for a in range(conn.shape[1]):
        ux, uy, uz = (u3[conn[:, a], k] for k in range(3))
        gx, gy, gz = (grad[:, a, k].astype(np.float64) for k in range(3))
        e[:, 0] += gx * ux
        e[:, 1] += gy * uy
        e[:, 2] += gz * uz
        e[:, 3] += gy * ux + gx * uy
        e[:, 4] += gz * uy + gy * uz
        e[:, 5] += gz * ux + gx * uz
    return e


def effective_shear(e):
    """The header's formula on fp64 strains [..., 6] -> fp64."""
    e = np.asarray(e, np.float64)
    d0, d1, d2 = e[..., 0] - e[..., 1], e[..., 1] - e[..., 2], e[..., 2] - e[..., 0]
    sd = d0 * d0 + d1 * d1 + d2 * d2
    sg = e[..., 3] * e[..., 3] + e[..., 4] * e[..., 4] + e[..., 5] * e[..., 5]
    return np.sqrt(sd * (2.0 / 3.0) + sg)


def two_sqrt_j2(e):
    """2 sqrt(J2) of the strain deviator from the principal strains (numpy.linalg.eigvalsh of the strain tensor, whose
    off-diagonal entries are half the engineering shears) -> fp64 [...]."""
    e = np.asarray(e, np.float64)
    T = np.empty(e.shape[:-1] + (3, 3))
    for k in range(3):
        T[..., k, k] = e[..., k]
    for (i, j), k in (((0, 1), 3), ((1, 2), 4), ((0, 2), 5)):
        T[..., i, j] = T[..., j, i] = 0.5 * e[..., k]
    p = np.linalg.eigvalsh(T)
    dev = p - p.mean(-1, keepdims=True)
    return 2.0 * np.sqrt(0.5 * (dev * dev).sum(-1))


class EnvelopeReference:
    """The maps from their start values, raised by the stated rule: np.where(x > p, x, p) for maxima,
    np.where(x < p, x, p) for minima."""

    def __init__(self, E):
        self.von_mises = np.zeros(E, np.float32)
        self.shear_strain = np.zeros(E, np.float32)
        self.stress_min = np.full((E, 6), np.inf, np.float32)
        self.stress_max = np.full((E, 6), -np.inf, np.float32)
        self.samples = 0

    def add(self, fields, shear32=None):
        """fields: f32 [E, 13] of cwf_hip_derived_fields for the sampled u; shear32: f32 [E] of the same u."""
        x = fields[:, 12]
        self.von_mises = np.where(x > self.von_mises, x, self.von_mises)
        s = fields[:, 6:12]
        self.stress_min = np.where(s < self.stress_min, s, self.stress_min)
        self.stress_max = np.where(s > self.stress_max, s, self.stress_max)
        if shear32 is not None:
            self.shear_strain = np.where(shear32 > self.shear_strain, shear32, self.shear_strain)
        self.samples += 1


def ulps_apart(a, b):
    """|a - b| in units of the last place, per entry, for finite non-negative f32 arrays."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


# ---- the soil column ------------------------------------------------------------------------------------------------
def column_clear_elements(case, nz, h=ac.COLUMN_H):
    """The elements of the nz-cell column in which the up-going pulse and the one reflected at the free surface do not
    overlap. The incident curve of absorbing_common is a Gaussian of sigma = 6 h cut off 4 sigma before its peak, so
    the pulse is taken as 4 sigma either side of its peak: it has passed a height z before its reflection arrives
    there when 2 (H - z) >= 8 sigma. An element counts when its highest node satisfies that. -> bool [E]"""
    conn, _ = corners(case.packing)
    ztop = case.mesh.coords[:, 2][conn].max(1)
    return ztop <= nz * h - 4.0 * 6.0 * h + 1e-9


@functools.lru_cache(maxsize=None)
def column_case(nz=COLUMN_NZ):
    return ac.column_case("S", nz=nz)


def column_run(dt, nz=COLUMN_NZ):
    """The incident S wave of tests/monitors_common.column_incident on the nz-cell column -> dict(ids, Cn, pattern,
    pts, steps, vals)."""
    from cwf import absorbing

    case = column_case(nz)
    ids, Cn = absorbing.dashpots(case.mesh, case.cfg, absorbing.faces_of_group(case.mesh, "BASE"))
    d = np.zeros(3)
    d[ac.column_axis("S")] = 1.0
    pattern = absorbing.incident_pattern(ids, Cn, d, case.packing.node_count)
    pts, steps = ac.incident_curve("S", dt, nz=nz)
    vals = np.array([p[1] for p in pts] + [pts[-1][1]])
    return dict(ids=ids, Cn=Cn, pattern=pattern, pts=pts, steps=steps, vals=vals)


def column_envelope_f64(dt, nz=COLUMN_NZ):
    """The all-float64 dense run of the scheme on the column and its own shear-strain envelope (every step sampled,
    kept in float64) -> (envelope [E], the run's dict)."""
    case = column_case(nz)
    ref = ac.dense_of(case)
    R = column_run(dt, nz)
    env = np.zeros(case.packing.element_count)
    for n, u, _ in ac.scheme_f64(ref["K"], ref["mass"], ref["fixed"], dt, R["steps"] + 1,
                                 lambda n: R["vals"][n] * R["pattern"], (R["ids"], R["Cn"])):
        if n:
            env = np.maximum(env, effective_shear(element_strain64(case.packing, u)))
    return env, R


def column_target(R):
    """max |v_inc| / V_s: the shear strain amplitude of a plane S wave of particle velocity v_inc."""
    return float(np.abs(R["vals"]).max()) / ac.wave_speed(ac.SOIL, "S")


def column_dt_estimate(nz=COLUMN_NZ):
    """0.9 x the critical step from the dense eigenvalue (the device's estimate is within a per cent of it)."""
    return 0.9 * 2.0 / math.sqrt(ac.dense_of(column_case(nz))["lam_max"])
