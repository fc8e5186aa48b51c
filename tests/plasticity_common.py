"""Shared by the plasticity tests (include/cwf_hip.h "Plasticity"): the header's element update, corner forces and node
fold restated in numpy float64 in their statement order (numpy fuses nothing, so every term has the device's bits),
vectorised over elements. A Restatement enters the stepper's scheme (explicit_common.scheme_steps) as its correction
force, p_at = lambda n, u: R.step(u)."""
import numpy as np

import element_monitors_common as ec
import explicit_common as xc
from cwf import pack

FLT_MAX = 3.4028234663852886e38
KINDS = {k: xc.KINDS[k] for k in ("parity", "lattice", "groups")}  # plasticity is tet4 only
VARIANTS = {k: xc.VARIANTS[k] for k in ("undamped", "damped")}
HARDENING = 3.0e9  # the J2 cases' hardening modulus: a tenth of the block's Young's modulus


def von_mises(s):
    """post.hip's von Mises of Voigt stresses [..., 6], float64."""
    dxy, dyz, dzx = s[..., 0] - s[..., 1], s[..., 1] - s[..., 2], s[..., 2] - s[..., 0]
    energy = 0.5 * (dxy * dxy + dyz * dyz + dzx * dzx) + 3.0 * (s[..., 3] * s[..., 3] + s[..., 4] * s[..., 4] +
                                                               s[..., 5] * s[..., 5])
    return np.sqrt(np.where(energy < 0.0, 0.0, energy))


def iso_row_fold(D, x):
    """D x by element_tensors' ISO row fold. D [n, 6, 6], x [n, 6] -> [n, 6]."""
    out = np.empty_like(x)
    for r in range(3):
        acc = np.zeros(x.shape[0])
        for k in range(3):
            acc = acc + D[:, r, k] * x[:, k]
        out[:, r] = acc
    for r in range(3, 6):
        out[:, r] = 0.0 + D[:, r, r] * x[:, r]
    return out


def j2_update(D, sy, H, V, e, ep, abar, wp):
    """The header's block on n elements at once: D [n,6,6], sy, H, V [n], e, ep [n,6], abar, wp [n] -> (yielded
    bool [n], ep, abar, wp, sp), new arrays."""
    ee = e - ep
    st = iso_row_fold(D, ee)
    q = von_mises(st)
    Y = sy + H * abar
    with np.errstate(invalid="ignore", divide="ignore"):
        y = q > Y
        mu = D[:, 3, 3]
        dg = (q - Y) / (3.0 * mu + H)
        pm = ((st[:, 0] + st[:, 1]) + st[:, 2]) / 3.0
        fac = (1.5 * dg) / q
        epn = ep.copy()
        for r in range(3):
            epn[:, r] = ep[:, r] + fac * (st[:, r] - pm)
        for r in range(3, 6):
            epn[:, r] = ep[:, r] + (2.0 * fac) * st[:, r]
        abarn = abar + dg
        wpn = wp + V * ((sy + H * abarn) * dg)
    ep2 = np.where(y[:, None], epn, ep)
    abar2 = np.where(y, abarn, abar)
    wp2 = np.where(y, wpn, wp)
    return y, ep2, abar2, wp2, iso_row_fold(D, ep2)


def safe_cast(v):
    """pack.cpp's safe_cast_double_to_float (finite values clamp to +-FLT_MAX)."""
    return pack._safe_f32(v)


class Restatement:
    """The plastic pass of a packing in numpy: slots (plastic elements, ascending), their state, and the correction
    force p [3N] (caller's node order) of a displacement."""

    def __init__(self, P, materials, sy, H):
        self.P = P
        conn, grad = ec.corners(P)
        assert conn.shape[1] == 4
        mat = np.asarray(P.material_index, np.int64)
        sy = np.broadcast_to(np.asarray(sy, np.float64), (len(materials),))
        H = np.broadcast_to(np.asarray(H, np.float64), (len(materials),))
        plastic = (sy > 0.0) & np.isfinite(sy)
        self.elem = np.flatnonzero(plastic[mat])
        self.conn, self.grad = conn[self.elem], grad[self.elem].astype(np.float64)
        Dall = np.stack([np.asarray(m.stiffness, np.float64).reshape(6, 6) for m in materials])
        self.D = Dall[mat[self.elem]]
        self.sy, self.H = sy[mat[self.elem]], H[mat[self.elem]]
        self.V = np.asarray(P.volume, np.float32)[self.elem].astype(np.float64)
        n = self.elem.size
        self.ep, self.abar, self.wp = np.zeros((n, 6)), np.zeros(n), np.zeros(n)
        self.E, self.N = P.element_count, P.node_count
        self.affected = np.unique(self.conn)

    def strain(self, u):
        return ec.element_strain64(self.P, u)[self.elem]

    def step(self, u):
        """The element pass and the node fold at u = u_n (f32 [3N]) -> p f32 [3N]; the state advances."""
        _, self.ep, self.abar, self.wp, sp = j2_update(self.D, self.sy, self.H, self.V, self.strain(u), self.ep,
                                                       self.abar, self.wp)
        return self.correction(sp)

    def correction(self, sp):
        """The corner forces of the slots' plastic stresses sp [n,6] (kept as self.corner) and their node fold -> p."""
        p = np.zeros((self.N, 3), np.float64)
        V = self.V
        c = np.empty((self.elem.size, 4, 3), np.float32)
        for a in range(4):
            gx, gy, gz = self.grad[:, a, 0], self.grad[:, a, 1], self.grad[:, a, 2]
            c[:, a, 0] = safe_cast(V * ((gx * sp[:, 0] + gy * sp[:, 3]) + gz * sp[:, 5]))
            c[:, a, 1] = safe_cast(V * ((gy * sp[:, 1] + gx * sp[:, 3]) + gz * sp[:, 4]))
            c[:, a, 2] = safe_cast(V * ((gz * sp[:, 2] + gy * sp[:, 4]) + gx * sp[:, 5]))
        self.corner = c
        # a node's incidences in ascending element order from +0.0: one element at a time (a tet's corners are
        # distinct nodes, so one vectorised add per element row never meets a node twice)
        for q in range(self.elem.size):
            p[self.conn[q]] = p[self.conn[q]] + c[q].astype(np.float64)
        return safe_cast(p.reshape(-1))

    def full(self):
        """(ep [E,6], abar [E], wp [E]) in the caller's element order, zeros at elastic elements."""
        ep, abar, wp = np.zeros((self.E, 6)), np.zeros(self.E), np.zeros(self.E)
        ep[self.elem], abar[self.elem], wp[self.elem] = self.ep, self.abar, self.wp
        return ep, abar, wp


def plastic_scheme(P, apply, R, force_at, alpha, beta, dt, u0, v0, first_step, steps, dash=None):
    """explicit_common.host_scheme on the packing P with the plastic pass R (a Restatement, or None: the elastic
    scheme) -> (u, v, p of the last step)."""
    return xc.host_scheme(apply, np.repeat(P.lumped_mass, 3), xc.constrained(P), P.bc_value, force_at, alpha, beta, dt,
                          u0, v0, first_step, steps, dash, p_at=None if R is None else (lambda n, u: R.step(u)),
                          with_p=True)


def bits64(a):
    return np.ascontiguousarray(a, np.float64).reshape(-1).view(np.uint64)


def assert_state(st, state, what):
    """ep, abar, wp of the stepper against the restatement's `state` (Restatement.full()), bit for bit."""
    ps = st.plasticity()
    for name, a, b in (("ep", ps.plastic_strain, state[0]), ("abar", ps.equivalent_plastic_strain, state[1]),
                       ("wp", ps.plastic_work, state[2])):
        bad = np.flatnonzero(bits64(a) != bits64(b))
        assert bad.size == 0, (what, name, bad[:5], np.asarray(a).reshape(-1)[bad[:5]], b.reshape(-1)[bad[:5]])


def plastic_scenario(tmp_path, yield_stress):
    """explicit_common.block_scenario (216 tets held at x = 0, a traction on the far face) with a yield stress on its
    material and a frame in every VTU. The explicit driver holds the load of t = 0 (the traction's curve starts at 0),
    so the block moves under its own weight: stresses of some kPa near the held face."""
    return xc.block_scenario(tmp_path, name="plastic.yaml", replacements=(
        ("vtu_stride: 10", "vtu_stride: 1"),
        ("    rho: 2500.0\n", f"    rho: 2500.0\n    yield_stress: {yield_stress!r}\n    hardening_modulus: 3.0e9\n")))
