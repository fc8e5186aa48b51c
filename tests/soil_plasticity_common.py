"""Shared by the soil plasticity tests (include/cwf_hip.h "Soil plasticity"): the header's return map restated in
numpy float64 in its statement order (numpy fuses nothing, so every term has the device's bits), vectorised over
elements, and plasticity_common's Restatement with that map in place of the J2 one. Corner forces and the node fold
are that Restatement's."""
import numpy as np

import plasticity_common as pc


def dp_update(D, par, sig0, V, e, ep, abar, wp):
    """The header's block on n elements at once: D [n,6,6], par [n,4] = alpha, kappa, beta, H, sig0 [n,6] or None, V
    [n], e, ep [n,6], abar, wp [n] -> (branch int [n]: 0 elastic, 1 cone, 2 apex; ep, abar, wp, sp), new arrays."""
    alpha, kappa, beta, H = par[:, 0], par[:, 1], par[:, 2], par[:, 3]
    ee = e - ep
    st = pc.iso_row_fold(D, ee)
    if sig0 is not None:
        st = sig0 + st
    with np.errstate(all="ignore"):
        pm = ((st[:, 0] + st[:, 1]) + st[:, 2]) / 3.0
        s = st.copy()
        for r in range(3):
            s[:, r] = st[:, r] - pm
        j2 = 0.5 * ((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2]) + \
            ((s[:, 3] * s[:, 3] + s[:, 4] * s[:, 4]) + s[:, 5] * s[:, 5])
        J = np.sqrt(np.where(j2 < 0.0, 0.0, j2))
        kc = kappa + H * abar
        f = (J + (3.0 * alpha) * pm) - kc
        yielded = f > 0.0
        mu = D[:, 3, 3]
        Kb = D[:, 0, 1] + (2.0 / 3.0) * mu
        dl = f / ((mu + ((9.0 * Kb) * alpha) * beta) + H)
        Jn = J - mu * dl
        cone = yielded & ((Jn >= 0.0) | ~(alpha > 0.0))
        apex = yielded & ~cone
        # the cone
        half = (0.5 * dl) / J
        bdl = beta * dl
        epc = ep.copy()
        for r in range(3):
            epc[:, r] = ep[:, r] + (half * s[:, r] + bdl)
        for r in range(3, 6):
            epc[:, r] = ep[:, r] + (2.0 * half) * s[:, r]
        abarc = abar + dl
        wpc = wp + V * (dl * (Jn + (3.0 * beta) * (pm - ((3.0 * Kb) * beta) * dl)))
        # the apex
        pa = kc / (3.0 * alpha)
        dv = (pm - pa) / Kb
        third = dv / 3.0
        epa = ep.copy()
        for r in range(3):
            epa[:, r] = ep[:, r] + (s[:, r] / (2.0 * mu) + third)
        for r in range(3, 6):
            epa[:, r] = ep[:, r] + s[:, r] / mu
        abara = abar + J / mu
        wpa = wp + V * (pa * dv)
    branch = np.where(cone, 1, np.where(apex, 2, 0))
    ep2 = np.where(cone[:, None], epc, np.where(apex[:, None], epa, ep))
    abar2 = np.where(cone, abarc, np.where(apex, abara, abar))
    wp2 = np.where(cone, wpc, np.where(apex, wpa, wp))
    return branch, ep2, abar2, wp2, pc.iso_row_fold(D, ep2)


class SoilRestatement(pc.Restatement):
    """plasticity_common.Restatement with the Drucker-Prager map: per-material alpha, kappa, beta, H (scalars apply to
    every material; kappa = inf: elastic) and an optional stress at rest sig0 [E,6] in the caller's element order.
    branch: the last step's outcome per slot; seen: the outcomes met so far per slot, as a bit set (1 cone, 2 apex)."""

    def __init__(self, P, materials, alpha, kappa, beta=0.0, H=0.0, sig0=None):
        M = len(materials)
        par = np.stack([np.broadcast_to(np.asarray(x, np.float64), (M,)) for x in (alpha, kappa, beta, H)], axis=1)
        # the parent's slot choice is "sy finite and > 0": any finite kappa counts, so hand it 1.0 there
        super().__init__(P, materials, np.where(np.isfinite(par[:, 1]), 1.0, np.inf), 0.0)
        mat = np.asarray(P.material_index, np.int64)
        self.par = par[mat[self.elem]]
        self.sig0 = None if sig0 is None else np.asarray(sig0, np.float64).reshape(-1, 6)[self.elem]
        self.branch = np.zeros(self.elem.size, np.int64)
        self.seen = np.zeros(self.elem.size, np.int64)

    def step(self, u):
        """The element pass and the node fold at u = u_n (f32 [3N]) -> p f32 [3N]; the state advances."""
        self.branch, self.ep, self.abar, self.wp, sp = dp_update(self.D, self.par, self.sig0, self.V, self.strain(u),
                                                                 self.ep, self.abar, self.wp)
        self.seen |= self.branch
        return self.correction(sp)
