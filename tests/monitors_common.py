"""Shared by the monitor tests: the monitors' per-DOF terms of include/cwf_hip.h ("Monitors") in numpy float64 in the
stated association (numpy fuses nothing, so every term has the device's bits; only the order of the sums differs), fed
with what explicit_common.scheme_steps yields of one update pass."""
import numpy as np

import absorbing_common as ac

EPS = 2.0 ** -53


def norm3(a):
    """f32(sqrt((a0 a0 + a1 a1) + a2 a2)) per node of a float64 [3N] vector."""
    a = a.reshape(-1, 3)
    return np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]).astype(np.float32)


def peak_candidates(v, un, vn, dt):
    """The three values one update offers the peak maps: |u_(n+1)|, |v_(n+1/2)|, |(vn - v) / dt| per node, f32."""
    un64, vn64, v64 = un.astype(np.float64), vn.astype(np.float64), v.astype(np.float64)
    return norm3(un64), norm3(vn64), norm3((vn64 - v64) / dt)


def raise_peaks(peaks, cand):
    """max(p, x) = x > p ? x : p on each of the three maps, in place."""
    for p, x in zip(peaks, cand):
        up = x > p
        p[up] = x[up]


def energy_terms(mass, fixed, alpha, dt, v, y, f, un, vn, dashC=None, with_dissipation=True):
    """The ledger's per-DOF terms of one update -> float64 [4, 3N] (kin, pot, work, diss), 0 at constrained DOFs.
    mass: per DOF; dashC: (node ids, C [n,3,3]) as given to set_dashpots, or None. Works on float32 or float64 state."""
    m = mass.astype(np.float64)
    v64, vn64, un64 = v.astype(np.float64), vn.astype(np.float64), un.astype(np.float64)
    vb = 0.5 * (vn64 + v64)
    kin = 0.5 * (m * (vn64 * vn64))
    pot = 0.5 * (un64 * y.astype(np.float64))
    work = dt * (vb * f.astype(np.float64))
    diss = dt * (alpha * (m * (vb * vb)))
    if dashC is not None and len(dashC[0]):
        ids, Cn = dashC
        b = vb.reshape(-1, 3)[ids]
        extra = np.empty_like(b)
        for k in range(3):
            extra[:, k] = dt * (b[:, k] * ((Cn[:, k, 0] * b[:, 0] + Cn[:, k, 1] * b[:, 1]) + Cn[:, k, 2] * b[:, 2]))
        d3 = diss.reshape(-1, 3).copy()
        d3[ids] = d3[ids] + extra
        diss = d3.reshape(-1)
    if not with_dissipation:
        diss = np.zeros_like(diss)
    t = np.stack([kin, pot, work, diss])
    t[:, fixed] = 0.0
    return t


class LedgerReference:
    """Accumulates the restatement's ledger: per sampled step the four columns and, per column, the worst-case
    summation bound (terms - 1) 2^-53 sum |term| -- for the cumulative columns over every step so far."""

    def __init__(self):
        self.cum = np.zeros(2)
        self.cum_abs = np.zeros(2)
        self.cum_terms = 0
        self.rows, self.bounds, self.steps = [], [], []

    def add(self, step_count, t, sample=True):
        """t: energy_terms of the update that made the step count `step_count`."""
        self.cum += np.array([t[2].sum(), t[3].sum()])
        self.cum_abs += np.array([np.abs(t[2]).sum(), np.abs(t[3]).sum()])
        self.cum_terms += t.shape[1]
        if sample:
            n = t.shape[1]
            self.rows.append([t[0].sum(), t[1].sum(), self.cum[0], self.cum[1]])
            self.bounds.append([(n - 1) * EPS * np.abs(t[0]).sum(), (n - 1) * EPS * np.abs(t[1]).sum(),
                                (self.cum_terms - 1) * EPS * self.cum_abs[0],
                                (self.cum_terms - 1) * EPS * self.cum_abs[1]])
            self.steps.append(step_count)

    def arrays(self):
        return np.array(self.steps, np.uint64), np.array(self.rows).reshape(-1, 4), np.array(self.bounds).reshape(-1, 4)


def balance(rows):
    """kinetic + potential - work_cum + dissipated_cum of ledger rows [n, 4]."""
    rows = np.asarray(rows, np.float64)
    return (rows[:, 0] + rows[:, 1]) - rows[:, 2] + rows[:, 3]


def balance_drift(rows):
    """max |balance_i - balance_0| / max (kinetic + potential)."""
    b = balance(rows)
    total = np.asarray(rows)[:, 0] + np.asarray(rows)[:, 1]
    return float(np.abs(b - b[0]).max() / np.abs(total).max())


def column_incident(wave, dt):
    """The incident-wave run of the soil column (tests/test_gpu_absorbing.py, 4): the base's dashpots, the load
    pattern 2 C d and the Gaussian curve sampled per step -> dict(ids, Cn, pattern, pts, steps, vals)."""
    from cwf import absorbing

    case = ac.column_case(wave)
    ids, Cn = ac.column_dashpots(wave)
    d = np.zeros(3)
    d[ac.column_axis(wave)] = 1.0
    pattern = absorbing.incident_pattern(ids, Cn, d, case.packing.node_count)
    pts, steps = ac.incident_curve(wave, dt)
    vals = np.array([p[1] for p in pts] + [pts[-1][1]])
    return dict(ids=ids, Cn=Cn, pattern=pattern, pts=pts, steps=steps, vals=vals)


def ledger_of_f64_run(wave, dt, with_dissipation=True):
    """The ledger rows [steps, 4] of the all-float64 dense run of the incident-wave column, every step sampled."""
    ref = ac.column_dense(wave)
    K, mass, fixed = ref["K"], ref["mass"], ref["fixed"]
    R = column_incident(wave, dt)
    states = list(ac.scheme_f64(K, mass, fixed, dt, R["steps"] + 1, lambda n: R["vals"][n] * R["pattern"],
                                (R["ids"], R["Cn"])))
    led = LedgerReference()
    for i in range(len(states) - 1):
        _, u, v = states[i]
        _, un, vn = states[i + 1]
        t = energy_terms(mass, fixed, 0.0, dt, v, K @ u, R["vals"][i] * R["pattern"], un, vn, (R["ids"], R["Cn"]),
                         with_dissipation)
        led.add(i + 1, t)
    return led.arrays()[1]
