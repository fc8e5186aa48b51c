"""Shared by the load-source tests: the header's semantics block ("Load sources", include/cwf_hip.h) restated in
numpy, the source sets the bit-for-bit cases run, and the free-field slab (an obliquely incident plane wave through a
plane-strain slab with dashpots and free-field input on its four faces) with its all-float64 reference."""
import functools
import math
from dataclasses import replace

import numpy as np

import absorbing_common as ac
import explicit_common as xc
from cwf import absorbing, explicit, meshgen, pack, scenarios
from cwf.explicit import LoadSource
from cwf.physics import Assignment, DirichletFix, compute_lame


# ---- the semantics block --------------------------------------------------------------------------------------------
def curve_values(points, ts):
    """cwf_explicit_curve_value (the library's host function, a linear scan) at each of ts."""
    cache = {}
    out = np.empty(len(ts))
    for i, t in enumerate(ts):
        t = float(t)
        if t not in cache:
            cache[t] = explicit.curve_value(points, t)
        out[i] = cache[t]
    return out


def source_force(fext32, sources, n, dt, reverse=False):
    """f_n [3N] float32: acc = (double)f_ext, then per source in ascending index acc = acc + A c(n dt - tau) (the
    product rounded, then the sum: numpy fuses nothing), safe_cast at the loaded nodes; f_ext elsewhere.
    reverse: the sources in descending order instead (to show that the order is visible in the bits)."""
    acc = fext32.astype(np.float64).reshape(-1, 3).copy()
    loaded = np.zeros(acc.shape[0], bool)
    tn = float(n) * dt
    for s in (list(sources)[::-1] if reverse else sources):
        ids = np.asarray(s.node_ids, np.int64)
        c = curve_values(s.points(), tn - np.asarray(s.delay, np.float64))
        acc[ids] = acc[ids] + np.asarray(s.amplitude, np.float64).reshape(-1, 3) * c[:, None]
        loaded[ids] = True
    out = fext32.copy().reshape(-1, 3)
    out[loaded] = pack._safe_f32(acc[loaded].reshape(-1)).reshape(-1, 3)
    return out.reshape(-1)


# ---- the sets of the bit-for-bit cases ------------------------------------------------------------------------------
def mixed_sources(rng, case, dt):
    """Eight sources on 65 nodes of the 80-node block; see mixed_facts for what they cover between them."""
    N = case.packing.node_count
    fixed = xc.group(case, "FIXED")
    over = int(fixed[3])
    free = np.setdiff1d(np.arange(N), fixed)
    hub = int(free[rng.integers(free.size)])
    rest = rng.permutation(np.setdiff1d(np.arange(N), [hub, over]))[:63]
    pool = np.concatenate([[hub, over], rest])
    assert np.intersect1d(rest, fixed).size > 0  # constrained loaded nodes beside the overflowing one

    def amp(n):
        return 1e3 * rng.standard_normal((n, 3))

    def with_hub(nodes):
        return np.concatenate([nodes, [hub]]).astype(np.uint32)

    k = float
    t0 = np.arange(4096) * (dt / 16.0)
    long_curve = list(zip(t0, 1.0 + np.cumsum(rng.standard_normal(4096)) * 0.05))
    out = [
        LoadSource(long_curve, with_hub(pool[2:42]), amp(41), rng.uniform(-20.0 * dt, 30.0 * dt, 41)),
        LoadSource([(0.0, 0.7)], with_hub(pool[37:47]), amp(11), rng.uniform(-5.0 * dt, 5.0 * dt, 11)),
        LoadSource([(0.0, 0.0), (k(20) * dt, 1.0)], with_hub(pool[47:56]), amp(10), np.zeros(10)),
        LoadSource([(0.0, 0.0), (k(5) * dt, 0.0), (k(5) * dt, 1.0), (k(30) * dt, 1.0), (k(30) * dt, -0.5),
                    (k(40) * dt, 0.0)], with_hub(pool[56:65]), amp(10),
                   np.concatenate([np.zeros(5), rng.uniform(0.0, 10.0 * dt, 5)])),
        LoadSource([(0.0, 1.0), (k(10) * dt, 1.0), (k(20) * dt, 1.0)], np.array([over, hub], np.uint32),
                   np.array([[1e39, -1e39, 5.0], amp(1)[0]]), np.array([0.0, -2.5 * dt])),
    ]
    # sources 5 and 6 cancel each other at the hub with amplitudes of 1e13: what of the smaller terms survives the
    # float32 cast depends on where in the sum the pair stands, so the ascending order shows in the bits
    pts = [(0.0, 0.5 + rng.random()), (k(7) * dt, 0.5 + rng.random()), (k(60) * dt, 0.5 + rng.random())]
    pair, tau = np.array([[3e13, -7e13, 1e13]]), rng.uniform(-3.0 * dt, 3.0 * dt, 1)
    out.append(LoadSource(pts, np.array([hub], np.uint32), pair, tau))
    out.append(LoadSource(pts, np.array([hub], np.uint32), -pair, tau))
    pts = [(0.0, rng.standard_normal()), (k(7) * dt, rng.standard_normal()), (k(60) * dt, rng.standard_normal())]
    out.append(LoadSource(pts, np.array([hub], np.uint32), amp(1), rng.uniform(-3.0 * dt, 3.0 * dt, 1)))
    return out


def mixed_facts(sources, dt, steps, node_count):
    """What a set covers over steps 0 .. steps - 1, computed from the set itself."""
    count = np.zeros(node_count, np.int64)
    f = dict(before_first=False, on_a_knot=False, between=False, past_last=False, negative_delay=False,
             duplicate_knot=False, points=set(), entries=0, overflow_node=None)
    for s in sources:
        ids = np.asarray(s.node_ids, np.int64)
        count[ids] += 1
        times = np.array([p[0] for p in s.points()])
        f["points"].add(times.size)
        f["entries"] += ids.size
        f["duplicate_knot"] |= bool(np.any(np.diff(times) == 0.0))
        f["negative_delay"] |= bool(np.any(np.asarray(s.delay) < 0.0))
        big = np.abs(np.asarray(s.amplitude)).max(1) > 1e38
        if big.any():
            f["overflow_node"] = int(ids[big][0])
        for n in range(steps):
            t = float(n) * dt - np.asarray(s.delay, np.float64)
            f["before_first"] |= bool(np.any(t < times[0]))
            f["past_last"] |= bool(np.any(t > times[-1]))
            on = np.isin(t, times[1:]) if times.size > 1 else np.zeros(t.size, bool)
            f["on_a_knot"] |= bool(on.any())
            f["between"] |= bool(np.any((t > times[0]) & (t < times[-1]) & ~np.isin(t, times)))
    f["loaded"] = int((count > 0).sum())
    f["entries_per_node"] = set(int(c) for c in count[count > 0])
    f["hub"] = int(count.argmax())
    return f


def spread_sources(rng, case, dt, loaded=257):
    """Two sources: a 64-point curve on `loaded` random nodes with their own delays, a ramp on the first half."""
    N = case.packing.node_count
    nodes = rng.permutation(N)[:loaded].astype(np.uint32)
    times = np.sort(rng.uniform(0.0, 60.0 * dt, 64))
    curve = list(zip(times, rng.standard_normal(64)))
    half = nodes[:max(loaded // 2, 1)]
    return [LoadSource(curve, nodes, 1e3 * rng.standard_normal((loaded, 3)), rng.uniform(-5.0 * dt, 20.0 * dt, loaded)),
            LoadSource([(0.0, 0.0), (float(25) * dt, 1.0)], half, 1e3 * rng.standard_normal((half.size, 3)),
                       rng.uniform(0.0, 10.0 * dt, half.size))]


def record_sources(rng, case, dt):
    """A three-component record: three sources on every node, zero delay, source k along axis k."""
    N = case.packing.node_count
    scale = 1e3 * (1.0 + rng.random(N))
    out = []
    for k in range(3):
        A = np.zeros((N, 3))
        A[:, k] = scale
        rec = list(zip(np.arange(128) * (dt / 2.0), np.cumsum(rng.standard_normal(128)) * 0.1))
        out.append(LoadSource(rec, rng.permutation(N).astype(np.uint32), A, np.zeros(N)))
    return out


def one_node_source(rng, case, dt):
    return [LoadSource([(0.0, 0.0), (2.0 * dt, 1.0), (9.0 * dt, -1.0), (30.0 * dt, 0.25)], np.array([41], np.uint32),
                       1e3 * rng.standard_normal((1, 3)), np.array([3.5 * dt]))]


BIG_SETS = {"n257": spread_sources, "every": record_sources}


# ---- the free-field slab --------------------------------------------------------------------------------------------
SLAB_H = 0.25
SLAB_SIGMA = 4.0      # the pulse's spatial standard deviation c sigma_t in cells, for the wave it is made for
SLAB_ANGLE = 30.0     # khat from +z, in the x-z plane
SLAB_PEAK = 1e-3      # m/s


@functools.lru_cache(maxsize=None)
def slab_case(nx, nz, h=SLAB_H):
    """kuhn_block(nx, 1, nz, h) of the soil m1 with u_y held on every node: plane strain in the x-z plane."""
    tm = meshgen.kuhn_block(nx, 1, nz, h)
    tm.node_groups["ALL"] = np.arange(tm.node_count, dtype=np.uint32)
    mesh = pack.from_tetmesh(tm)
    fixes = [DirichletFix("ALL", (False, True, False), (None, 0.0, None))]
    cfg = scenarios.make_config(gravity=(0.0, 0.0, 0.0), point=(0.0, 0.0, 0.0), dirichlet=fixes)
    cfg = replace(cfg, materials=[ac.SOIL], assignments=[Assignment("SOLID", ac.SOIL.name)])
    return scenarios.Case(f"slab-{nx}x{nz}", mesh, cfg, pack.build_packed_buffers(mesh, cfg))


def slab_wave(wave):
    """(d, khat, c) of the P or the SV wave at SLAB_ANGLE."""
    a = math.radians(SLAB_ANGLE)
    k = np.array([math.sin(a), 0.0, math.cos(a)])
    d = k if wave == "P" else np.array([math.cos(a), 0.0, -math.sin(a)])
    return d, k, ac.wave_speed(ac.SOIL, "P" if wave == "P" else "S")


@functools.lru_cache(maxsize=None)
def slab_boundary(nx, nz, wave):
    """Dashpots and the plane wave's entries on the four faces x = min / max, z = min / max -> (ids, Cn, source ids,
    A, tau, interior nodes). The origin is the corner the front reaches first, so every delay is >= 0."""
    case = slab_case(nx, nz)
    m, X = case.mesh, case.mesh.coords
    lo, hi = X.min(0), X.max(0)
    faces = np.concatenate([meshgen.boundary_faces(m.tets, np.nonzero(X[:, a] == v)[0])
                            for a, v in ((0, lo[0]), (0, hi[0]), (2, lo[2]), (2, hi[2]))])
    ids, Cn = absorbing.dashpots(m, case.cfg, faces)
    d, k, c = slab_wave(wave)
    sid, A, tau, speed = absorbing.incident_plane_wave(m, case.cfg, faces, d, k, (lo[0], 0.0, lo[2]))
    assert speed == c and np.array_equal(sid, ids) and tau.min() >= 0.0
    margin = 3.0 * SLAB_H
    inside = np.all((X[:, [0, 2]] >= lo[[0, 2]] + margin) & (X[:, [0, 2]] <= hi[[0, 2]] - margin), axis=1)
    return ids, Cn, sid, A, tau, np.nonzero(inside)[0]


def slab_pulse(nx, nz, wave):
    """The Gaussian velocity pulse g(t) = peak exp(-1/2 ((t - t0) / sigma_t)^2) with c sigma_t = SLAB_SIGMA cells and
    t0 = 6 sigma_t, and the time by which it has crossed the slab and left: -> (sigma_t, t0, t_end). The dominant
    wavelength, taken at the spectrum's 1 / sqrt(e) point omega = 1 / sigma_t, is 2 pi SLAB_SIGMA = 25 cells."""
    d, k, c = slab_wave(wave)
    sigma_t = SLAB_SIGMA * SLAB_H / c
    t0 = 6.0 * sigma_t
    cross = (k[0] * nx + k[2] * nz) * SLAB_H / c
    return sigma_t, t0, t0 + cross + 6.0 * sigma_t


def slab_curve(nx, nz, wave):
    """The pulse as a 4096-point curve over [0, t_end]: finer than any step, so the linear interpolation between its
    points is exact to (spacing / sigma_t)^2 / 8 < 1e-5 of the peak."""
    sigma_t, t0, t_end = slab_pulse(nx, nz, wave)
    t = np.linspace(0.0, t_end, 4096)
    return list(zip(t, SLAB_PEAK * np.exp(-0.5 * ((t - t0) / sigma_t) ** 2)))


def slab_analytic(nx, nz, wave, t, nodes):
    """u = d G(t - tau(x)) and v = d g(t - tau(x)) of the plane wave at `nodes`, [n,3] each; G the integral of g."""
    case = slab_case(nx, nz)
    X = case.mesh.coords
    d, k, c = slab_wave(wave)
    sigma_t, t0, _ = slab_pulse(nx, nz, wave)
    lo = X.min(0)
    s = t - (X[nodes] - np.array([lo[0], 0.0, lo[2]])) @ k / c
    g = SLAB_PEAK * np.exp(-0.5 * ((s - t0) / sigma_t) ** 2)
    G = SLAB_PEAK * sigma_t * math.sqrt(math.pi / 2.0) * (1.0 + np.vectorize(math.erf)((s - t0) / (sigma_t * math.sqrt(2.0))))
    return G[:, None] * d[None, :], g[:, None] * d[None, :]


def slab_force(nx, nz, wave, dt, delays=True):
    """force_at(n) of the float64 reference: the source's A g(n dt - tau) scattered into a [3N] vector."""
    case = slab_case(nx, nz)
    ids, Cn, sid, A, tau, _ = slab_boundary(nx, nz, wave)
    pts = slab_curve(nx, nz, wave)
    times, values = np.array([p[0] for p in pts]), np.array([p[1] for p in pts])
    if not delays:
        tau = np.zeros_like(tau)
    N = case.packing.node_count

    def force_at(n):
        f = np.zeros((N, 3))
        f[sid] = A * np.interp(n * dt - tau, times, values)[:, None]
        return f.reshape(-1)

    return force_at


def slab_deviation(nx, nz, wave, dt, states):
    """A run's worst deviation from the analytic wave at the interior nodes over its steps: (u, v), each relative to
    the analytic field's own maximum (v: the half-step velocity against g at t_(n-1/2))."""
    inside = slab_boundary(nx, nz, wave)[5]
    du = dv = 0.0
    umax = vmax = 0.0
    for n, u, v in states:
        ua, _ = slab_analytic(nx, nz, wave, n * dt, inside)
        _, va = slab_analytic(nx, nz, wave, (n - 0.5) * dt, inside)
        du = max(du, float(np.abs(np.asarray(u, np.float64).reshape(-1, 3)[inside] - ua).max()))
        dv = max(dv, float(np.abs(np.asarray(v, np.float64).reshape(-1, 3)[inside] - va).max()))
        umax, vmax = max(umax, float(np.abs(ua).max())), max(vmax, float(np.abs(va).max()))
    return du / umax, dv / vmax


@functools.lru_cache(maxsize=None)
def slab_dense(nx, nz):
    from helpers import dense_stiffness

    case = slab_case(nx, nz)
    P = case.packing
    D = P.dof_count
    K = dense_stiffness(P, case.mesh.coords, case.mesh.tets, case.materials[0].stiffness).reshape(D, D)
    fixed = xc.constrained(P)
    mass = np.repeat(P.lumped_mass.astype(np.float64), 3)
    for a in (K, fixed, mass):
        a.setflags(write=False)
    return K, mass, fixed


@functools.lru_cache(maxsize=None)
def slab_reference(nx, nz, wave, dt):
    """The all-float64 runs with the dense K: with delays (A), the same with operator and force through float32 (B,
    the f32-operator floor), and with every delay zero. -> dict(steps, A, B, zero, dev_A, dev_zero, left, floor_u,
    floor_v); the deviations are slab_deviation's, `left` the energy at the end over its peak (run A)."""
    K, mass, fixed = slab_dense(nx, nz)
    ids, Cn = slab_boundary(nx, nz, wave)[:2]
    steps = int(math.ceil(slab_pulse(nx, nz, wave)[2] / dt))
    with_tau, without = slab_force(nx, nz, wave, dt), slab_force(nx, nz, wave, dt, delays=False)
    A = list(ac.scheme_f64(K, mass, fixed, dt, steps + 1, with_tau, (ids, Cn)))
    B = list(ac.scheme_f64(K, mass, fixed, dt, steps + 1, with_tau, (ids, Cn), round_operator=True))
    Z = list(ac.scheme_f64(K, mass, fixed, dt, steps + 1, without, (ids, Cn)))
    E = ac.energies_f64(K, mass, A)
    npk = int(E.argmax())

    def dev(a, ref):
        return float(np.abs(a - ref).max() / np.abs(ref).max())

    return dict(steps=steps, A=A, B=B, npk=npk, dev_A=slab_deviation(nx, nz, wave, dt, A[:-1]),
                dev_zero=slab_deviation(nx, nz, wave, dt, Z[:-1]), left=float(E[-1] / E.max()),
                floor_u=dev(B[npk][1], A[npk][1]), floor_v=dev(B[npk][2], A[npk][2]))
