"""Shared by the tied-boundary tests: blocks whose lateral perimeter can be tied (one constraint mask per group), the
group records P_G | Q_G by the library for explicit_common.scheme_steps (the scheme of include/cwf_hip.h "Tied
boundaries" in numpy), the projection of v, and the reduced dense system (T^T K T, T^T M T) for all-fp64 runs."""
import functools
from dataclasses import replace

import numpy as np

import absorbing_common as ac
import explicit_common as xc
from cwf import _lib, meshgen, pack, scenarios, ties
from cwf.physics import Assignment, DirichletFix


# ---- meshes ---------------------------------------------------------------------------------------------------------
def perimeter(X):
    """The nodes on the four lateral faces (x or y at an end of the block)."""
    lo, hi = X.min(0), X.max(0)
    return np.nonzero((X[:, 0] == lo[0]) | (X[:, 0] == hi[0]) | (X[:, 1] == lo[1]) | (X[:, 1] == hi[1]))[0]


@functools.lru_cache(maxsize=None)
def tie_case(nx=4, ny=3, nz=3, h=0.25, jitter=False, element="tet4", harmonic=None, hold_side=True):
    """scenarios.block_case's block with other constraints: nothing is held at x = 0; with hold_side every lateral
    perimeter node (group SIDE) is held in y, so the members of a level share the mask 2 and the interior is free.
    Groups SIDE, BASE (z = 0), and the block's own TIP (the point load's face)."""
    tm = meshgen.hex_block(nx, ny, nz, h) if element == "hex8" else meshgen.kuhn_block(nx, ny, nz, h)
    tm.node_groups["SIDE"] = perimeter(tm.coords).astype(np.uint32)
    tm.node_groups["BASE"] = np.nonzero(tm.coords[:, 2] == 0.0)[0].astype(np.uint32)
    if jitter:
        tm = meshgen.jitter_and_permute(tm, h)
    mesh = pack.from_tetmesh(tm)
    fixes = [DirichletFix("SIDE", (False, True, False), (None, 0.0, None))] if hold_side else []
    cfg = scenarios.make_config(dirichlet=fixes, harmonic=harmonic)
    case = scenarios.Case(f"tie{nx}x{ny}x{nz}", mesh, cfg, pack.build_packed_buffers(mesh, cfg))
    assert np.array_equal(np.sort(xc.group(case, "SIDE")), perimeter(mesh.coords))
    return case


@functools.lru_cache(maxsize=None)
def column3d_case(nz=ac.COLUMN_NZ, h=ac.COLUMN_H):
    """absorbing_common's column, kuhn_block(2, 2, nz, h) of the soil m1, with no held axes and no loads."""
    tm = meshgen.kuhn_block(2, 2, nz, h)
    n = np.arange(tm.node_count, dtype=np.uint32)
    tm.node_groups["ALL"] = n
    tm.node_groups["BASE"] = n[:9]
    tm.node_groups["TOP"] = n[-9:]
    mesh = pack.from_tetmesh(tm)
    cfg = scenarios.make_config(gravity=(0.0, 0.0, 0.0), point=(0.0, 0.0, 0.0), dirichlet=[])
    cfg = replace(cfg, materials=[ac.SOIL], assignments=[Assignment("SOLID", ac.SOIL.name)])
    return scenarios.Case("column3d", mesh, cfg, pack.build_packed_buffers(mesh, cfg))


def plane_ties(case):
    """Every plane of the column as one group of 9 -> (offsets, ids)."""
    return ties.levels(case.mesh.coords, np.arange(case.packing.node_count), 2)


# ---- the restatement's tie records ----------------------------------------------------------------------------------
def group_records(groups, mass32, alpha, dt, dash=None):
    """M_G [G], P_G, Q_G [G,3,3] by cwf_explicit_dashpot_update(C_G, M_G): M_G and C_G summed in member order (C_G from
    the first member with a dashpot). dash: (ids, C [n,3,3]) or None."""
    L = _lib.load()
    where = {} if dash is None else {int(n): i for i, n in enumerate(dash[0])}
    M, P, Q = np.zeros(len(groups)), np.zeros((len(groups), 3, 3)), np.zeros((len(groups), 3, 3))
    for g, members in enumerate(groups):
        m, CG = None, None
        for n in members:
            mn = float(np.float64(np.float32(mass32[n])))
            m = mn if m is None else m + mn
            if int(n) in where:
                Ci = np.asarray(dash[1][where[int(n)]], np.float64)
                CG = Ci.copy() if CG is None else CG + Ci
        CG = np.zeros((3, 3)) if CG is None else np.ascontiguousarray(CG)
        rc = L.cwf_explicit_dashpot_update(_lib.ptr(CG), m, float(alpha), float(dt), _lib.ptr(P[g]), _lib.ptr(Q[g]))
        assert rc == 0, (g, _lib.last_error(None))
        M[g] = m
    return M, P, Q


def project(v, groups, mass32, fixed):
    """set_ties' projection: every member's v becomes f32(sum f64(m_i) f64(v_i) / M_G), constrained components 0."""
    out = np.array(v, np.float32).reshape(-1, 3)
    fx = np.asarray(fixed).reshape(-1, 3)
    for members in groups:
        M, acc = None, None
        for n in members:
            mn = float(np.float64(np.float32(mass32[n])))
            t = mn * out[n].astype(np.float64)
            M, acc = (mn, t) if M is None else (M + mn, acc + t)
        mean = (acc / M).astype(np.float32)
        mean[fx[members[0]]] = 0.0
        out[members] = mean
    return out.reshape(-1)


# ---- the reduced dense system ---------------------------------------------------------------------------------------
def reduction(groups, node_count):
    """The 0/1 map of the ties by nodes: reduced node r of node n (a group is one reduced node, an untied node its
    own) -> (rnode [N], reduced node count)."""
    rnode = np.full(node_count, -1, np.int64)
    for g, members in enumerate(groups):
        rnode[members] = g
    rest = np.nonzero(rnode < 0)[0]
    rnode[rest] = len(groups) + np.arange(rest.size)
    return rnode, len(groups) + rest.size


def reduced_system(K, mass, fixed, groups, dash=None):
    """(T^T K T, T^T M T) and the constraints of the reduced DOFs -> dict(K, mass, fixed, T-as-index `dof` [D] (u = ur[dof]),
    dash (reduced ids, C_G) or None)."""
    D = mass.size
    rnode, R = reduction(groups, D // 3)
    dof = (3 * rnode[:, None] + np.arange(3)[None, :]).reshape(-1)
    T = np.zeros((D, 3 * R))
    T[np.arange(D), dof] = 1.0
    Kr = T.T @ K @ T
    mr = T.T @ mass
    fr = np.zeros(3 * R, bool)
    fr[dof[fixed]] = True
    rd = None
    if dash is not None:
        ids = np.unique(rnode[np.asarray(dash[0], np.int64)])
        CG = np.zeros((ids.size, 3, 3))
        for n, Ci in zip(dash[0], dash[1]):
            CG[np.searchsorted(ids, rnode[n])] += Ci
        rd = (ids, CG)
    return dict(K=Kr, mass=mr, fixed=fr, dof=dof, dash=rd, T=T)


def lam_max(K, mass, fixed):
    s = 1.0 / np.sqrt(mass[~fixed])
    return float(np.linalg.eigvalsh(K[np.ix_(~fixed, ~fixed)] * s[:, None] * s[None, :])[-1])


# ---- the tied 3-D column --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def column_reference():
    """The tied 3-D column (every plane of 9 nodes one group, dashpots on the base, the Gaussian incident S pulse of
    absorbing_common.incident_curve) at dt = 0.9 x the untied critical step of the dense K: the all-fp64 run of the
    reduced dense system, the all-fp64 untied and unheld control, and the float32 restatement (its operator the dense K
    in fp64, rounded to f32) whose distance from the reduced run at the run's end is the f32-storage floor."""
    from cwf import absorbing

    case = column3d_case()
    P = case.packing
    N, D = P.node_count, P.dof_count
    ref = ac.dense_of(case)
    K, mass, fixed = ref["K"], ref["mass"], ref["fixed"]
    assert not fixed.any()
    dt = 0.9 * 2.0 / np.sqrt(ref["lam_max"])
    ids, Cn = absorbing.dashpots(case.mesh, case.cfg, absorbing.faces_of_group(case.mesh, "BASE"))
    pattern = absorbing.incident_pattern(ids, Cn, np.array([1.0, 0.0, 0.0]), N)
    pts, steps = ac.incident_curve("S", dt)
    assert steps + 2 <= 4096
    vals = np.array([p[1] for p in pts] + [pts[-1][1]] * 2)
    off, tids = plane_ties(case)
    groups = ties.groups_of(off, tids)
    assert len(groups) == ac.COLUMN_NZ + 1 and all(len(g) == 9 for g in groups)
    red = reduced_system(K, mass, fixed, groups, (ids, Cn))
    dof, T = red["dof"], red["T"]
    run = list(ac.scheme_f64(red["K"], red["mass"], red["fixed"], dt, steps + 1, lambda n: T.T @ (vals[n] * pattern),
                             red["dash"]))
    E = ac.energies_f64(red["K"], red["mass"], run)
    top = 3 * xc.group(case, "TOP")
    top_v = np.array([s[2][dof][top].mean() for s in run])
    npk = int(np.abs(top_v).argmax())
    doubling, left = float(np.abs(top_v).max()) / 1e-3, float(E[-1] / E.max())
    control = list(ac.scheme_f64(K, mass, fixed, dt, npk, lambda n: vals[n] * pattern, (ids, Cn)))
    ux = control[npk][1][top]
    top_u_peak = float(run[npk][1][dof][top].mean())
    control_spread = float(ux.max() - ux.min()) / abs(top_u_peak)
    # the float32 restatement with the dense operator
    mass32 = P.lumped_mass
    MG, PG, QG = group_records(groups, mass32, 0.0, dt, (ids, Cn))
    u, v = xc.host_scheme(lambda w: (K @ w.astype(np.float64)).astype(np.float32), np.repeat(mass32, 3), fixed,
                          np.zeros(D, np.float32), lambda n: pack._safe_f32(vals[n] * pattern), 0.0, 0.0, dt,
                          np.zeros(D, np.float32), np.zeros(D, np.float32), 0, steps, None, (groups, MG, PG, QG))
    u_end, v_end = run[steps][1][dof], run[steps][2][dof]

    def dev(a, b):
        return float(np.abs(a.astype(np.float64) - b).max() / np.abs(b).max())

    def assert_conditions():
        assert abs(doubling - 2.0) <= 0.02 * 2.0, doubling
        assert left <= 1e-3, left

    return dict(dt=dt, steps=steps, pts=pts, pattern=pattern, ids=ids, Cn=Cn, ties=(off, tids), groups=groups, npk=npk,
                conditions=f"peak top velocity / incident peak {doubling:.4f}, energy end / peak {left:.2e}",
                doubling=doubling, left=left, assert_conditions=assert_conditions, control_spread=control_spread,
                top_u_peak=top_u_peak, u_end=u_end, v_end=v_end, floor_u=dev(u, u_end), floor_v=dev(v, v_end),
                u32=u, v32=v)
