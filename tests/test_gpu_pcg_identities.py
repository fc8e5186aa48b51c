"""The operators and the scalars inside the FAST PCG schedules, pinned by identities of the first six iterates against
the fp64 reference of tests/operator_probe_common.py. apply_keff never runs the operators of k_pcg_resident and
k_pcg_lattice, and a whole solve tolerates a slightly wrong operator, a dropped dot share or a stale alpha; the
iterates themselves do not.

For j = 1 .. 6 a cold solve with max_iterations = j and tol = 1e-30 gives x_j, r_j and the telemetry (the fused launch
rotates four p buffers and two r / Ap parities, so six iterations pass every buffer twice). With d = x_j - x_(j-1),
q = r_(j-1) - r_j (x_0 = 0, r_0 = b), all in fp64, on the free rows (u = 2^-24, A = sum_e |Ke|, c_v the family's
vector cap of tests/test_gpu_operator_probe.py):

  recurrence   |q - K_ref d|_i <= u [c_v (A|d|)_i + 2 (A|x_j|)_i + 2 (|r_(j-1)|_i + |r_j|_i)]: the operator's
               rounding, the stored x's and the stored r's. At j = 1, d = x_1: the in-kernel operator entry-wise.
  constrained  x_j and r_j on constrained DOFs are the oracle's (x = b, r = 0).
  j = 1        x_1 = alpha_last M^-1 b within 8 u alpha_last (|M^-1||b|)_i, M^-1 = pcg.fast_block_inverse;
               alpha_last = (b.z) / (z.K_ref z) within (c_v + 8) u (|z|.A|z|) / (z.K_ref z) relative.
  j >= 2       eta_j = |r_j.d| / sum_i (|r_(j-1)|_i + (A|d|)_i) |d_i| <= max(64 u, 8 eta_j of the oracle's own
               truncated solves (tets: the pinned f32 PCG; hex8: its numpy restatement on K_ref)). A 1% error in
               alpha gives eta >~ 1e-4.
  telemetry    iterations == j; residual_norm = |r_j|_2 of the returned r and rhs_norm = |b|_2, formed in fp64,
               within D 2^-52 relative; residual_history[j] == residual_norm. The fused and the resident launches
               by design sum each node's r.r formed in fp32 (three roundings), so their residual_norm carries
               1.5 u more; measured gap at most 1.1e-8.

The j = 1 check found alpha_last and beta_last of the fused and resident schedules one iteration ahead at a
max-iterations stop (the scalars of the update that never runs; 5 - 46% off alpha_1 here); lattice_common.hpp
fused_decide now leaves them at the last update made, as pcg.cpp and the two-kernel schedule report them.

Trivial stops (zero rhs, rhs on constrained DOFs only, tol = 0.99, warm starts) follow the oracle's solve_pcg on the
same input. The last test runs the recurrence and eta on slab shards of one block through the LOCAL communicator.
Measured eta per schedule: profiles/operator_probe_accuracy.txt."""
import functools

import numpy as np
import pytest

import operator_probe_common as OP
from cwf import _lib, pcg, scenarios
from helpers import oracle_system
from test_gpu_lattice_layered import SHAPES as LAYERED_SHAPES
from test_gpu_operator_probe import CAPS, family_of

pytestmark = pytest.mark.gpu

U = OP.U
KNOBS = ("CWF_FUSED", "CWF_RESIDENT", "CWF_LATTICE", "CWF_LAT_ZR", "CWF_LAT_L", "CWF_FUSED_MAXWG", "CWF_GROUPS",
         "CWF_GROUP_NT", "CWF_GEO", "CWF_TILE_PIPE", "CWF_RENUMBER", "CWF_HEX_NT")
CASES = {
    "40x17x9": lambda: scenarios.block_case(40, 17, 9, h=0.1),
    "rollers-12x10x7": lambda: scenarios.roller_case(12, 10, 7),
    "hex8-33x9x5": lambda: scenarios.block_case(33, 9, 5, h=0.1, element="hex8"),
    "thin-3x3x60": lambda: scenarios.block_case(3, 3, 60, h=0.1),
    "rayleigh-6x4x3": lambda: scenarios.block_case(6, 4, 3, h=0.1, xi=0.05, w=(10.0, 100.0)),
    "layered-12x10x9": lambda: scenarios.layered_case(*LAYERED_SHAPES["12x10x9"][0], LAYERED_SHAPES["12x10x9"][1]),
    "layered-5x4x4": lambda: scenarios.layered_case(*LAYERED_SHAPES["5x4x4"][0], LAYERED_SHAPES["5x4x4"][1]),
    "jitter-7x6x5": lambda: scenarios.block_case(7, 6, 5, h=0.1, jitter=True),
    "hex8-6x4x3": lambda: scenarios.block_case(6, 4, 3, h=0.1, element="hex8"),
}
BLOCKS = ["40x17x9", "rollers-12x10x7", "hex8-33x9x5", "thin-3x3x60", "rayleigh-6x4x3"]
# schedule -> (knobs, kernel prefix, cases of the identities, case of the trivial stops)
SCHEDULES = {
    "resident": ({}, "k_pcg_resident", BLOCKS, "rayleigh-6x4x3"),
    "fused": ({"CWF_FUSED": "1"}, "k_pcg_lattice", BLOCKS, "rayleigh-6x4x3"),
    "two-kernel-z-stored": ({"CWF_FUSED": "0", "CWF_LAT_ZR": "0"}, "k_keff_lattice<", BLOCKS, "rayleigh-6x4x3"),
    "two-kernel-z-from-r": ({"CWF_FUSED": "0", "CWF_LAT_ZR": "1"}, "k_keff_lattice<", BLOCKS, "rayleigh-6x4x3"),
    "layered": ({}, "k_keff_lattice_layered", ["layered-12x10x9"], "layered-5x4x4"),
    "fan-groups": ({}, "k_keff_groups_pipe", ["jitter-7x6x5"], "jitter-7x6x5"),
    "hex-tiles": ({"CWF_LATTICE": "0"}, "k_keff_hex_tiles", ["hex8-33x9x5"], "hex8-6x4x3"),
}
IDENTITY_CASES = [(s, c) for s, v in SCHEDULES.items() for c in v[2]]
FP32_NODE_NORMS = ("k_pcg_resident", "k_pcg_lattice")  # schedules whose |r| sums per-node fp32 products (see the test)
STEPS = 6


@functools.lru_cache(maxsize=None)
def case_of(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def reference(name):
    return OP.reference_of(case_of(name))


@functools.lru_cache(maxsize=None)
def rhs_of(name, kind):
    case = case_of(name)
    if kind == "static":
        b = case.static_rhs()
    else:
        b = np.random.Generator(np.random.PCG64(17)).uniform(-1, 1, case.packing.dof_count).astype(np.float32)
        b[reference(name).fixed] = 0.0
    b.setflags(write=False)
    return b


def numpy_pcg(ref, Minv, b, max_iterations, tol, x0=None):
    """orc_solve_pcg restated on K_ref (hex8 has no oracle solve): f32 vectors, fp64 operator rounded once per row,
    fp64 dots. -> dict(x, r, iterations, converged)."""
    f32 = np.float32
    fixed = ref.fixed

    def precondition(r):
        return np.einsum("nij,nj->ni", Minv, r.astype(np.float64).reshape(-1, 3)).reshape(-1).astype(f32)

    def dot(a, c):
        return float(a.astype(np.float64) @ c.astype(np.float64))

    x = np.zeros(ref.D, f32) if x0 is None else np.array(x0, f32)
    r = b - ref.apply(x).astype(f32)
    x[fixed], r[fixed] = b[fixed], 0.0
    bn = np.sqrt(dot(b, b))
    limit = tol * (bn if bn >= 1e-12 else 1.0)
    out = dict(x=x, r=r, iterations=0, converged=True)
    if np.sqrt(dot(r, r)) <= limit:
        return out
    out["converged"] = False
    z = precondition(r)
    rho = dot(r, z)
    p = np.where(fixed, f32(0.0), z)
    for it in range(max_iterations):
        Ap = ref.apply(p).astype(f32)
        alpha = rho / dot(p, Ap)
        x += (alpha * p.astype(np.float64)).astype(f32)
        r -= (alpha * Ap.astype(np.float64)).astype(f32)
        x[fixed], r[fixed] = b[fixed], 0.0
        out["iterations"] = it + 1
        if np.sqrt(dot(r, r)) <= limit:
            out["converged"] = True
            break
        z = precondition(r)
        rho, rho0 = dot(r, z), rho
        p = np.where(fixed, f32(0.0), (z.astype(np.float64) + (rho / rho0) * p.astype(np.float64)).astype(f32))
    return out


def hex_block_inverse(name):
    """The fp64 block-Jacobi inverse of K_ref's node blocks, constrained axes as identity rows (test_hex8's)."""
    ref = reference(name)
    blk = np.zeros((ref.N, 3, 3))
    n = ref.conn.shape[1]
    for a in range(n):
        np.add.at(blk, ref.conn[:, a], ref.Ke[:, 3 * a:3 * a + 3, 3 * a:3 * a + 3])
    blk += ref.m.reshape(-1, 3)[:, :, None] * np.eye(3)[None]
    fx = ref.fixed.reshape(-1, 3)
    for k in range(3):
        blk[fx[:, k], k, :] = 0.0
        blk[fx[:, k], :, k] = 0.0
        blk[fx[:, k], k, k] = 1.0
    return np.linalg.inv(blk)


def reference_solve(name, b, max_iterations, tol, x0=None):
    """The oracle's solve_pcg of the case (tets), its numpy restatement on K_ref (hex8): dict(x, r, iterations,
    converged)."""
    case = case_of(name)
    if OP.is_hex(case):
        return numpy_pcg(reference(name), hex_block_inverse(name), np.asarray(b), max_iterations, tol, x0)
    o = oracle_system(case.packing, case.materials, *case.scalars())
    out = o.solve_pcg(b, max_iterations, tol, warm_start=x0 is not None, x=x0)
    t = out["telemetry"]
    return dict(x=out["x"], r=out["r"], iterations=int(t.iterations), converged=bool(t.converged))


@functools.lru_cache(maxsize=None)
def reference_iterates(name, kind):
    """x_j, r_j (fp64 [STEPS + 1, D]) of the reference's truncated solves and their eta_j, shared by the schedules."""
    b = rhs_of(name, kind)
    xs, rs = [np.zeros(b.size)], [b.astype(np.float64)]
    for j in range(1, STEPS + 1):
        s = reference_solve(name, b, j, 1e-30)
        assert s["iterations"] == j
        xs.append(s["x"].astype(np.float64))
        rs.append(s["r"].astype(np.float64))
    xs, rs = np.stack(xs), np.stack(rs)
    return xs, rs, etas(reference(name), xs, rs)


def etas(ref, xs, rs):
    """eta_j for j = 1 .. STEPS (index j; eta_0 = 0) and the fp64 pieces they are made of."""
    d = np.diff(xs, axis=0)
    Ad = ref.apply_abs(d.T).T
    out = np.zeros(xs.shape[0])
    free = ref.free
    for j in range(1, xs.shape[0]):
        dj = d[j - 1]
        den = float(np.sum(((np.abs(rs[j - 1]) + Ad[j - 1]) * np.abs(dj))[free]))
        out[j] = abs(float(rs[j][free] @ dj[free])) / den
    return out


def recurrence(ref, xs, rs, c_v):
    """(|q - K_ref d|_i over its bound, the worst free row per j (index j), and the operator's share alone at j = 1
    (d = x_1): what is left of the error after the x and r terms, in u (A|d|)_i)."""
    free = ref.free
    d, q = np.diff(xs, axis=0), -np.diff(rs, axis=0)
    Kd, Ad, Ax = ref.apply(d.T).T, ref.apply_abs(d.T).T, ref.apply_abs(xs[1:].T).T
    rec = np.zeros(xs.shape[0])
    for j in range(1, xs.shape[0]):
        bound = U * (c_v * Ad[j - 1] + 2.0 * Ax[j - 1] + 2.0 * (np.abs(rs[j - 1]) + np.abs(rs[j])))
        err = np.abs(q[j - 1] - Kd[j - 1])
        ok = free & (bound > 0)
        rec[j] = float(np.max(err[ok] / bound[ok]))
        assert np.all(err[free & (bound == 0)] == 0.0)
    rest = np.abs(q[0] - Kd[0]) - U * (2.0 * Ax[0] + 2.0 * (np.abs(rs[0]) + np.abs(rs[1])))
    ok = free & (Ad[0] > 0)
    return rec, max(0.0, float(np.max(rest[ok] / (U * Ad[0][ok]))))


def make_system(name, schedule, monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in SCHEDULES[schedule][0].items():
        monkeypatch.setenv(k, v)
    case = case_of(name)
    s = pcg.MatrixFreeSystem.from_packing(case.packing, case.materials, *case.scalars(), mode=_lib.MODE_FAST)
    kern = (_lib.load().cwf_hip_system_keff_kernel(s.handle()) or b"").decode()
    assert kern.startswith(SCHEDULES[schedule][1]), kern
    return s, kern


def solve(s, b, max_iterations, tol, x0=None):
    x = np.zeros_like(b) if x0 is None else np.array(x0, np.float32)
    r = np.zeros_like(b)
    t = pcg.solve_pcg(s, np.asarray(b), pcg.PcgSettings(max_iterations, tol, x0 is not None),
                      pcg.PcgVectors(x, r)).value()
    return t, x, r


@pytest.mark.parametrize("kind", ["static", "random"])
@pytest.mark.parametrize("schedule,name", IDENTITY_CASES)
def test_first_iterates_satisfy_the_pcg_identities(schedule, name, kind, monkeypatch):
    ref = reference(name)
    b = rhs_of(name, kind)
    b64 = b.astype(np.float64)
    xo, ro, eta_ref = reference_iterates(name, kind)
    s, kern = make_system(name, schedule, monkeypatch)
    c_v = CAPS[family_of(kern)][1]
    free, fixed = ref.free, ref.fixed
    D = ref.D
    xs, rs, tels, hists = [np.zeros(D)], [b64], [None], [None]
    for j in range(1, STEPS + 1):
        t, x, r = solve(s, b, j, 1e-30)
        xs.append(x.astype(np.float64))
        rs.append(r.astype(np.float64))
        tels.append(t)
        hists.append(pcg.residual_history(s))
    inv = np.zeros(9 * ref.N, np.float32)
    pcg.fast_block_inverse(s, inv).value()
    s.close()
    xs, rs = np.stack(xs), np.stack(rs)
    # telemetry
    bn = float(np.linalg.norm(b64))
    res_gap = rhs_gap = 0.0
    for j in range(1, STEPS + 1):
        t = tels[j]
        assert t.iterations == j and not t.converged
        rn = float(np.linalg.norm(rs[j]))
        res_gap, rhs_gap = max(res_gap, abs(t.residual_norm - rn) / rn), max(rhs_gap, abs(t.rhs_norm - bn) / bn)
        assert hists[j].size == j + 1 and hists[j][j] == t.residual_norm
    # fp64 sums of the stored f32 values in another order: D 2^-52. The fused and resident launches form each node's
    # r.r as one fp32 FMA chain of three non-negative terms (lattice_common.hpp fused_entry_dots) and sum those in
    # fp64: three roundings of u per node, so r.r within 3 u and its root within 1.5 u; measured 1.1e-8 at most
    # (profiles/operator_probe_accuracy.txt)
    res_cap = D * 2.0 ** -52 + (1.5 * U * (1 + 1e-3) if kern.startswith(FP32_NODE_NORMS) else 0.0)
    # constrained entries: the oracle's
    assert np.array_equal(xs[1:, fixed], xo[1:, fixed]) and np.array_equal(rs[1:, fixed], ro[1:, fixed])
    assert np.all(xs[1:, fixed] == b64[fixed]) and np.all(rs[1:, fixed] == 0.0)
    # the recurrence identity
    rec, op1 = recurrence(ref, xs, rs, c_v)
    # the preconditioner and alpha at j = 1
    Minv = inv.astype(np.float64).reshape(-1, 3, 3)
    z = np.einsum("nij,nj->ni", Minv, b64.reshape(-1, 3)).reshape(-1)
    za = np.einsum("nij,nj->ni", np.abs(Minv), np.abs(b64).reshape(-1, 3)).reshape(-1)
    z, za = np.where(fixed, 0.0, z), np.where(fixed, 0.0, za)
    alpha = tels[1].alpha_last
    x1 = float(np.max(np.abs(xs[1] - alpha * z)[free & (za > 0)] / (U * alpha * za[free & (za > 0)])))
    zKz = float(z @ np.where(fixed, 0.0, ref.apply(z)))
    alpha_ref = float(b64 @ z) / zKz
    alpha_err = abs(alpha - alpha_ref) / alpha_ref
    alpha_cap = (c_v + 8.0) * U * float(np.abs(z) @ np.where(fixed, 0.0, ref.apply_abs(z))) / zKz
    # alpha at j >= 2 through orthogonality
    eta = etas(ref, xs, rs)
    print(f"{schedule} {name} {kind}: {kern}  recurrence / bound per j {np.array2string(rec[1:], precision=3)} (c_v "
          f"{c_v:g}; the operator's share at j = 1: {op1:.2f} u A|d|)  x_1 {x1:.2f} of 8 u  alpha_1 error "
          f"{alpha_err:.2e} (cap {alpha_cap:.2e})  eta_j {np.array2string(eta[2:], precision=2)}  oracle eta_j "
          f"{np.array2string(eta_ref[2:], precision=2)}  residual_norm gap {res_gap:.2e} (cap {res_cap:.2e})  "
          f"rhs_norm gap {rhs_gap:.2e} (cap {D * 2.0 ** -52:.2e})")
    assert np.all(rec[1:] <= 1.0), rec
    assert x1 <= 8.0
    assert alpha_err <= alpha_cap
    for j in range(2, STEPS + 1):
        assert eta[j] <= max(64 * U, 8 * eta_ref[j]), (j, eta[j], eta_ref[j])
    assert res_gap <= res_cap
    assert rhs_gap <= D * 2.0 ** -52


@pytest.mark.parametrize("schedule", list(SCHEDULES))
def test_trivial_stops_follow_the_oracle(schedule, monkeypatch):
    name = SCHEDULES[schedule][3]
    ref = reference(name)
    s, kern = make_system(name, schedule, monkeypatch)
    D = ref.D
    b = rhs_of(name, "static")
    rng = np.random.Generator(np.random.PCG64(19))

    def both(what, rhs, its, tol, x0=None):
        t, x, r = solve(s, rhs, its, tol, x0)
        o = reference_solve(name, rhs, its, tol, x0)
        print(f"{schedule} {name} {what}: {kern}  ({t.iterations}, {t.converged}) oracle ({o['iterations']}, "
              f"{o['converged']})")
        assert (t.iterations, t.converged) == (o["iterations"], o["converged"]), what
        return t, x, r, o

    # zero rhs: converged at once, x = 0
    t, x, r, o = both("zero rhs", np.zeros(D, np.float32), 50, 1e-6)
    assert (t.iterations, t.converged) == (0, True)
    assert np.array_equal(x, o["x"]) and np.all(x == 0.0) and np.all(r == 0.0)
    # rhs on constrained DOFs only: x takes the prescribed values, no free row is loaded
    if ref.fixed.any():
        bc = np.where(ref.fixed, rng.uniform(-1e-3, 1e-3, D), 0.0).astype(np.float32)
        t, x, r, o = both("constrained rhs", bc, 50, 1e-6)
        assert (t.iterations, t.converged) == (0, True)
        assert np.array_equal(x, o["x"]) and np.array_equal(x, bc) and np.all(r == 0.0)
    # tol = 0.99: the first iteration's test decides
    t, x, r, o = both("tol 0.99", b, 50, 0.99)
    assert t.iterations >= 1
    # a warm start from a converged x: no iteration, x untouched bit for bit. The start is converged to 1e-6 in the
    # recurrence residual; the restart forms b - K x afresh, whose fp32 rounding noise is tens of 1e-6 |b|
    # (tests/helpers.py), so it is asked for 1e-3
    t0, x0, _ = solve(s, b, 2000, 1e-6)
    assert t0.converged
    t, x, r, o = both("warm start, converged", b, 50, 1e-3, x0)
    assert (t.iterations, t.converged) == (0, True)
    assert np.array_equal(x.view(np.uint32), x0.view(np.uint32))
    # a warm start with max_iterations = 1, from the third iterate
    _, x3, _ = solve(s, b, 3, 1e-30)
    t, x, r, o = both("warm start, one iteration", b, 1, 1e-30, x3)
    assert (t.iterations, t.converged) == (1, False)
    # the same step from the same start: FAST's solution contract against the oracle (1e-4 relative)
    assert np.linalg.norm(x.astype(np.float64) - o["x"]) <= 1e-4 * np.linalg.norm(o["x"].astype(np.float64))
    s.close()


# ---- slab shards on one GPU (LOCAL communicator) ---------------------------------------------------------------------
SLAB_SHAPE = (10, 6, 12)  # 13 node planes of 11 x 7 nodes
SLAB_PLANES = {"two-slabs": [0, 6, 13], "three-slabs": [0, 4, 8, 13], "one-plane-slab": [0, 6, 7, 13]}
CASES["10x6x12"] = lambda: scenarios.block_case(*SLAB_SHAPE, h=0.1)


@pytest.mark.parametrize("kind", ["static", "random"])
@pytest.mark.parametrize("cut", list(SLAB_PLANES))
def test_slab_shards_satisfy_the_recurrence(cut, kind, monkeypatch):
    """The recurrence identity on the gathered iterates of a block cut into slabs of node planes (the last case with a
    rank that owns one plane only), driven through shard.solve_pcg_group and compared with the global K_ref: the
    ghost-plane rows and the rank-total folds of the scalars are what this adds to the one-handle cases."""
    from cwf import shard

    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    name = "10x6x12"
    glob, ref = case_of(name), reference(name)
    P = glob.packing
    sK, sM = glob.scalars()
    b = rhs_of(name, kind)
    plane = (SLAB_SHAPE[0] + 1) * (SLAB_SHAPE[1] + 1)
    begin = np.asarray(SLAB_PLANES[cut], np.uint64) * plane
    nranks = begin.size - 1
    comm = shard.Comm.local(nranks)
    systems, shards, rhs = [], [], []
    for r in range(nranks):
        src = pcg.MatrixFreeSystem.from_packing(P, glob.materials, sK, sM, mode=_lib.MODE_FAST)
        sh = shard.build_shard(src, begin, r)
        s = sh.system(glob.materials, sK, sM)
        comm.attach(s, sh)
        systems.append(s)
        shards.append(sh)
        rhs.append(sh.local_dofs(b))
    kerns = [(_lib.load().cwf_hip_system_keff_kernel(s.handle()) or b"").decode() for s in systems]
    c_v = max(CAPS[family_of(k)][1] for k in kerns)
    xs, rs = [np.zeros(ref.D)], [b.astype(np.float64)]
    for j in range(1, STEPS + 1):
        xl = [np.zeros(3 * sh.local_nodes, np.float32) for sh in shards]
        rl = [np.zeros(3 * sh.local_nodes, np.float32) for sh in shards]
        t = shard.solve_pcg_group(systems, rhs, pcg.PcgSettings(j, 1e-30), xl, residuals=rl).value()
        assert t.iterations == j and not t.converged
        x, r = np.zeros((ref.N, 3)), np.zeros((ref.N, 3))
        for sh, xv, rv in zip(shards, xl, rl):
            g = sh.node_global[: sh.owned_nodes].astype(np.int64)
            x[g], r[g] = xv.reshape(-1, 3)[: sh.owned_nodes], rv.reshape(-1, 3)[: sh.owned_nodes]
        xs.append(x.reshape(-1))
        rs.append(r.reshape(-1))
    comm.close()
    xs, rs = np.stack(xs), np.stack(rs)
    rec, op1 = recurrence(ref, xs, rs, c_v)
    eta = etas(ref, xs, rs)
    _, _, eta_ref = reference_iterates(name, kind)
    print(f"{cut} {kind}: {kerns}  recurrence / bound per j {np.array2string(rec[1:], precision=3)} (c_v {c_v:g}; the "
          f"operator's share at j = 1: {op1:.2f} u A|d|)  eta_j {np.array2string(eta[2:], precision=2)}  oracle eta_j "
          f"{np.array2string(eta_ref[2:], precision=2)}")
    assert np.all(xs[1:, ref.fixed] == b.astype(np.float64)[ref.fixed]) and np.all(rs[1:, ref.fixed] == 0.0)
    assert np.all(rec[1:] <= 1.0), rec
    for j in range(2, STEPS + 1):
        assert eta[j] <= max(64 * U, 8 * eta_ref[j]), (j, eta[j], eta_ref[j])
