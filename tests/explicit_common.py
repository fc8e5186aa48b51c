"""The bottom of the explicit-stepper tests' imports (cwf, numpy and helpers only; the other *_common modules and the
test files import from here, never the other way round): the one numpy restatement of the step of include/cwf_hip.h
that the GPU is compared with bit for bit -- the scalar update, the dashpot rows, the tie groups' rows and a correction
force -- and the fixtures the family shares: the operator kinds, damping variants and checkpoints, the cached blocks,
handles, a seeded state, the load of a step, a stepper checked against the restatement, and the scenario runner."""
import collections
import ctypes as C
import functools
import math
import os
import re
import subprocess
import sys
from dataclasses import replace

import numpy as np
import pytest

from cwf import _lib, meshgen, pack, pcg, scenarios
from cwf.explicit import ExplicitStepper
from cwf.physics import RayleighCoefficients, compute_lame, evaluate_curve
from helpers import assert_bitwise

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(ROOT, "tests", "golden", "data", "cantilever.yaml")
U, V, F, PF = (ExplicitStepper.DISPLACEMENT, ExplicitStepper.VELOCITY, ExplicitStepper.EXTERNAL_FORCE,
               ExplicitStepper.PLASTIC_FORCE)
DOF_BITS = np.array([1, 2, 4], np.uint32)
KINDS = {
    "parity": dict(mode=_lib.MODE_PARITY),
    "lattice": dict(mode=_lib.MODE_FAST),
    "groups": dict(mode=_lib.MODE_FAST, jitter=True),
    "hex8": dict(mode=_lib.MODE_FAST, element="hex8"),
}
VARIANTS = {
    "undamped": dict(alpha=0.0, beta=0.0),
    "damped": dict(alpha=5.0, beta=2e-5),
    "curve_bc_state": dict(alpha=0.0, beta=0.0, curve=True),
}
CHECKPOINTS = (1, 2, 3, 53)  # advance(1) three times, then 50 more in one call


# ---- the step -------------------------------------------------------------------------------------------------------
Step = collections.namedtuple("Step", "n u v y f p un vn")


def dashpot_rows(P, Q, V, G):
    """The header's matrix rows in its association order: V, G [n,3] float64 -> v_new [n,3] float64."""
    out = np.empty_like(V)
    for k in range(3):
        out[:, k] = ((P[:, k, 0] * V[:, 0] + P[:, k, 1] * V[:, 1]) + P[:, k, 2] * V[:, 2]) + \
                    ((Q[:, k, 0] * G[:, 0] + Q[:, k, 1] * G[:, 1]) + Q[:, k, 2] * G[:, 2])
    return out


def gather_sum(terms):
    """The header's sum of a group's terms [c, 3] float64, a function of c alone."""
    terms = np.asarray(terms, np.float64)
    c = terms.shape[0]
    if c <= 8:
        acc = np.zeros(3)
        for j in range(c):
            acc = acc + terms[j]
        return acc
    L = np.zeros((64, 3))
    for b in range(0, c, 64):
        chunk = terms[b:b + 64]
        L[:chunk.shape[0]] = L[:chunk.shape[0]] + chunk
    s = 32
    while s >= 1:
        L[:s] = L[:s] + L[s:2 * s]
        s //= 2
    return L[0].copy()


def scheme_steps(apply, mass, fixed, bcv, force_at, alpha, beta, dt, u0, v0, first_step, steps, dash=None, tie=None,
                 p_at=None):
    """The header's scheme, steps first_step .. first_step + steps - 1, one at a time: float32 state, float64 math,
    rounded where stored. Yields a Step for the update that takes the step count from n to n + 1 -- u_n, v_(n-1/2),
    y = K w, f_n, the correction force p (None without p_at) and the stored u_(n+1), v_(n+1/2); float32 each.
    apply(w) -> y (float32); force_at(n) -> f_n (float32); p_at(n, u_n) -> p (float32), called before the operator
    (plasticity's Restatement plugs in as lambda n, u: R.step(u)); dash = (node ids, P, Q [n,3,3]) of the dashpot
    nodes; tie = (groups [index arrays], M_G, P_G, Q_G) of ties_common.group_records. Nodes without a dashpot take the
    scalar expression, dashpot nodes the matrix rows (a tied one's are overwritten by its group's); then the mask."""
    u, v = u0.astype(np.float32), v0.astype(np.float32)
    half = alpha * dt / 2.0
    c1, c2 = (1.0 - half) / (1.0 + half), dt / (1.0 + half)
    m = mass.astype(np.float64)
    for n in range(first_step, first_step + steps):
        p = p_at(n, u) if p_at is not None else None
        w = (u.astype(np.float64) + beta * v.astype(np.float64)).astype(np.float32) if beta != 0.0 else u
        y = apply(w)
        f = force_at(n)
        net = f.astype(np.float64) - y.astype(np.float64)
        if p is not None:
            net = net + p.astype(np.float64)
        g = net / m
        v64 = v.astype(np.float64).reshape(-1, 3)
        vn = (c1 * v.astype(np.float64) + c2 * g).astype(np.float32)
        if dash is not None and len(dash[0]):
            ids, P, Q = dash
            vn.reshape(-1, 3)[ids] = dashpot_rows(P, Q, v64[ids], g.reshape(-1, 3)[ids]).astype(np.float32)
        if tie is not None:
            groups, MG, PG, QG = tie
            terms = np.where(fixed, 0.0, net).reshape(-1, 3)  # a constrained component adds nothing
            for k, members in enumerate(groups):
                gG = gather_sum(terms[members]) / MG[k]
                c = len(members)
                rows = dashpot_rows(np.broadcast_to(PG[k], (c, 3, 3)), np.broadcast_to(QG[k], (c, 3, 3)),
                                    v64[members], np.broadcast_to(gG, (c, 3)))
                vn.reshape(-1, 3)[members] = rows.astype(np.float32)
        un = (u.astype(np.float64) + dt * vn.astype(np.float64)).astype(np.float32)
        un[fixed] = bcv[fixed]
        vn[fixed] = 0.0
        yield Step(n, u, v, y, f, p, un, vn)
        u, v = un, vn


def host_scheme(apply, mass, fixed, bcv, force_at, alpha, beta, dt, u0, v0, first_step, steps, dash=None, tie=None,
                p_at=None, with_p=False):
    """scheme_steps run to its end -> (u, v) after `steps` steps; with_p: (u, v, p of the last step)."""
    u, v, p = u0.astype(np.float32), v0.astype(np.float32), np.zeros(u0.size, np.float32)
    for s in scheme_steps(apply, mass, fixed, bcv, force_at, alpha, beta, dt, u0, v0, first_step, steps, dash, tie,
                          p_at):
        u, v, p = s.un, s.vn, (p if s.p is None else s.p)
    return (u, v, p) if with_p else (u, v)


# ---- meshes, handles, inputs ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mesh_case(jitter=False, element="tet4", harmonic=None):
    """The 4 x 3 x 3-cell block (80 nodes, 216 tets); shared: a user copies what it modifies."""
    return scenarios.block_case(4, 3, 3, h=0.25, jitter=jitter, element=element, harmonic=harmonic)


@functools.lru_cache(maxsize=None)
def big_case():
    """392 nodes: two workgroups of the update pass and a tail."""
    return scenarios.block_case(7, 6, 6)


def case_of(kind, harmonic=None):
    k = KINDS[kind]
    return mesh_case(k.get("jitter", False), k.get("element", "tet4"), harmonic)


def constrained(P):
    return (np.repeat(P.bc_mask, 3) & np.tile(DOF_BITS, P.node_count)) != 0


def group(case, name):
    return case.mesh.node_groups[case.mesh.group_names[name]].astype(np.int64)


def new_system(case, kind, scalars=(1.0, 0.0), kinds=KINDS):
    return pcg.MatrixFreeSystem.from_packing(case.packing, case.materials, scalars[0], scalars[1],
                                             mode=kinds[kind]["mode"])


def applier(system, D):
    """apply(w) -> y = K w by cwf_hip_apply_keff on `system`."""
    def apply(w):
        y = np.zeros(D, np.float32)
        r = pcg.apply_keff(system, np.ascontiguousarray(w, np.float32), y)
        assert r.has_value(), r.error()
        return y

    return apply


def advance(st, n):
    r = st.advance(n)
    assert r.has_value(), r.error()
    assert r.value().finite
    return r.value()


def with_bc(P, bcv):
    return replace(P, bc_value=bcv)


def random_spd(rng, mass32, dt):
    """Full symmetric positive-definite matrices of the size m / dt, where B = C dt / (2 m) is of order one."""
    G = rng.standard_normal((len(mass32), 3, 3))
    Cn = G @ G.transpose(0, 2, 1) + 0.5 * np.eye(3)
    Cn = 0.5 * (Cn + Cn.transpose(0, 2, 1))
    return Cn * (mass32.astype(np.float64) / dt)[:, None, None]


def seeded_state(P, fixed, rng=None):
    """-> (bcv, u0, v0): the packing's constraint values and a state at rest; with rng (variant curve_bc_state)
    non-zero constraint values and a random state that meets them, u0 drawn before v0."""
    D = P.dof_count
    bcv = P.bc_value.copy()
    u0, v0 = np.zeros(D, np.float32), np.zeros(D, np.float32)
    if rng is not None:
        bcv[fixed] = np.float32(1e-4)
        u0 = (1e-6 * rng.standard_normal(D)).astype(np.float32)
        v0 = (1e-3 * rng.standard_normal(D)).astype(np.float32)
        u0[fixed] = bcv[fixed]
        v0[fixed] = 0.0
    return bcv, u0, v0


def constant_force(P):
    f = P.external_force.copy()
    return lambda n: f


def curve_force(base, pattern, curve, dt, value=evaluate_curve):
    """force_at of a load pattern: f_n = f32(base + c(n dt) pattern), c by `value` (the packer's evaluation, or the
    stepper's explicit.curve_value)."""
    return lambda n: pack._safe_f32(base + value(curve, n * dt) * pattern)


def deviation(a, ref):
    return float(np.abs(np.asarray(a, np.float64) - ref).max() / np.abs(ref).max())


# ---- a stepper against the restatement ------------------------------------------------------------------------------
class SchemeRun:
    """One case of "the stepper is the scheme": the seeded constraints and state of a variant, a stepper on a handle
    that carries a Newmark step's scalars (the stepper runs the operator at (1, 0) regardless), a second handle at
    (1, 0) for the restatement's y, and the comparison at checkpoints. The caller attaches what it tests between the
    construction and load()."""

    def __init__(self, case, kind, variant, seed=7):
        self.case, self.P = case, case.packing
        self.alpha, self.beta = VARIANTS[variant]["alpha"], VARIANTS[variant]["beta"]
        self.curve = VARIANTS[variant].get("curve", False)
        self.fixed = constrained(self.P)
        self.mass = np.repeat(self.P.lumped_mass, 3)
        self.rng = np.random.Generator(np.random.PCG64(seed))
        self.bcv, self.u0, self.v0 = seeded_state(self.P, self.fixed, self.rng if self.curve else None)
        self.sys_a = new_system(case, kind, case.scalars())
        self.sys_b = new_system(case, kind, (1.0, 0.0))
        self.st = ExplicitStepper(with_bc(self.P, self.bcv) if self.curve else self.P, case.materials,
                                  RayleighCoefficients(self.alpha, self.beta), system=self.sys_a)
        self.dt = self.st.telemetry().dt
        self.apply = applier(self.sys_b, self.P.dof_count)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.st.close()
        self.sys_a.close()
        self.sys_b.close()

    def load(self):
        """The variant's load and state on the stepper, and force_at: the packed force, or (curve_bc_state) the
        case's pattern and curve with the seeded state."""
        if self.curve:
            base, pattern = self.case.load_pattern()
            _, c = self.case.load_curve
            self.st.set_load_pattern(base, pattern)
            self.st.set_load_curve(c)
            self.st.set_state(U, self.u0)
            self.st.set_state(V, self.v0)
            self.force_at = curve_force(base, pattern, c, self.dt)
        else:
            self.force_at = constant_force(self.P)

    def host(self, u, v, first_step, steps, dash=None, tie=None):
        return host_scheme(self.apply, self.mass, self.fixed, self.bcv, self.force_at, self.alpha, self.beta, self.dt,
                           u, v, first_step, steps, dash, tie)

    def check(self, checkpoints, what, dash=None, tie=None, each=None):
        """advance to every checkpoint against the restatement, u and v bitwise -> the restatement's last (u, v)."""
        u, v, done = self.u0, self.v0, 0
        for upto in checkpoints:
            r = self.st.advance(upto - done)
            assert r.has_value(), r.error()
            t = r.value()
            assert t.steps == upto and t.time == upto * self.dt and t.finite
            u, v = self.host(u, v, done, upto - done, dash, tie)
            done = upto
            assert_bitwise(self.st.get_state(U), u, f"{what} after {upto} steps: u")
            assert_bitwise(self.st.get_state(V), v, f"{what} after {upto} steps: v")
            if each is not None:
                each(f"{what} after {upto} steps")
        assert np.abs(u[~self.fixed]).max() > 0.0 and np.abs(v[~self.fixed]).max() > 0.0
        return u, v

    def check_mask_wins(self, ids):
        """Constrained components of the nodes `ids` (dashpot or tied nodes): u is the constraint's value, v is 0."""
        held = self.fixed.reshape(-1, 3)[ids]
        assert np.array_equal(self.st.get_state(U).reshape(-1, 3)[ids][held], self.bcv.reshape(-1, 3)[ids][held])
        assert np.all(self.st.get_state(V).reshape(-1, 3)[ids][held] == 0.0)


def refused(call, msg, ctx=()):
    """call() raises a RuntimeError whose text holds msg and every context entry of ctx."""
    with pytest.raises(RuntimeError) as e:
        call()
    assert msg in str(e.value) and all(f"'{c}'" in str(e.value) for c in ctx), str(e.value)


def check_ledger(led, ref, what):
    """An EnergyLedger against (steps, rows, bounds) of monitors_common.LedgerReference.arrays() -> its rows [n, 4]."""
    steps, rows, bounds = ref
    assert np.array_equal(led.steps, steps), (what, led.steps, steps)
    got = np.stack([led.kinetic, led.potential, led.work, led.dissipated], axis=1)
    err = np.abs(got - rows)
    worst = float((err / np.maximum(bounds, 1e-300)).max()) if rows.size else 0.0
    print(f"{what}: ledger error / summation bound, worst of {rows.shape[0]} rows x 4 columns: {worst:.3e}")
    assert np.all(err <= bounds), (what, np.argwhere(err > bounds)[:5], err.max())
    return got


# ---- the scenario runner --------------------------------------------------------------------------------------------
def run_cli(args):
    return subprocess.run([sys.executable, "-m", "cwf.run", *args], capture_output=True, text=True, cwd=ROOT,
                          env=dict(os.environ, PYTHONPATH=os.path.join(ROOT, "civiwave-fem_amd")))


def block_scenario(tmp_path, replacements=(), name="block.yaml"):
    """The cantilever scenario on a mesh that has more than its own single tet: its text with another mesh, 216 tets
    held at x = 0 and loaded at the far face, a shorter output interval, and the caller's further (old, new)
    replacements, each of which must meet its text exactly once."""
    tm = meshgen.kuhn_block(4, 3, 3, 0.25)
    x = tm.coords[:, 0]
    tm.node_groups = {"FIXED_BASE": np.nonzero(x == x.min())[0].astype(np.uint32),
                      "LOAD_FACE": np.nonzero(x == x.max())[0].astype(np.uint32)}
    meshgen.write_gmsh(tm, str(tmp_path / "block.msh"), surface_groups=("FIXED_BASE", "LOAD_FACE"))
    text = open(YAML).read()
    for old, new in (("path: tests/data/cantilever.msh", "path: block.msh"), ("dt: 0.01111", "dt: 0.001"),
                     *replacements):
        assert text.count(old) == 1, old
        text = text.replace(old, new)
    y = tmp_path / name
    y.write_text(text)
    return str(y)


# ---- host side: the header's structs, and what the absorbing and the source tests share -----------------------------
def header_struct_size(name):
    """sizeof of `typedef struct name { ... } name;` in the header, every member naturally aligned in declaration
    order (no padding)."""
    text = open(_lib.HEADER_PATH).read()
    m = re.search(r"typedef struct " + name + r"\s*\{(.*?)\}\s*" + name + ";", text, re.S)
    assert m, name
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    size = {"double": 8, "uint64_t": 8, "uint32_t": 4, "int32_t": 4}
    total = 0
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        names = decl.split(",")
        if "*" in decl:
            total += 8 * len(names)
            continue
        total += size[decl.split()[0]] * len(names)
    return total


H = 0.25
BASE_YAML = open(YAML).read()
ABSORBING = """absorbing:
  - group: BASE
    incident: {direction: [1, 0, 0.5], velocity_curve: load_curve1}
  - group: SIDES
"""


def speeds(mat):
    """(rho, V_p, V_s) of a material."""
    l = compute_lame(mat.youngs_modulus, mat.poisson_ratio)
    return mat.density, math.sqrt((l.lambda_ + 2.0 * l.mu) / mat.density), math.sqrt(l.mu / mat.density)


def face_geometry(X, face):
    """(area, unit normal) of a triangle or of a quad as its triangles (0,1,2) + (0,2,3)."""
    p = X[np.asarray(face, np.int64)]
    c1 = np.cross(p[1] - p[0], p[2] - p[0])
    area, s = 0.5 * np.linalg.norm(c1), c1
    if len(face) == 4:
        c2 = np.cross(p[2] - p[0], p[3] - p[0])
        area, s = area + 0.5 * np.linalg.norm(c2), c1 + c2
    return area, s / np.linalg.norm(s)


def raw_json(text):
    """cwf_config_json of a scenario text."""
    L = _lib.load()
    h = C.c_void_p()
    assert L.cwf_config_load_string(text.encode(), C.byref(h)) == 0, _lib.last_error(None)
    try:
        return L.cwf_config_json(h).decode()
    finally:
        L.cwf_config_destroy(h)
