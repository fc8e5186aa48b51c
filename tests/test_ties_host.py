"""Tied boundaries on the host (no GPU): the three tie-set helpers of csrc/ties.cpp through cwf.ties, the index tables
of csrc/ties_tables.cpp through their C++ test program (against its own cases, against a numpy restatement, and
stand-alone under the host sanitizers), the scenario's ``tied:`` block (every validation message with its
breadcrumb, the serialisation of a document without it, the driver's merge), the restatement's accuracy against the
all-fp64 reduced dense system, and the largest eigenvalue of the reduced system against the full one."""
import dataclasses
import os
import subprocess

import numpy as np
import pytest

import absorbing_common as ac
import explicit_common as xc
import ties_common as tc
from cwf import ties

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "civiwave-fem_amd", "csrc")
TEST_CPP = os.path.join(ROOT, "tests", "cpp", "ties_tables_test.cpp")

# ties_common.column_reference measured ("Tied boundaries"): the float32 restatement against the
# all-fp64 reduced dense run at the run's end, max |delta| / max |reference|
FLOOR_U, FLOOR_V = 6.01e-7, 2.50e-2


def faces(X):
    lo, hi = X.min(0), X.max(0)
    return {(a, e): np.nonzero(X[:, a] == (lo, hi)[e][a])[0] for a in (0, 1) for e in (0, 1)}


def periodic_ties(X):
    f = faces(X)
    return ties.merge(X.shape[0], ties.periodic(X, f[0, 0], f[0, 1], 0), ties.periodic(X, f[1, 0], f[1, 1], 1))


# ---- the helpers ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("jitter", [False, True])
def test_levels_periodic_and_merge_on_the_block(jitter):
    case = tc.tie_case(jitter=jitter)
    X = case.mesh.coords
    N = X.shape[0]
    side = tc.perimeter(X)
    off, ids = ties.levels(X, side[::-1], 2)  # the caller's order does not matter
    groups = ties.groups_of(off, ids)
    assert [len(g) for g in groups] == [14, 14, 14, 14]
    for k, g in enumerate(groups):  # ascending in z, members ascending
        assert np.all(X[g, 2] == 0.25 * k) and np.all(np.diff(g.astype(np.int64)) > 0)
    assert np.array_equal(np.sort(ids), side)
    f = faces(X)
    for axis in (0, 1):
        po, pi = ties.periodic(X, f[axis, 0], f[axis, 1], axis)
        pairs = pi.reshape(-1, 2)
        assert np.array_equal(po, 2 * np.arange(pairs.shape[0] + 1)) and np.array_equal(pairs[:, 0], f[axis, 0])
        other = [k for k in range(3) if k != axis]
        assert np.array_equal(X[pairs[:, 0]][:, other], X[pairs[:, 1]][:, other])
        assert np.all(X[pairs[:, 1], axis] == X[:, axis].max())
    mo, mi = periodic_ties(X)
    merged = ties.groups_of(mo, mi)
    sizes = np.array([len(g) for g in merged])
    assert np.count_nonzero(sizes == 4) == 4 and np.count_nonzero(sizes == 2) == 4 * (3 + 2) and sizes.size == 24
    assert np.unique(mi).size == mi.size == side.size  # disjoint, and every perimeter node once
    firsts = [int(g[0]) for g in merged]
    assert firsts == sorted(firsts) and all(np.all(np.diff(g.astype(np.int64)) > 0) for g in merged)
    for g in (g for g in merged if len(g) == 4):
        assert np.unique(X[g, 2]).size == 1 and np.unique(X[g][:, :2], axis=0).shape[0] == 4  # the four vertical edges
    # a level with one node is dropped; an empty list gives no group
    assert ties.levels(X, [side[0]], 2)[0].tolist() == [0]
    assert ties.levels(X, [], 2)[0].tolist() == [0]
    assert ties.merge(N)[0].tolist() == [0]


def test_tolerance_is_relative_to_the_extent():
    case = tc.tie_case()
    X = case.mesh.coords.copy()
    side = tc.perimeter(X)
    top = side[X[side, 2] == X[:, 2].max()]
    X[top[::2], 2] += 1e-6 * 0.75  # 1e-6 of the extent along z
    assert [len(g) for g in ties.groups_of(*ties.levels(X, side, 2))] == [14, 14, 14, 7, 7]  # 0 means 1e-9
    assert [len(g) for g in ties.groups_of(*ties.levels(X, side, 2, 1e-5))] == [14, 14, 14, 14]
    assert [len(g) for g in ties.groups_of(*ties.levels(X, side, 2, 1e-7))] == [14, 14, 14, 7, 7]
    f = faces(case.mesh.coords)
    Y = case.mesh.coords.copy()
    Y[f[0, 1][3], 1] += 1e-6 * 0.75
    with pytest.raises(ValueError, match="periodic faces do not match"):
        ties.periodic(Y, f[0, 0], f[0, 1], 0)
    assert ties.periodic(Y, f[0, 0], f[0, 1], 0, 1e-5)[1].size == 2 * f[0, 0].size


def test_helper_refusals():
    case = tc.tie_case()
    X = case.mesh.coords
    N = X.shape[0]
    f = faces(X)
    inside = int(np.nonzero((X[:, 0] == 0.25) & (X[:, 1] == 0.25) & (X[:, 2] == 0.25))[0][0])
    for call, msg, ctx in (
            (lambda: ties.levels(X, [0, 1, N], 2), "tied node out of range", ["index=2", f"node={N}"]),
            (lambda: ties.levels(X, [0, 1, 0], 2), "tied node listed twice", ["index=2", "node=0"]),
            (lambda: ties.levels(X, [0, 1], 3), "tie axis must be 0, 1 or 2", ["axis=3"]),
            (lambda: ties.levels(X, [0, 1], 2, -1.0), "tie tolerance must be finite and not negative", []),
            (lambda: ties.periodic(X, f[0, 0], f[0, 1][:-1], 0), "periodic faces do not match",
             [f"node={f[0, 0][-1]}", "face=A"]),
            (lambda: ties.periodic(X, f[0, 0][:-1], f[0, 1], 0), "periodic faces do not match",
             [f"node={f[0, 1][-1]}", "face=B"]),
            (lambda: ties.periodic(X, f[0, 0], np.append(f[0, 1][1:], inside), 0), "periodic faces do not match",
             [f"node={f[0, 0][0]}", "face=A"]),
            (lambda: ties.periodic(X, f[0, 0], f[0, 0], 0), "tied node listed twice", ["face=B", "index=0"]),
            (lambda: ties.merge(N, (np.array([0, 2]), np.array([0, N]))), "tied node out of range", ["index=1"]),
            (lambda: ties.merge(N, (np.array([0, 2, 1]), np.array([0, 1]))), "tie offsets must ascend from 0",
             ["group=1"])):
        with pytest.raises(ValueError) as e:
            call()
        assert msg in str(e.value) and all(f"'{c}'" in str(e.value) for c in ctx), str(e.value)
    # merge: groups that share nodes become one; a group of one node is dropped
    off, ids = ties.merge(N, (np.array([0, 2, 4, 5]), np.array([7, 3, 9, 7, 11])), (np.array([0, 2]), np.array([20, 9])))
    assert [g.tolist() for g in ties.groups_of(off, ids)] == [[3, 7, 9, 20]]


# ---- the tables -----------------------------------------------------------------------------------------------------
def build(tmp_path, name, extra, flags=()):
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-ffp-contract=off", *flags, "-I" + CSRC, TEST_CPP, *extra,
                    "-o", exe], check=True)
    return exe


def numpy_tables(N, dash, off, ids, perm):
    """ties_tables.hpp restated: the dashpot nodes' slots first, then the other tied nodes in list order; the CSR's
    members are the internal places of the listed nodes."""
    slot = np.full(max(N, 4), 0xFFFFFFFF, np.uint64)
    slot[dash] = np.arange(len(dash))
    node, group = list(dash), [0xFFFFFFFF] * len(dash)
    for g in range(len(off) - 1):
        for n in ids[off[g]:off[g + 1]]:
            if slot[n] == 0xFFFFFFFF:
                slot[n] = len(node)
                node.append(n)
                group.append(0xFFFFFFFF)
            group[int(slot[n])] = g
    place = np.empty(N, np.int64)
    place[perm] = np.arange(N)
    return dict(slot=slot.tolist(), node=node, group=group, toff=list(off), tnode=place[ids].tolist())


def test_tables_program_against_the_library_and_numpy(tmp_path):
    libdir = os.path.join(ROOT, "civiwave-fem_amd", "lib")
    exe = build(tmp_path, "ties_tables_test", [f"-L{libdir}", "-lcwf_hip", f"-Wl,-rpath,{libdir}"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout, out.stderr)
    # the block's level ties with dashpots on the base, through a random node order
    case = tc.tie_case()
    N = case.packing.node_count
    rng = np.random.Generator(np.random.PCG64(4))
    off, ids = ties.levels(case.mesh.coords, tc.perimeter(case.mesh.coords), 2)
    ids = rng.permutation(ids[:14]).tolist() + ids[14:].tolist()
    dash = rng.permutation(xc.group(case, "BASE")).tolist()
    perm = rng.permutation(N).tolist()
    path = tmp_path / "set.txt"
    path.write_text("\n".join([str(N)] + [" ".join(map(str, [len(v)] + list(v))) for v in (dash, off.tolist(), ids, perm)]))
    out = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout, out.stderr)
    got = {l.split()[0]: [int(x) for x in l.split()[1:]] for l in out.stdout.strip().splitlines()}
    want = numpy_tables(N, dash, [int(x) for x in off], ids, np.array(perm))
    assert got == want
    assert len(got["node"]) == 20 + 42 and got["group"].count(0) == 14  # 6 untied dashpot nodes, 42 tied without one


def test_tables_program_stand_alone_with_host_sanitizers(tmp_path):
    exe = build(tmp_path, "ties_tables_test_san", [os.path.join(CSRC, "ties_tables.cpp")],
                ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                 "-static-libubsan"])
    out = subprocess.run([exe], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"), capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout, out.stderr)


# ---- the restatement ------------------------------------------------------------------------------------------------
def test_gather_sum_orders():
    """The header's two orders on terms whose sum depends on the order: up to 8 members the list order, beyond that
    the 64 lane sums and their pairwise fold."""
    big = np.array([1e16, 1.0, -1e16, 1.0, 1.0, 1.0, 1.0, 1.0])
    t = np.stack([big, big[::-1], np.ones(8)], 1)
    back = 0.0
    for x in big[::-1]:
        back = back + float(x)
    assert xc.gather_sum(t).tolist() == [5.0, back, 8.0] and back != 5.0  # ((1e16 + 1) - 1e16) + 5 ones in list order
    # nine members: lane sums first (every member its own lane), then strides 32 .. 1: lanes 0 and 8 meet at stride 8,
    # ((t0 + t8) + t4) + (t2 + t6) meets ((t1 + t5) + (t3 + t7)) at stride 1
    t9 = np.array([1e16, 1.0, -1e16, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0])
    t = np.stack([t9, np.arange(9.0), np.ones(9)], 1)
    want = (((t9[0] + t9[8]) + t9[4]) + (t9[2] + t9[6])) + ((t9[1] + t9[5]) + (t9[3] + t9[7]))
    assert xc.gather_sum(t).tolist() == [want, 36.0, 9.0] and want != 7.0
    # 130 members: lane l holds t_l + t_(l + 64) (+ t_(l + 128) for l < 2)
    rng = np.random.Generator(np.random.PCG64(1))
    t = rng.standard_normal((130, 3)) * 10.0 ** rng.integers(-8, 8, (130, 1))
    L = t[:64] + t[64:128]
    L[:2] = L[:2] + t[128:]
    for s in (32, 16, 8, 4, 2, 1):
        L = L[:s] + L[s:2 * s]
    assert np.array_equal(xc.gather_sum(t), L[0])


def test_restatement_against_the_fp64_reduced_system():
    """Measured: u 6.01e-7, v 2.50e-2 at the end of the 320-step run (v has all but left by then: its reference is
    1.4e-3 of the peak). Asserted at 8 x the measured value, the margin of an f32-storage floor elsewhere."""
    R = tc.column_reference()
    print(f"tied column, fp64 reduced run: {R['conditions']}; untied control spread / peak {R['control_spread']:.3e}; "
          f"restatement against it at the end: u {R['floor_u']:.3e} v {R['floor_v']:.3e}")
    R["assert_conditions"]()
    assert R["control_spread"] > 1e-3  # the untied, unheld column does not keep its planes together
    assert 0.0 < R["floor_u"] <= 8.0 * FLOOR_U and 0.0 < R["floor_v"] <= 8.0 * FLOOR_V
    # the restatement keeps every plane together, bit for bit
    for g in R["groups"]:
        for a in (R["u32"], R["v32"]):
            rows = a.reshape(-1, 3)[g].view(np.uint32)
            assert np.all(rows == rows[0])


@pytest.mark.parametrize("which", ["levels", "periodic"])
def test_tied_lambda_max_does_not_exceed_the_untied(which):
    case = tc.tie_case()
    ref = ac.dense_of(case)
    X = case.mesh.coords
    off, ids = ties.levels(X, tc.perimeter(X), 2) if which == "levels" else periodic_ties(X)
    red = tc.reduced_system(ref["K"], ref["mass"], ref["fixed"], ties.groups_of(off, ids))
    lam = tc.lam_max(red["K"], red["mass"], red["fixed"])
    print(f"{which}: lambda_max reduced {lam:.6e}, full {ref['lam_max']:.6e}, ratio {lam / ref['lam_max']:.4f}")
    assert 0.0 < lam <= ref["lam_max"] * (1.0 + 1e-12)


# ---- the scenario's ``tied:`` block ---------------------------------------------------------------------------------
GOLDEN_YAML = os.path.join(ROOT, "tests", "golden", "data", "cantilever.yaml")
GOLDEN_JSON = os.path.join(ROOT, "tests", "golden", "cantilever_config.json")  # the parser's output before the key
TIED = "tied:\n  - group: SIDE\n    axis: 2\n  - pair: [XLO, XHI]\n    axis: 0\n"


def _json_of(text):
    import ctypes as C

    from cwf import _lib

    L = _lib.load()
    h = C.c_void_p()
    assert L.cwf_config_load_string(text.encode(), C.byref(h)) == 0, _lib.last_error(None)
    try:
        return L.cwf_config_json(h).decode()
    finally:
        L.cwf_config_destroy(h)


def test_config_takes_the_tied_block_and_keeps_documents_without_it():
    from cwf import config
    from cwf.physics import TiedBoundary

    base = open(GOLDEN_YAML).read()
    # a document without the key serialises byte for byte to what it did before the key existed
    assert _json_of(base) == open(GOLDEN_JSON).read()
    assert config.load_config_from_string(base).value().tied == []
    r = config.load_config_from_string(base + "\n" + TIED)
    assert r.has_value(), r.error()
    assert r.value().tied == [TiedBoundary(2, "SIDE", None), TiedBoundary(0, None, ("XLO", "XHI"))]
    # the key sits at the document's end; removing it gives the golden text back
    text = _json_of(base + "\n" + TIED)
    block = ', "tied": [{"group": "SIDE", "axis": 2}, {"pair": ["XLO", "XHI"], "axis": 0}]'
    assert text.endswith(block + "}") and text.replace(block, "") == open(GOLDEN_JSON).read()
    assert config.load_config_from_string(base + "\ntied: []\n").value().tied == []


@pytest.mark.parametrize("block,message,context", [
    ("tied: 3\n", "tied must be a sequence when present", ["tied"]),
    ("tied:\n  - 3\n", "tied entry must be a map", ["tied", "[0]"]),
    ("tied:\n  - group: A\n    axis: 0\n  - axis: 2\n", "tied entry needs either group or pair", ["tied", "[1]"]),
    ("tied:\n  - group: A\n    pair: [A, B]\n    axis: 1\n", "tied entry needs either group or pair", ["tied", "[0]"]),
    ("tied:\n  - group: A\n    axis: 3\n", "tied.axis must be 0, 1 or 2", ["tied", "[0]", "axis"]),
    ("tied:\n  - group: A\n    axis: -1\n", "tied.axis must be 0, 1 or 2", ["tied", "[0]", "axis"]),
    ("tied:\n  - pair: [A, B]\n", "tied.axis must be 0, 1 or 2", ["tied", "[0]", "axis"]),
    ("tied:\n  - pair: [A]\n    axis: 0\n", "tied.pair must be a sequence of two group names", ["tied", "[0]", "pair"]),
    ("tied:\n  - pair: [A, B, C]\n    axis: 0\n", "tied.pair must be a sequence of two group names", ["tied", "[0]", "pair"]),
    ("tied:\n  - pair: A\n    axis: 0\n", "tied.pair must be a sequence of two group names", ["tied", "[0]", "pair"]),
    ("tied:\n  - group: [A, B]\n    axis: 0\n", "tied.group must be a group name", ["tied", "[0]", "group"]),
])
def test_config_refuses_a_malformed_tied_block(block, message, context):
    from cwf import config

    r = config.load_config_from_string(open(GOLDEN_YAML).read() + "\n" + block)
    assert not r.has_value()
    assert (r.error().message, r.error().context) == (message, context)


def test_driver_merges_the_entries_and_names_an_unknown_group():
    """cwf.run.tied_setup on the block: a group entry and two pair entries become one set; an unknown group and faces
    that do not match are refused with the entry's index."""
    from cwf import run
    from cwf.physics import TiedBoundary

    case = tc.tie_case()
    m, P = case.mesh, case.packing
    X = m.coords
    f = faces(X)
    first = max(m.group_names.values()) + 1
    for k, (name, nodes) in enumerate((("XLO", f[0, 0]), ("XHI", f[0, 1]), ("YLO", f[1, 0]), ("YHI", f[1, 1]))):
        m.group_names[name] = first + k
        m.node_groups[first + k] = nodes.astype(np.uint32)
    try:
        cfg = dataclasses.replace(case.cfg, tied=[TiedBoundary(0, None, ("XLO", "XHI")), TiedBoundary(1, None, ("YLO", "YHI"))])
        off, ids = run.tied_setup(cfg, m, P)
        want = periodic_ties(X)
        assert np.array_equal(off, want[0]) and np.array_equal(ids, want[1])
        cfg = dataclasses.replace(case.cfg, tied=[TiedBoundary(2, "SIDE", None), TiedBoundary(0, None, ("XLO", "XHI"))])
        off, ids = run.tied_setup(cfg, m, P)  # the x pairs lie within the levels: the levels remain
        want = ties.levels(X, tc.perimeter(X), 2)
        assert np.array_equal(off, want[0]) and np.array_equal(ids, want[1])
        for tied, text in (([TiedBoundary(2, "SIDE", None), TiedBoundary(2, "NOWHERE", None)], "tied [1]: unknown group 'NOWHERE'"),
                           ([TiedBoundary(0, None, ("XLO", "NOWHERE"))], "tied [0]: unknown group 'NOWHERE'"),
                           ([TiedBoundary(0, None, ("XLO", "YHI"))], "tied [0]: ties.periodic failed: tied node listed twice")):
            with pytest.raises(run.ScenarioError) as e:
                run.tied_setup(dataclasses.replace(case.cfg, tied=tied), m, P)
            assert text in str(e.value), str(e.value)
    finally:
        for name in ("XLO", "XHI", "YLO", "YHI"):
            m.node_groups.pop(m.group_names.pop(name))
