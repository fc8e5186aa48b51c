"""Absorbing boundaries, host side (no GPU): the exported entry points, cwf_absorbing_dashpots against a numpy
restatement of the share rule (uniform and layered blocks, tet4 and hex8, rotation equivariance, refusals),
cwf_explicit_dashpot_update against numpy.linalg.inv, the incident pattern, and the scenario config's ``absorbing:``
list (dataclasses, error texts with their contexts, byte-identical JSON without the key)."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

from cwf import _lib, absorbing, config, meshgen, pack, scenarios
from cwf.physics import AbsorbingBoundary, IncidentWave
from explicit_common import ABSORBING, BASE_YAML, H, face_geometry, raw_json, speeds

SYMBOLS = {"cwf_hip_explicit_set_dashpots", "cwf_hip_explicit_get_dashpots", "cwf_explicit_dashpot_update",
           "cwf_absorbing_dashpots"}


def test_library_declares_and_exports_the_entry_points():
    L = _lib.load()
    assert SYMBOLS <= set(_lib.declared_symbols())
    for n in SYMBOLS:
        assert hasattr(L, n), n
        assert getattr(L, n).argtypes is not None, n
    assert L.cwf_hip_abi_version() == 1
    assert C.sizeof(_lib.ExplicitDescC) == 56


def share_rule(X, faces, material_of_face):
    """node -> C_n: every face gives each of its k nodes rho (a / k)(V_p nu nu^T + V_s (I - nu nu^T))."""
    out = {}
    for f, face in enumerate(faces):
        area, nu = face_geometry(X, face)
        rho, vp, vs = speeds(material_of_face(f))
        nn = np.outer(nu, nu)
        Cf = rho * (area / len(face)) * (vp * nn + vs * (np.eye(3) - nn))
        for n in face:
            out[int(n)] = out.get(int(n), np.zeros((3, 3))) + Cf
    return out


def check_against_share_rule(mesh, cfg, faces, material_of_face):
    ids, Cn = absorbing.dashpots(mesh, cfg, faces)
    want = share_rule(mesh.coords, faces.tolist(), material_of_face)
    assert ids.dtype == np.uint32 and list(ids) == sorted(want)
    for n, got in zip(ids, Cn):
        ref = want[int(n)]
        assert np.abs(got - ref).max() <= 1e-14 * np.abs(ref).max(), (n, got, ref)
    return ids, Cn


@pytest.mark.parametrize("element", ["tet4", "hex8"])
def test_dashpots_of_the_bottom_face(element):
    case = scenarios.block_case(4, 3, 3, h=H, element=element)
    m, cfg = case.mesh, case.cfg
    bottom = np.nonzero(m.coords[:, 2] == 0.0)[0]
    faces = meshgen.boundary_faces(m.tets, bottom)
    assert faces.shape == ((12, 4) if element == "hex8" else (24, 3))
    ids, Cn = check_against_share_rule(m, cfg, faces, lambda f: cfg.materials[0])
    assert np.array_equal(ids, bottom.astype(np.uint32))
    rho, vp, vs = speeds(cfg.materials[0])
    area = (4 * H) * (3 * H)
    total = Cn.sum(0)
    assert abs(total[2, 2] - rho * vp * area) <= 1e-12 * rho * vp * area
    for k in (0, 1):
        assert abs(total[k, k] - rho * vs * area) <= 1e-12 * rho * vs * area
    off = Cn[:, ~np.eye(3, dtype=bool)]
    assert np.all(off == 0.0)


@pytest.mark.parametrize("element", ["tet4", "hex8"])
def test_side_face_of_a_layered_block_takes_each_stratums_impedance(element):
    layers = [0, 1, 1, 2]
    case = scenarios.layered_case(3, 2, 4, layers, h=H, element=element)
    m, cfg = case.mesh, case.cfg
    side = np.nonzero(m.coords[:, 0] == 0.0)[0]
    faces = meshgen.boundary_faces(m.tets, side)
    zc = m.coords[faces.astype(np.int64)][:, :, 2].mean(1)
    slot = [layers[int(z // H)] for z in zc]
    assert set(slot) == {0, 1, 2}
    ids, Cn = check_against_share_rule(m, cfg, faces, lambda f: scenarios.LAYER_MATERIALS[slot[f]])
    # a node inside stratum 1 (plane 2: cells 1 and 2 both hold m1) against one inside nothing else: the ratio of
    # their C_xx is the ratio of rho V_p only if the strata were read per face
    total = Cn.sum(0)
    want = sum(speeds(scenarios.LAYER_MATERIALS[s])[0] * speeds(scenarios.LAYER_MATERIALS[s])[1] * (2 * H) * H
               for s in layers)
    assert abs(total[0, 0] - want) <= 1e-12 * want


def test_rotation_equivariance_on_a_jittered_permuted_block():
    tm = meshgen.jitter_and_permute(meshgen.kuhn_block(3, 3, 3, H), H)
    mesh = pack.from_tetmesh(tm)
    cfg = scenarios.make_config()
    faces = meshgen.boundary_faces(mesh.tets, np.arange(mesh.node_count))  # the whole boundary: six normals
    assert len(faces) == 6 * 9 * 2
    ids, Cn = absorbing.dashpots(mesh, cfg, faces)
    a, b, c = 0.7, -0.4, 1.1
    Rx = np.array([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]])
    Ry = np.array([[math.cos(b), 0, math.sin(b)], [0, 1, 0], [-math.sin(b), 0, math.cos(b)]])
    Rz = np.array([[math.cos(c), -math.sin(c), 0], [math.sin(c), math.cos(c), 0], [0, 0, 1]])
    R = Rz @ Ry @ Rx
    rot = pack.from_tetmesh(meshgen.TetMesh(tm.coords @ R.T, tm.tets, tm.node_groups))
    ids2, Cn2 = absorbing.dashpots(rot, cfg, faces)
    assert np.array_equal(ids, ids2)
    assert np.abs(Cn2[:, ~np.eye(3, dtype=bool)]).max() > 0.0  # full matrices, not diagonals
    for n, C1, C2 in zip(ids, Cn, Cn2):
        assert np.abs(C2 - R @ C1 @ R.T).max() <= 1e-12 * np.linalg.norm(C1), n


def test_refusals_of_faces():
    case = scenarios.block_case(4, 3, 3, h=H)
    m, cfg = case.mesh, case.cfg
    good = meshgen.boundary_faces(m.tets, np.nonzero(m.coords[:, 2] == 0.0)[0])
    t = m.tets.astype(np.int64)
    allf = np.sort(np.concatenate([t[:, [0, 1, 2]], t[:, [0, 1, 3]], t[:, [0, 2, 3]], t[:, [1, 2, 3]]]), 1)
    uniq, cnt = np.unique(allf, axis=0, return_counts=True)
    interior = uniq[cnt == 2][0].astype(np.uint32)

    def refused(bad, at=2):
        faces = good.copy()
        faces[at] = bad
        with pytest.raises(RuntimeError) as e:
            absorbing.dashpots(m, cfg, faces)
        return str(e.value)

    msg = refused(interior)
    assert "absorbing face is not a boundary face of the mesh" in msg and "'face=2'" in msg
    msg = refused([good[0][0], good[0][0], good[0][1]], at=5)
    assert "absorbing face has zero area" in msg and "'face=5'" in msg
    msg = refused([good[0][0], good[0][1], m.node_count], at=7)
    assert "absorbing face references node out of range" in msg and "'face=7'" in msg \
        and f"'node={m.node_count}'" in msg
    # three collinear nodes: zero area too
    line = np.nonzero((m.coords[:, 1] == 0.0) & (m.coords[:, 2] == 0.0))[0][:3]
    assert "absorbing face has zero area" in refused(line.astype(np.uint32))


def lib_update(Cm, mass, alpha, dt):
    Cm = np.ascontiguousarray(Cm, np.float64)
    P, Q = np.zeros(9), np.zeros(9)
    rc = _lib.load().cwf_explicit_dashpot_update(_lib.ptr(Cm), mass, alpha, dt, _lib.ptr(P), _lib.ptr(Q))
    return rc, P.reshape(3, 3), Q.reshape(3, 3)


@pytest.mark.parametrize("alpha", [0.0, 5.0])
def test_dashpot_update_against_numpy(alpha):
    """Random SPD matrices G G^T + 3 I (condition number below ~10), scaled over six decades around m / dt, where
    B = C dt / (2 m) passes through 1: the closed-form inverse and numpy's agree to a few condition numbers of
    rounding, far inside 1e-13 of the largest entry."""
    rng = np.random.Generator(np.random.PCG64(3))
    mass, dt = 37.5, 4.0e-5
    I = np.eye(3)
    for decade in range(-3, 4):
        for _ in range(8):
            G = rng.standard_normal((3, 3))
            Cm = (G @ G.T + 3.0 * I) * (10.0 ** decade) * mass / dt
            rc, P, Q = lib_update(Cm, mass, alpha, dt)
            assert rc == 0
            h, B = alpha * dt / 2.0, Cm * dt / (2.0 * mass)
            A = np.linalg.inv((1.0 + h) * I + B)
            for got, want in ((P, A @ ((1.0 - h) * I - B)), (Q, dt * A)):
                assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max(), (decade, got, want)
    rc, P, Q = lib_update(np.zeros((3, 3)), mass, alpha, dt)
    h = alpha * dt / 2.0
    # C = 0: the scalar scheme's c1 I and c2 I, up to the rounding of the inverse's products
    assert rc == 0 and np.abs(P - I * ((1.0 - h) / (1.0 + h))).max() <= 4e-16
    assert np.abs(Q - I * (dt / (1.0 + h))).max() <= 4e-16 * dt


def test_dashpot_update_refusals():
    L = _lib.load()
    good = np.array([[4.0, 1.0, 0.5], [1.0, 3.0, 0.2], [0.5, 0.2, 2.0]])
    assert lib_update(good, 2.0, 0.0, 1e-3)[0] == 0
    asym = good.copy()
    asym[0, 1] += 1e-9
    assert lib_update(asym, 2.0, 0.0, 1e-3)[0] == -11
    assert L.cwf_hip_last_error(None).decode() == "dashpot matrix is not symmetric"
    within = good.copy()
    within[0, 1] += 1e-13  # below 1e-12 x trace
    assert lib_update(within, 2.0, 0.0, 1e-3)[0] == 0
    indefinite = np.array([[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    assert lib_update(indefinite, 2.0, 0.0, 1e-3)[0] == -11
    assert L.cwf_hip_last_error(None).decode() == "dashpot matrix is not positive semidefinite"
    assert lib_update(-good, 2.0, 0.0, 1e-3)[0] == -11
    for bad in (np.nan, np.inf):
        nf = good.copy()
        nf[2, 2] = bad
        assert lib_update(nf, 2.0, 0.0, 1e-3)[0] == -11
        assert L.cwf_hip_last_error(None).decode() == "dashpot matrix is not finite"
    for mass in (0.0, -1.0, np.nan):
        assert lib_update(good, mass, 0.0, 1e-3)[0] == -11
        assert L.cwf_hip_last_error(None).decode() == "dashpot node mass must be positive"
    # semidefinite is accepted: a face-normal dashpot alone (rank one)
    nu = np.array([1.0, 2.0, 2.0]) / 3.0
    assert lib_update(5.0 * np.outer(nu, nu), 2.0, 0.0, 1e-3)[0] == 0


def test_incident_pattern_rows_are_twice_c_times_d():
    rng = np.random.Generator(np.random.PCG64(5))
    ids = np.array([7, 2, 11], np.uint32)
    G = rng.standard_normal((3, 3, 3))
    Cn = G @ G.transpose(0, 2, 1)
    d = np.array([0.3, -2.0, 0.5])  # used as given, not normalised
    pat = absorbing.incident_pattern(ids, Cn, d, 13).reshape(13, 3)
    for n, Cm in zip(ids, Cn):
        assert np.array_equal(pat[n], 2.0 * (Cm @ d))
    rest = np.ones(13, bool)
    rest[ids] = False
    assert np.all(pat[rest] == 0.0)


# ---- config ---------------------------------------------------------------------------------------------------------
def test_config_block_parses_into_the_dataclasses():
    r = config.load_config_from_string(BASE_YAML + ABSORBING)
    assert r.has_value(), r.error()
    assert r.value().absorbing == [AbsorbingBoundary("BASE", IncidentWave((1.0, 0.0, 0.5), "load_curve1")),
                                   AbsorbingBoundary("SIDES", None)]
    assert config.load_config_from_string(BASE_YAML).value().absorbing == []


def test_json_without_the_key_is_unchanged_and_with_it_only_appends():
    without, with_key = raw_json(BASE_YAML), raw_json(BASE_YAML + ABSORBING)
    assert "absorbing" not in without
    assert without.endswith('"probes": [1, 2]}}')  # the document's last section, as before
    assert with_key.startswith(without[:-1]) and json.loads(with_key)["absorbing"] == [
        {"group": "BASE", "incident": {"direction": [1.0, 0.0, 0.5], "velocity_curve": "load_curve1"}},
        {"group": "SIDES", "incident": None}]
    d = json.loads(without)
    assert "absorbing" not in d and list(d)[-1] == "output"


@pytest.mark.parametrize("name,block,msg,ctx", [
    ("not a list", "absorbing:\n  group: BASE\n", "absorbing must be a sequence when present", ["absorbing"]),
    ("entry not a map", "absorbing:\n  - BASE\n", "absorbing entry must be a map", ["absorbing", "[0]"]),
    ("group missing", "absorbing:\n  - group: BASE\n  - incident: {direction: [1, 0, 0], velocity_curve: load_curve1}\n",
     "absorbing.group is missing", ["absorbing", "[1]", "group"]),
    ("unknown curve", "absorbing:\n  - group: BASE\n    incident: {direction: [1, 0, 0], velocity_curve: quake}\n",
     "absorbing incident wave references unknown curve", ["absorbing", "[0]", "incident", "velocity_curve"]),
    ("curve missing", "absorbing:\n  - group: BASE\n    incident: {direction: [1, 0, 0]}\n",
     "absorbing incident wave references unknown curve", ["absorbing", "[0]", "incident", "velocity_curve"]),
    ("direction of two", "absorbing:\n  - group: BASE\n    incident: {direction: [1, 0], velocity_curve: load_curve1}\n",
     "absorbing.incident.direction must be a non-zero sequence[3]", ["absorbing", "[0]", "incident", "direction"]),
    ("direction missing", "absorbing:\n  - group: BASE\n    incident: {velocity_curve: load_curve1}\n",
     "absorbing.incident.direction must be a non-zero sequence[3]", ["absorbing", "[0]", "incident", "direction"]),
    ("direction zero", "absorbing:\n  - group: BASE\n    incident: {direction: [0, 0, 0.0], velocity_curve: load_curve1}\n",
     "absorbing.incident.direction must be a non-zero sequence[3]", ["absorbing", "[0]", "incident", "direction"]),
    ("incident not a map", "absorbing:\n  - group: BASE\n    incident: [1, 0, 0]\n",
     "absorbing.incident must be a map", ["absorbing", "[0]", "incident"]),
])
def test_config_errors_carry_their_context(name, block, msg, ctx):
    r = config.load_config_from_string(BASE_YAML + block)
    assert not r.has_value(), name
    assert r.error().message == msg and r.error().context == ctx, (name, r.error())


def test_native_scenario_refuses_absorbing_boundaries(tmp_path):
    """cwf_scenario_create steps by Newmark: the key is refused before any mesh or device is touched."""
    y = tmp_path / "s.yaml"
    y.write_text(BASE_YAML + ABSORBING)
    L = _lib.load()
    sc = C.c_void_p()
    assert L.cwf_scenario_create(os.fsencode(str(y)), _lib.MODE_PARITY, 0, _lib.SCENARIO_PACK_ONLY, C.byref(sc)) == -13
    assert L.cwf_hip_last_error(None).decode() == "absorbing boundaries need the explicit integrator"
    assert not sc.value
