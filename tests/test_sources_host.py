"""Load sources and the obliquely incident plane wave, host side (no GPU): the exported entry points,
cwf_absorbing_incident_plane against a numpy restatement of the header's formula (bottom and side faces, tet4 and hex8,
rotation equivariance, normal incidence = 2 C_n d, winding independence, refusals), the two new keys of the scenario
config's ``absorbing[i].incident``, and the runner's choice between the pattern-and-curve path and load sources."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

from cwf import _lib, absorbing, config, meshgen, pack, run, scenarios
from cwf.explicit import LoadSource
from cwf.physics import AbsorbingBoundary, IncidentWave, compute_lame
from explicit_common import ABSORBING, BASE_YAML, H, face_geometry, raw_json, speeds

SYMBOLS = {"cwf_hip_explicit_set_sources", "cwf_hip_explicit_get_sources", "cwf_hip_explicit_source_info",
           "cwf_absorbing_incident_plane"}
TOL = 1e-9  # CWF_PLANE_WAVE_TOLERANCE


def test_library_declares_and_exports_the_entry_points():
    L = _lib.load()
    assert SYMBOLS <= set(_lib.declared_symbols())
    for n in SYMBOLS:
        assert hasattr(L, n), n
        assert getattr(L, n).argtypes is not None, n
    assert C.sizeof(_lib.ExplicitSourceDescC) == 56 and C.sizeof(_lib.ExplicitSourceInfoC) == 40
    text = open(_lib.HEADER_PATH).read()
    assert "#define CWF_EXPLICIT_MAX_SOURCES 8" in text and "#define CWF_PLANE_WAVE_TOLERANCE 1e-9" in text


def plane_wave_rule(X, tets, faces, mat, d, k, x0):
    """The header's formula in numpy: node -> A_n, node -> tau_n, c. The outward normal is the one pointing away from
    the centroid of the element that holds all of the face's nodes."""
    d, k, x0 = (np.asarray(v, np.float64) for v in (d, k, x0))
    kh = k / np.linalg.norm(k)
    l = compute_lame(mat.youngs_modulus, mat.poisson_ratio)
    rho, vp, vs = speeds(mat)
    q = abs(d @ kh) / np.linalg.norm(d)
    c = vp if q >= 1.0 - TOL else vs
    S = -(l.lambda_ * (d @ kh) * np.eye(3) + l.mu * (np.outer(d, kh) + np.outer(kh, d))) / c
    A = {}
    for face in faces:
        area, nu = face_geometry(X, face)
        owner = [e for e in tets if set(int(n) for n in face) <= set(int(n) for n in e)]
        assert len(owner) == 1
        if (X[np.asarray(face, np.int64)].mean(0) - X[np.asarray(owner[0], np.int64)].mean(0)) @ nu < 0.0:
            nu = -nu
        nn = np.outer(nu, nu)
        Af = (area / len(face)) * (rho * (vp * nn + vs * (np.eye(3) - nn)) @ d + S @ nu)
        for n in face:
            A[int(n)] = A.get(int(n), np.zeros(3)) + Af
    tau = {n: float(kh @ (X[n] - x0)) / c for n in A}
    return A, tau, c


def check_against_rule(mesh, cfg, faces, d, k, x0):
    ids, A, tau, c = absorbing.incident_plane_wave(mesh, cfg, faces, d, k, x0)
    wantA, wantT, wantc = plane_wave_rule(mesh.coords, mesh.tets.tolist(), faces.tolist(), cfg.materials[0], d, k, x0)
    assert ids.dtype == np.uint32 and list(ids) == sorted(wantA)
    assert c == wantc
    scale = max(np.abs(v).max() for v in wantA.values())
    for n, a, t in zip(ids, A, tau):
        assert np.abs(a - wantA[int(n)]).max() <= 1e-13 * scale, (n, a, wantA[int(n)])
        assert abs(t - wantT[int(n)]) <= 1e-15 * (1.0 + abs(wantT[int(n)])), (n, t, wantT[int(n)])
    return ids, A, tau, c


def oblique(angle_deg, wave):
    """khat at angle_deg from +z in the x-z plane and the unit polarisation of a P or an SV wave along it."""
    a = math.radians(angle_deg)
    k = np.array([math.sin(a), 0.0, math.cos(a)])
    return (k if wave == "P" else np.array([math.cos(a), 0.0, -math.sin(a)])), 3.0 * k  # khat is normalised inside


@pytest.mark.parametrize("wave", ["P", "SV"])
@pytest.mark.parametrize("element", ["tet4", "hex8"])
def test_plane_wave_on_the_bottom_and_a_side_face(element, wave):
    case = scenarios.block_case(4, 3, 3, h=H, element=element)
    m, cfg = case.mesh, case.cfg
    d, k = oblique(30.0, wave)
    d = 0.7 * d  # used as given
    x0 = (0.1, -0.2, 0.05)
    for on in (m.coords[:, 2] == 0.0, m.coords[:, 0] == 0.0):
        faces = meshgen.boundary_faces(m.tets, np.nonzero(on)[0])
        ids, A, tau, c = check_against_rule(m, cfg, faces, d, k, x0)
        assert np.array_equal(ids, np.nonzero(on)[0].astype(np.uint32))
        assert np.unique(np.round(tau * c / H, 9)).size > 1  # the delays differ from node to node
        assert c == speeds(cfg.materials[0])[1 if wave == "P" else 2]


def test_rotation_equivariance_on_a_jittered_permuted_block():
    tm = meshgen.jitter_and_permute(meshgen.kuhn_block(3, 3, 3, H), H)
    mesh = pack.from_tetmesh(tm)
    cfg = scenarios.make_config()
    faces = meshgen.boundary_faces(mesh.tets, np.arange(mesh.node_count))
    a, b, c = 0.7, -0.4, 1.1
    Rx = np.array([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]])
    Ry = np.array([[math.cos(b), 0, math.sin(b)], [0, 1, 0], [-math.sin(b), 0, math.cos(b)]])
    Rz = np.array([[math.cos(c), -math.sin(c), 0], [math.sin(c), math.cos(c), 0], [0, 0, 1]])
    R = Rz @ Ry @ Rx
    rot = pack.from_tetmesh(meshgen.TetMesh(tm.coords @ R.T, tm.tets, tm.node_groups))
    x0 = np.array([0.3, 0.1, -0.2])
    for wave in ("P", "SV"):
        d, k = oblique(30.0, wave)
        ids, A, tau, speed = check_against_rule(mesh, cfg, faces, d, k, x0)
        ids2, A2, tau2, speed2 = absorbing.incident_plane_wave(rot, cfg, faces, R @ d, R @ k, R @ x0)
        assert np.array_equal(ids, ids2) and speed == speed2
        assert np.abs(A2 - A @ R.T).max() <= 1e-12 * np.abs(A).max()
        assert np.abs(tau2 - tau).max() <= 1e-12 * np.abs(tau).max()


@pytest.mark.parametrize("element", ["tet4", "hex8"])
def test_normal_incidence_is_twice_c_times_d_with_equal_delays(element):
    case = scenarios.block_case(4, 3, 3, h=H, element=element)
    m, cfg = case.mesh, case.cfg
    faces = meshgen.boundary_faces(m.tets, np.nonzero(m.coords[:, 2] == 0.0)[0])
    ids, Cn = absorbing.dashpots(m, cfg, faces)
    for d in ((0.0, 0.0, 1.0), (1.0, 0.0, 0.0), (0.3, -0.4, 0.0)):  # P, S, S: khat = +z = -nu
        ids2, A, tau, c = absorbing.incident_plane_wave(m, cfg, faces, d, (0.0, 0.0, 2.0), (0.0, 0.0, 0.0))
        want = absorbing.incident_pattern(ids, Cn, d, m.node_count).reshape(-1, 3)[ids]
        assert np.array_equal(ids, ids2)
        assert np.abs(A - want).max() <= 1e-13 * np.abs(want).max()
        assert np.all(tau == tau[0]) and tau[0] == 0.0


def test_flipping_the_face_winding_changes_nothing():
    case = scenarios.block_case(4, 3, 3, h=H)
    m, cfg = case.mesh, case.cfg
    faces = meshgen.boundary_faces(m.tets, np.nonzero(m.coords[:, 0] == 0.0)[0])
    d, k = oblique(30.0, "SV")
    a = absorbing.incident_plane_wave(m, cfg, faces, d, k)
    flipped = faces[:, ::-1].copy()
    flipped[::2] = faces[::2]  # every other face flipped: a mixed list
    b = absorbing.incident_plane_wave(m, cfg, np.ascontiguousarray(flipped), d, k)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_refusals_of_the_plane_wave():
    case = scenarios.block_case(4, 3, 3, h=H)
    m, cfg = case.mesh, case.cfg
    good = meshgen.boundary_faces(m.tets, np.nonzero(m.coords[:, 2] == 0.0)[0])

    def refused(faces=good, d=(0.0, 0.0, 1.0), k=(0.0, 0.0, 1.0), mesh=m, cf=cfg):
        with pytest.raises(RuntimeError) as e:
            absorbing.incident_plane_wave(mesh, cf, faces, d, k)
        return str(e.value)

    msg = refused(d=(1.0, 0.0, 1.0))
    assert "polarisation is neither parallel nor perpendicular to the propagation" in msg and "cosine=0.707" in msg
    assert "neither parallel" in refused(d=(1e-4, 0.0, 1.0))  # cosine 1 - 5e-9: outside the tolerance
    assert "propagation must be a non-zero finite vector" in refused(k=(0.0, 0.0, 0.0))
    assert "polarisation must be a non-zero finite vector" in refused(d=(0.0, 0.0, 0.0))
    bad = good.copy()
    bad[3] = [good[0][0], good[1][1], int(np.nonzero(m.coords[:, 2] == m.coords[:, 2].max())[0][0])]
    msg = refused(faces=bad)
    assert "absorbing face is not a boundary face of the mesh" in msg and "'face=3'" in msg
    # a side face of a layered block: strata
    lay = scenarios.layered_case(3, 2, 4, [0, 1, 1, 2], h=H)
    side = meshgen.boundary_faces(lay.mesh.tets, np.nonzero(lay.mesh.coords[:, 0] == 0.0)[0])
    msg = refused(faces=side, mesh=lay.mesh, cf=lay.cfg, d=(1.0, 0.0, 0.0), k=(1.0, 0.0, 0.0))
    assert "plane wave faces span more than one material" in msg
    assert "face=" in msg and "material=" in msg and "first_material=" in msg
    # within one stratum it is accepted
    zc = lay.mesh.coords[side.astype(np.int64)][:, :, 2].mean(1)
    ids, A, tau, c = absorbing.incident_plane_wave(lay.mesh, lay.cfg, side[(zc > H) & (zc < 3 * H)], (1.0, 0.0, 0.0),
                                                   (1.0, 0.0, 0.0))
    assert c == speeds(scenarios.LAYER_MATERIALS[1])[1]


# ---- config ---------------------------------------------------------------------------------------------------------
OBLIQUE = """absorbing:
  - group: BASE
    incident: {direction: [1, 0, 0.5], velocity_curve: load_curve1, propagation: [0.5, 0, -1], origin: [0, 0, 2.5]}
  - group: SIDES
    incident: {direction: [1, 0, 0], velocity_curve: load_curve1, propagation: [1, 0, 0]}
"""


def test_the_two_new_keys_parse():
    r = config.load_config_from_string(BASE_YAML + OBLIQUE)
    assert r.has_value(), r.error()
    assert r.value().absorbing == [
        AbsorbingBoundary("BASE", IncidentWave((1.0, 0.0, 0.5), "load_curve1", (0.5, 0.0, -1.0), (0.0, 0.0, 2.5))),
        AbsorbingBoundary("SIDES", IncidentWave((1.0, 0.0, 0.0), "load_curve1", (1.0, 0.0, 0.0), None))]
    inc = json.loads(raw_json(BASE_YAML + OBLIQUE))["absorbing"]
    assert inc[0]["incident"] == {"direction": [1.0, 0.0, 0.5], "velocity_curve": "load_curve1",
                                  "propagation": [0.5, 0.0, -1.0], "origin": [0.0, 0.0, 2.5]}
    assert "origin" not in inc[1]["incident"] and inc[1]["incident"]["propagation"] == [1.0, 0.0, 0.0]


def test_a_document_without_the_keys_gives_todays_json_and_dataclasses():
    want = ('"absorbing": [{"group": "BASE", "incident": {"direction": [1, 0, 0.5], "velocity_curve": "load_curve1"}}, '
            '{"group": "SIDES", "incident": null}]}')
    got = raw_json(BASE_YAML + ABSORBING)
    assert got.endswith(want), got[-len(want) - 20:]
    assert got == raw_json(BASE_YAML)[:-1] + ", " + want
    r = config.load_config_from_string(BASE_YAML + ABSORBING)
    assert r.value().absorbing[0].incident == IncidentWave((1.0, 0.0, 0.5), "load_curve1")
    assert IncidentWave((1.0, 0.0, 0.5), "load_curve1").propagation is None


@pytest.mark.parametrize("name,inc,msg,key", [
    ("propagation of two", "propagation: [1, 0]", "absorbing.incident.propagation must be a non-zero sequence[3]",
     "propagation"),
    ("propagation zero", "propagation: [0, 0.0, 0]", "absorbing.incident.propagation must be a non-zero sequence[3]",
     "propagation"),
    ("propagation a scalar", "propagation: 1", "absorbing.incident.propagation must be a non-zero sequence[3]",
     "propagation"),
    ("origin of two", "propagation: [1, 0, 0], origin: [1, 0]", "absorbing.incident.origin must be a sequence[3]",
     "origin"),
])
def test_bad_keys_give_the_error_and_its_context(name, inc, msg, key):
    block = f"absorbing:\n  - group: SIDES\n  - group: BASE\n    incident: {{direction: [1, 0, 0], velocity_curve: load_curve1, {inc}}}\n"
    r = config.load_config_from_string(BASE_YAML + block)
    assert not r.has_value(), name
    assert r.error().message == msg and r.error().context == ["absorbing", "[1]", "incident", key], (name, r.error())


# ---- the runner's choice --------------------------------------------------------------------------------------------
def block_scenario(absorbing_entries):
    """The 4 x 3 x 3 block with groups BASE (z = 0) and LEFT (x = 0), two curves, and the given ``absorbing`` list."""
    from dataclasses import replace

    from cwf.physics import Curve

    tm = meshgen.kuhn_block(4, 3, 3, H)
    tm.node_groups["BASE"] = np.nonzero(tm.coords[:, 2] == 0.0)[0].astype(np.uint32)
    tm.node_groups["LEFT"] = np.nonzero(tm.coords[:, 0] == 0.0)[0].astype(np.uint32)
    mesh = pack.from_tetmesh(tm)
    cfg = scenarios.make_config()
    curves = dict(cfg.curves, quake=Curve([(0.0, 0.0), (1e-4, 1e-3), (1e-3, 0.0)]),
                  second=Curve([(0.0, 0.0), (2e-4, -1e-3), (1e-3, 0.0)]))
    cfg = replace(cfg, curves=curves, absorbing=absorbing_entries)
    return mesh, cfg, pack.build_packed_buffers(mesh, cfg)


def test_absorbing_setup_takes_todays_path_for_todays_form():
    entries = [AbsorbingBoundary("BASE", IncidentWave((1.0, 0.0, 0.25), "quake")), AbsorbingBoundary("LEFT", None)]
    m, cfg, P = block_scenario(entries)
    setup = run.absorbing_setup(cfg, m, P)
    ids, Cn, base, pattern, curve = setup  # the five it always returned
    assert len(setup) == 5 and not setup.sources
    bi, bC = absorbing.dashpots(m, cfg, absorbing.faces_of_group(m, "BASE"))
    li, lC = absorbing.dashpots(m, cfg, absorbing.faces_of_group(m, "LEFT"))
    wi, wC = absorbing.merge([(bi, bC), (li, lC)])
    assert np.array_equal(ids, wi) and np.array_equal(Cn, wC)
    assert np.array_equal(base, pack.assemble_load_vector(m, cfg, P.lumped_mass64))
    assert np.array_equal(pattern, absorbing.incident_pattern(bi, bC, (1.0, 0.0, 0.25), P.node_count))
    assert curve is cfg.curves["quake"]


def test_absorbing_setup_with_two_curves_yields_two_sources():
    entries = [AbsorbingBoundary("BASE", IncidentWave((0.0, 0.0, 1.0), "quake")),
               AbsorbingBoundary("LEFT", IncidentWave((1.0, 0.0, 0.0), "second", (1.0, 0.0, 0.0), (0.0, 0.0, 0.0)))]
    m, cfg, P = block_scenario(entries)
    setup = run.absorbing_setup(cfg, m, P)
    ids, Cn, base, pattern, curve = setup
    assert base is None and pattern is None and curve is None and len(setup.sources) == 2
    a, b = setup.sources
    assert isinstance(a, LoadSource) and a.curve is cfg.curves["quake"] and b.curve is cfg.curves["second"]
    bi, bC = absorbing.dashpots(m, cfg, absorbing.faces_of_group(m, "BASE"))
    assert np.array_equal(a.node_ids, bi) and np.array_equal(a.amplitude, 2.0 * (bC @ np.array([0.0, 0.0, 1.0])))
    assert np.all(a.delay == 0.0)
    li, A, tau, _ = absorbing.incident_plane_wave(m, cfg, absorbing.faces_of_group(m, "LEFT"), (1.0, 0.0, 0.0),
                                                  (1.0, 0.0, 0.0))
    assert np.array_equal(b.node_ids, li) and np.array_equal(b.amplitude, A) and np.array_equal(b.delay, tau)
    # one oblique entry on one curve is a source too
    m, cfg, P = block_scenario([AbsorbingBoundary("BASE", IncidentWave((0.5, 0.0, 1.0), "quake", (0.5, 0.0, 1.0)))])
    setup = run.absorbing_setup(cfg, m, P)
    assert len(setup.sources) == 1 and setup[4] is None and np.unique(setup.sources[0].delay).size > 1
