"""Absorbing (viscous, Lysmer-Kuhlemeyer) boundaries of the explicit stepper and the incident wave through them
(include/cwf_hip.h "Absorbing boundaries").

``dashpots`` turns a face list into per-node 3x3 matrices C_n by the library (cwf_absorbing_dashpots, host only);
``ExplicitStepper.set_dashpots`` takes them. ``incident_pattern`` is the load pattern of the compliant base: with the
stepper's load curve c(t) it applies 2 C_n d c(t), the force of an incident wave of particle velocity d c(t).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib, meshgen
from .physics import compute_lame


def faces_of_group(mesh, name: str) -> np.ndarray:
    """The faces of physical group `name`: its mesh.surfaces entries; when it has none, the boundary faces of the
    mesh whose nodes all lie in the node group of that name. u32 [F,3] (triangles) or [F,4] (quads)."""
    gid = mesh.group_names.get(name)
    if gid is None:
        raise KeyError(f"absorbing boundary references missing physical group '{name}'")
    faces = [tuple(nodes) for sg, nodes in mesh.surfaces if sg == gid]
    if faces:
        k = len(faces[0])
        if any(len(f) != k for f in faces):
            raise ValueError(f"physical group '{name}' mixes triangles and quads")
        return np.asarray(faces, np.uint32).reshape(-1, k)
    nodes = mesh.node_groups.get(gid)
    k = 4 if mesh.tets.shape[1] == 8 else 3
    if nodes is None or not len(nodes):
        return np.zeros((0, k), np.uint32)
    return meshgen.boundary_faces(mesh.tets, nodes).reshape(-1, k)


def element_materials(mesh, cfg) -> np.ndarray:
    """The material slot of every element (the binding pack.preprocess makes), u32 [E]."""
    names = [m.name for m in cfg.materials]
    eg = mesh.element_group if mesh.element_group is not None else np.ones(mesh.element_count, np.uint32)
    mat = np.full(mesh.element_count, 0xFFFFFFFF, np.uint32)
    seen = set()
    for a in cfg.assignments:
        gid = mesh.group_names.get(a.group)
        if gid is None or gid in seen or a.material not in names:
            continue
        seen.add(gid)
        mat[eg == gid] = names.index(a.material)
    return mat


def _face_call_args(mesh, cfg, faces):
    """The mesh, material and face arguments cwf_absorbing_dashpots and cwf_absorbing_incident_plane share, and the
    arrays that keep them alive."""
    faces = np.ascontiguousarray(faces, np.uint32)
    if faces.ndim != 2 or faces.shape[1] not in (3, 4):
        raise ValueError("faces must be u32 [F,3] or [F,4]")
    coords = np.ascontiguousarray(mesh.coords, np.float64)
    conn = np.ascontiguousarray(mesh.tets, np.uint32)
    mat = np.ascontiguousarray(element_materials(mesh, cfg), np.uint32)
    lame = [compute_lame(m.youngs_modulus, m.poisson_ratio) for m in cfg.materials]
    rho = np.ascontiguousarray([m.density for m in cfg.materials], np.float64)
    lam = np.ascontiguousarray([l.lambda_ for l in lame], np.float64)
    mu = np.ascontiguousarray([l.mu for l in lame], np.float64)
    p = _lib.ptr
    args = (mesh.node_count, p(coords), conn.shape[0], conn.shape[1], p(conn), p(mat), len(cfg.materials), p(rho),
            p(lam), p(mu), faces.shape[0], faces.shape[1], p(faces))
    return args, max(1, min(mesh.node_count, faces.size)), (faces, coords, conn, mat, rho, lam, mu)


def dashpots(mesh, cfg, faces):
    """-> (node_ids u32 [n] ascending, C f64 [n,3,3]): the viscous-boundary matrices of `faces`, each face with the
    material of the element that owns it."""
    args, room, _keep = _face_call_args(mesh, cfg, faces)
    ids = np.zeros(room, np.uint32)
    Cn = np.zeros(9 * room, np.float64)
    count = C.c_uint64()
    p = _lib.ptr
    rc = _lib.load().cwf_absorbing_dashpots(*args, C.byref(count), p(ids), p(Cn))
    if rc:
        msg, ctx = _lib.last_error(None)
        raise RuntimeError(f"{msg} {ctx}")
    n = count.value
    return ids[:n].copy(), Cn[:9 * n].reshape(n, 3, 3).copy()


def incident_plane_wave(mesh, cfg, faces, polarisation, propagation, origin=(0.0, 0.0, 0.0)):
    """-> (node_ids u32 [n] ascending, A f64 [n,3], tau f64 [n], wave speed): the entries of the load source that
    feeds the plane wave of particle velocity d g(t - tau), tau = khat . (x - origin) / c, in through the dashpots of
    `faces` (cwf_absorbing_incident_plane): the dashpot's share C_n d plus the free-field traction. d = polarisation as
    given; khat = propagation normalised; c = V_p for d parallel to khat, V_s for d perpendicular, anything else is
    refused, and so are faces over more than one material."""
    args, room, _keep = _face_call_args(mesh, cfg, faces)
    d = np.ascontiguousarray(polarisation, np.float64).reshape(3)
    k = np.ascontiguousarray(propagation, np.float64).reshape(3)
    x0 = np.ascontiguousarray(origin, np.float64).reshape(3)
    ids = np.zeros(room, np.uint32)
    A = np.zeros(3 * room, np.float64)
    tau = np.zeros(room, np.float64)
    count, speed = C.c_uint64(), C.c_double()
    p = _lib.ptr
    rc = _lib.load().cwf_absorbing_incident_plane(*args, p(d), p(k), p(x0), C.byref(count), p(ids), p(A), p(tau),
                                                  C.byref(speed))
    if rc:
        msg, ctx = _lib.last_error(None)
        raise RuntimeError(f"{msg} {ctx}")
    n = count.value
    return ids[:n].copy(), A[:3 * n].reshape(n, 3).copy(), tau[:n].copy(), speed.value


def merge(parts):
    """Sum several (node_ids, C) per node -> (node_ids ascending, C)."""
    parts = [(np.asarray(i, np.int64), np.asarray(c, np.float64).reshape(-1, 3, 3)) for i, c in parts]
    if not parts:
        return np.zeros(0, np.uint32), np.zeros((0, 3, 3), np.float64)
    ids = np.unique(np.concatenate([i for i, _ in parts]))
    out = np.zeros((ids.size, 3, 3), np.float64)
    for i, c in parts:
        np.add.at(out, np.searchsorted(ids, i), c)
    return ids.astype(np.uint32), out


def incident_pattern(node_ids, C, direction, node_count: int) -> np.ndarray:
    """f64 [3N] with rows 2 C_n d: the stepper's load pattern of an incident wave of particle velocity d c(t) in m/s,
    c the stepper's load curve. `direction` is used as given, not normalised."""
    d = np.asarray(direction, np.float64).reshape(3)
    out = np.zeros((int(node_count), 3), np.float64)
    out[np.asarray(node_ids, np.int64)] = 2.0 * (np.asarray(C, np.float64).reshape(-1, 3, 3) @ d)
    return out.reshape(-1)
