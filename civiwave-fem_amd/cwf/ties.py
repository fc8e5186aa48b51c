"""Tie sets for ExplicitStepper.set_ties from node coordinates (include/cwf_hip.h "Tied boundaries"): the levels of a
laminar box, the pairs of two periodic faces, and the merge of groups that share nodes. Host only, by the library.

A tie set is (offsets u64 [groups + 1], node_ids u32 [members]): group g holds node_ids[offsets[g]:offsets[g + 1]].
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib


def _raise(what):
    msg, ctx = _lib.last_error(None)
    raise ValueError(f"{what} failed: {msg} {ctx}")


def _coords(coords):
    X = np.ascontiguousarray(coords, np.float64).reshape(-1, 3)
    return X, X.shape[0]


def levels(coords, node_ids, axis: int = 2, tolerance: float = 0.0):
    """The laminar box: the listed nodes binned by their coordinate along ``axis`` (tolerance relative to the model's
    extent along it, 0: 1e-9); every level of at least two nodes is one group. -> (offsets, node_ids)."""
    X, N = _coords(coords)
    ids = np.ascontiguousarray(node_ids, np.uint32).reshape(-1)
    G = C.c_uint64()
    off, out = np.zeros(ids.size // 2 + 2, np.uint64), np.zeros(max(ids.size, 1), np.uint32)
    if _lib.load().cwf_tie_levels(N, _lib.ptr(X), ids.size, _lib.ptr(ids), int(axis), float(tolerance), C.byref(G),
                                  _lib.ptr(off), _lib.ptr(out)):
        _raise("ties.levels")
    off = off[:G.value + 1].copy()
    return off, out[:int(off[-1])].copy()


def periodic(coords, ids_a, ids_b, axis: int, tolerance: float = 0.0):
    """Two opposite faces normal to ``axis``: each node of A with the node of B at the same place in the other two
    axes. -> (offsets, node_ids), group i = (ids_a[i], its partner)."""
    X, N = _coords(coords)
    a = np.ascontiguousarray(ids_a, np.uint32).reshape(-1)
    b = np.ascontiguousarray(ids_b, np.uint32).reshape(-1)
    G = C.c_uint64()
    off, out = np.zeros(a.size + 1, np.uint64), np.zeros(max(2 * a.size, 1), np.uint32)
    if _lib.load().cwf_tie_periodic(N, _lib.ptr(X), a.size, _lib.ptr(a), b.size, _lib.ptr(b), int(axis),
                                    float(tolerance), C.byref(G), _lib.ptr(off), _lib.ptr(out)):
        _raise("ties.periodic")
    off = off[:G.value + 1].copy()
    return off, out[:int(off[-1])].copy()


def merge(node_count: int, *sets):
    """Tie sets whose groups may share nodes -> the disjoint groups of their union, ordered by smallest member, members
    ascending."""
    offs, ids, base = [np.zeros(1, np.uint64)], [], 0
    for off, nodes in sets:
        off = np.asarray(off, np.uint64).reshape(-1)
        nodes = np.asarray(nodes, np.uint32).reshape(-1)
        offs.append(off[1:] + np.uint64(base))
        ids.append(nodes)
        base += nodes.size
    in_off = np.ascontiguousarray(np.concatenate(offs), np.uint64)
    in_ids = np.ascontiguousarray(np.concatenate(ids) if ids else np.zeros(0, np.uint32), np.uint32)
    G = C.c_uint64()
    off, out = np.zeros(in_ids.size // 2 + 2, np.uint64), np.zeros(max(in_ids.size, 1), np.uint32)
    if _lib.load().cwf_tie_merge(int(node_count), in_off.size - 1, _lib.ptr(in_off), _lib.ptr(in_ids), C.byref(G),
                                 _lib.ptr(off), _lib.ptr(out)):
        _raise("ties.merge")
    off = off[:G.value + 1].copy()
    return off, out[:int(off[-1])].copy()


def groups_of(offsets, node_ids):
    """The set as a list of index arrays."""
    off = np.asarray(offsets, np.int64)
    ids = np.asarray(node_ids)
    return [ids[off[g]:off[g + 1]] for g in range(off.size - 1)]
