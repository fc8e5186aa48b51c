"""cwf_hip_system_memory through the calls that allocate after create (csrc/devmem.hpp: one arena per handle), stage by
stage against tests/golden/memory_ledger.json. tests/golden/make_memory_ledger.py wrote that file from the library of
the commit before the arena, running the stage lists below: every number is an integer the layout code decides, so
the comparison is an equality. (Free device memory is never asked: other work shares the device.)

Handles: the 8 x 3 x 4 block and the jittered 7 x 6 x 5 block of test_gpu_create_paths, both FAST. A FAST handle that
renumbers its nodes refuses PARITY (test_gpu_renumber), so on it stage 3 is that refusal, which must not move the
number either; the jittered block runs a second time in the caller's node order, where PARITY (its node tiles and the
streamed folds' granules) does run. The renumbered handle is the one that allocates the caller-order mass and mask
of stage 7. Then a two-rank LOCAL PARITY shard: after attach, after the first group solve (the chunk-partial slot
block), after the second (the block is reused)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from cwf import _lib, modal, pcg, scenarios, shard

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "memory_ledger.json")
# name -> (mesh, keep the caller's node order)
HANDLES = {
    "block": (lambda: scenarios.block_case(8, 3, 4, h=0.1), False),
    "jitter": (lambda: scenarios.block_case(7, 6, 5, h=0.1, jitter=True), False),
    "jitter-caller-order": (lambda: scenarios.block_case(7, 6, 5, h=0.1, jitter=True), True),
}
SHARD_SHAPE = (10, 6, 12)  # 1,001 nodes: test_gpu_shard's PARITY shards, cut at a multiple of 256 nodes


def memory(s) -> int:
    mem = C.c_uint64()
    assert _lib.load().cwf_hip_system_memory(s._h, C.byref(mem)) == 0
    return int(mem.value)


def _solve(s, rhs):
    x, r = np.zeros_like(rhs), np.zeros_like(rhs)
    pcg.solve_pcg(s, rhs, pcg.PcgSettings(400, 1e-6, False), pcg.PcgVectors(x, r)).value()


def _modes(s, block):
    modal.solve_modes(s, modal.ModalSettings(modes=2, block=block, max_outer=2)).value()


def handle_stages(name):
    """[(stage, bytes)] of one handle, in the order of the module docstring's list."""
    make, keep = HANDLES[name]
    case = make()
    P = case.packing
    sK, sM = case.scalars()
    s = pcg.MatrixFreeSystem(P.connectivity, P.gradients, P.volume, P.material_index, case.materials, P.lumped_mass,
                             P.bc_mask, P.node_count, P.element_count, P.dof_count, sK, sM, P.reduction_block,
                             P.reduction_partials, (P.offsets, P.element_indices, P.local_indices), _lib.MODE_FAST, 0,
                             P.position64 if getattr(P, "position64", None) is not None else P.position0,
                             keep_node_order=keep)
    rhs = case.static_rhs()
    out = []

    def stage(label):
        out.append((label, memory(s)))

    s.handle()
    stage("1 create")
    _solve(s, rhs)
    stage("2 FAST solve")
    s.mode = _lib.MODE_PARITY
    try:
        _solve(s, rhs)
        stage("3 PARITY solve")
    except pcg.PcgException as e:  # a renumbered handle
        assert e.code == -13, e
        stage("3 PARITY refused")
    s.mode = _lib.MODE_FAST
    _modes(s, 4)
    stage("4 modal block 4")
    _modes(s, 8)
    stage("5 modal block 8")
    _modes(s, 4)
    stage("6 modal block 4 again")
    A = np.random.Generator(np.random.PCG64(2)).uniform(-1, 1, (2, P.dof_count)).astype(np.float32)
    modal.block_gram(s, A, mass_weighted=True).value()
    stage("7 mass-weighted gram, caller order")
    b = rhs.astype(np.float64)
    pcg.solve_refined(s, b).value()
    stage("8 refined solve")
    pcg.solve_refined(s, b).value()
    stage("9 refined solve again")
    s.close()
    return out


def shard_stages():
    """[(stage, [bytes of rank 0, of rank 1])] of a two-rank LOCAL PARITY system."""
    glob = scenarios.block_case(*SHARD_SHAPE, h=0.1, tol=1e-6)
    sK, sM = glob.scalars()
    P = glob.packing
    ranges = shard.slab_ranges(P.node_count, 2, align=256)
    comm = shard.Comm.local(2)
    systems, shards, rhs, xs = [], [], [], []
    for k in range(2):
        src = pcg.MatrixFreeSystem.from_packing(P, glob.materials, sK, sM, mode=_lib.MODE_PARITY)
        sh = shard.build_shard(src, ranges, k)
        s = sh.system(glob.materials, sK, sM, mode=_lib.MODE_PARITY)
        comm.attach(s, sh)
        systems.append(s)
        shards.append(sh)
        rhs.append(sh.local_dofs(glob.static_rhs()))
        xs.append(np.zeros(3 * sh.local_nodes, np.float32))
    out = [("attach", [memory(s) for s in systems])]
    for label in ("first group solve", "second group solve"):
        shard.solve_pcg_group(systems, rhs, pcg.PcgSettings(800, 1e-6, False), xs).value()
        out.append((label, [memory(s) for s in systems]))
    comm.close()
    for s in systems:
        s.close()
    return out


def record():
    """What the golden file holds (make_memory_ledger.py): JSON's lists for the tuples."""
    out = {name: [list(x) for x in handle_stages(name)] for name in sorted(HANDLES)}
    out["shard"] = [list(x) for x in shard_stages()]
    return out


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", sorted(HANDLES))
def test_handle_memory_by_stage(name):
    got = [list(x) for x in handle_stages(name)]
    for label, nbytes in got:
        print(f"{name}: {label}: {nbytes}")
    byte = dict(got)
    labels = [x[0] for x in got]
    # the list itself: what must allocate does, and what must not, does not
    assert byte[labels[5]] == byte[labels[4]] > byte[labels[3]], "modal regrow: larger once, then kept"
    assert byte[labels[8]] == byte[labels[7]] > byte[labels[6]], "refine workspace: once"
    if labels[2] == "3 PARITY refused":
        assert byte[labels[2]] == byte[labels[1]] and byte[labels[6]] > byte[labels[5]], "renumbered: mass and mask"
    else:
        assert byte[labels[2]] > byte[labels[1]] and byte[labels[6]] == byte[labels[5]]
    assert got == golden()[name]


def test_shard_memory_by_stage():
    got = [list(x) for x in shard_stages()]
    for label, nbytes in got:
        print(f"shard: {label}: {nbytes}")
    assert all(a > b for a, b in zip(got[1][1], got[0][1])), "the first PARITY group solve allocates"
    assert got[2][1] == got[1][1], "the second reuses the slot block"
    assert got == golden()["shard"]
