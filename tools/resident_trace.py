#!/usr/bin/env python3
"""Summarise the per-workgroup phase stamps of one resident-solve phase (CWF_RESIDENT_TRACE, resident.hip `stamp`):
s_memrealtime (100 MHz) per workgroup.

A box's row: 0 the phase's start (its poll begins: the previous phase's shares were stored just before), 1 every polled
granule carries the wanted tag, 7 the shares folded, 2 the scalars decided, 3 the own and halo p formed into the image,
4 the rows done, 5 the dots reduced, 6 the shares' granules stored (the phase's end). With the reducer role (the header
says "reducer 1") a box polls one decision granule and neither folds nor decides: its stamps 1, 7 and 2 are all
"decision seen". The last row is then the reducer's: 0 its poll start, 1 all shares seen (its last wave), 2 fold done,
3 decision stored, 4 the phase's end (thread 0's control-block stores issued).

Prints the median / max of each span, when the last workgroup arrived relative to the first one's release, and the
chain from the last share stored to the last box released: through the reducer's two hops, or (no reducer, old traces
included) through every box's sweep, fold and decide.

usage: python tools/resident_trace.py TRACE [INDEX]"""
import sys

import numpy as np


def blocks(path):
    cur = None
    for line in open(path):
        if line.startswith("#"):
            if cur:
                yield cur
            cur = {"hdr": line.strip(), "rows": []}
        elif line.strip() and cur is not None:
            cur["rows"].append([int(v) for v in line.split()])
    if cur:
        yield cur


def main():
    bs = list(blocks(sys.argv[1]))
    B = bs[int(sys.argv[2]) if len(sys.argv) > 2 else -1]
    a = np.array(B["rows"], np.int64)
    reducer = " reducer 1 " in B["hdr"] + " "
    red = None
    if reducer:  # the last row is the reducer's
        red, a = a[-1, 1:6].astype(np.float64) * 0.01, a[:-1]
    base = a[:, 1].min()
    t = (a[:, 1:8] - base).astype(np.float64) * 0.01  # us
    fold = (a[:, 8] - a[:, 2]).astype(np.float64) * 0.01 if a.shape[1] > 8 else None  # stamp 7: the fold done
    names = ["poll", "fold+decide", "form", "rows", "reduce", "shares"]
    print(f"{B['hdr']}: {len(a)} boxes" + (" + the reducer" if reducer else ""))
    for i, n in enumerate(names):
        d = t[:, i + 1] - t[:, i]
        note = "  (none: the reducer folds and decides)" if reducer and i == 1 else ""
        print(f"  {n:12s} median {np.median(d):6.2f}  max {d.max():6.2f} us{note}")
    if fold is not None and not reducer and np.all(a[:, 8] > 0):
        print(f"  (fold alone median {np.median(fold):.2f} max {fold.max():.2f} us; decide the rest)")
    print(f"  phase start spread {t[:, 0].max() - t[:, 0].min():.2f} us, release (wait done) spread "
          f"{t[:, 1].max() - t[:, 1].min():.2f} us, last end {t[:, 6].max():.2f} us after the first start, "
          f"compute (release -> end) median {np.median(t[:, 6] - t[:, 1]):.2f} max {np.max(t[:, 6] - t[:, 1]):.2f}")
    # the chain behind the slowest box: its shares stored (its stamp 0) -> ... -> the last box free to form (stamp 2)
    last = t[:, 0].max()
    if reducer and np.all(red > 0):
        r = red - base * 0.01
        print(f"  chain: last share stored -> reducer saw all {r[1] - last:.2f} -> folded {r[2] - r[1]:.2f} -> decision "
              f"stored {r[3] - r[2]:.2f} -> first box saw it {t[:, 1].min() - r[3]:.2f}, median {np.median(t[:, 1]) - r[3]:.2f}, "
              f"last {t[:, 1].max() - r[3]:.2f}: {t[:, 1].max() - last:.2f} us in all (median box {np.median(t[:, 1]) - last:.2f})")
        print(f"  reducer: poll {r[1] - r[0]:.2f}, fold {r[2] - r[1]:.2f}, decide + store {r[3] - r[2]:.2f}, "
              f"record {r[4] - r[3]:.2f} us")
    else:
        print(f"  chain: last share stored -> first box saw all {t[:, 1].min() - last:.2f}, median "
              f"{np.median(t[:, 1]) - last:.2f}, last {t[:, 1].max() - last:.2f} -> folded and decided (median box) "
              f"{np.median(t[:, 2] - t[:, 1]):.2f}: {t[:, 2].max() - last:.2f} us in all (median box "
              f"{np.median(t[:, 2]) - last:.2f})")
    # per box: the form + rows span by the number of block faces the box touches (box b = (bx, by, bz), x fastest)
    hdr = B["hdr"].split("boxes ")
    if len(hdr) > 1:
        gx, gy, gz = (int(v) for v in hdr[1].split("x"))
        b = a[:, 0]
        pos = np.stack([b % gx, (b // gx) % gy, b // (gx * gy)], 1)
        faces = ((pos == 0) | (pos == np.array([gx, gy, gz]) - 1)).sum(1)
        work = t[:, 4] - t[:, 2]
        for f in sorted(set(faces.tolist())):
            w = work[faces == f]
            print(f"  boxes on {f} block faces: {len(w):3d}, form + rows median {np.median(w):5.2f} max {w.max():5.2f} us")
        for ax, n in zip("xyz", (gx, gy, gz)):
            print(f"  along {ax}: " + " ".join(f"{np.median(work[pos[:, 'xyz'.index(ax)] == q]):.2f}" for q in range(n)))


if __name__ == "__main__":
    main()
