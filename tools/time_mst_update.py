#!/usr/bin/env python3
"""Time new balances for m users of a device-resident Merkle sum tree of 2^20 entries (names user{i}, random 8-byte balances,
two currencies), m = 1, 1024, 2^16 and 2^20 random leaves, in one process on one box:
  DeviceMerkleSumTree.update_leaves_at   the leaves and the nodes above them re-hashed in place (sg_mst_update_dev);
  DeviceMerkleSumTree.from_entries       a fresh tree of the changed entries, the only way at the parent commit.
Both from Python lists to a synchronized tree.  The roots are compared once per m.  Warm-up, then the median of several runs,
beside the Poseidon hashes either way: m + the distinct ancestors of every level against 2^(depth + 1) - 1.  With --out FILE
the table is written there as well.  `device call` is the part of an update spent in sg_mst_update_dev and the wait for its
stream; the rest is Python checking, sorting and packing the batch.  No GPU: fails."""
import argparse
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from circuits_halo2_amd import ffi
from circuits_halo2_amd.merkle_sum_tree import DeviceMerkleSumTree

DEPTH, NC = 20, 2
BATCHES = [1, 1024, 1 << 16, 1 << 20]


def timed(f, warm, reps):
    for _ in range(warm):
        f()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    ffi.check(ffi.lib().sg_init(0))
    rng = random.Random(1)
    n = 1 << DEPTH
    entries = [(f"user{i}", [rng.randrange(1 << 64) for _ in range(NC)]) for i in range(n)]
    tree = DeviceMerkleSumTree.from_entries(entries, NC)
    device_ms, update_dev = [], DeviceMerkleSumTree._update_dev

    def timed_update_dev(self, *buffers):
        t0 = time.perf_counter()
        update_dev(self, *buffers)
        device_ms.append((time.perf_counter() - t0) * 1e3)
    DeviceMerkleSumTree._update_dev = timed_update_dev
    lines = [f"# new balances for m of 2^{DEPTH} entries (user{{i}}, random 8-byte balances, {NC} currencies), Python lists -> synchronized tree",
             f"# {torch.cuda.get_device_name(0)}, host clock, one process; medians of {args.reps} runs after 2 (update) and 1 (rebuild)",
             f"# {'m':>8} {'update_leaves_at':>18} {'min':>9} {'max':>9} {'device call':>12} {'from_entries':>14} {'min':>9} {'max':>9} {'ratio':>8} {'hashes, update':>15} {'rebuild':>9}"]
    for m in BATCHES:
        idx = sorted(rng.sample(range(n), m))
        rows = [[rng.randrange(1 << 64) for _ in range(NC)] for _ in idx]
        changed = list(entries)
        for i, bal in zip(idx, rows):
            changed[i] = (changed[i][0], bal)
        tree.update_leaves_at(idx, rows)
        rebuilt = DeviceMerkleSumTree.from_entries(changed, NC)
        same = all(bytes(a) == bytes(b) for a, b in zip(tree.root(), rebuilt.root()))
        assert same and torch.equal(tree.d_h, rebuilt.d_h) and torch.equal(tree.d_b, rebuilt.d_b), f"m = {m}: the updated tree is not the rebuilt one"
        del rebuilt
        up = timed(lambda: tree.update_leaves_at(idx, rows), 2, args.reps)
        dev = statistics.median(device_ms[-args.reps:])
        re = timed(lambda: DeviceMerkleSumTree.from_entries(changed, NC), 1, args.reps)
        at = np.array(idx, dtype=np.int64)
        hashes = m + sum(np.unique(at >> l).size for l in range(1, DEPTH + 1))
        med_up, med_re = statistics.median(up), statistics.median(re)
        lines.append(f"  {m:>8} {med_up:>15.2f} ms {min(up):>9.2f} {max(up):>9.2f} {dev:>9.2f} ms {med_re:>11.1f} ms {min(re):>9.1f} {max(re):>9.1f} "
                     f"{med_re / med_up:>7.1f}x {hashes:>15} {(2 << DEPTH) - 1:>9}")
        entries = changed
    lines.append("# every updated tree had the rebuilt tree's root, node hashes and node balances")
    print("\n".join(lines))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
