#!/usr/bin/env python3
"""Time a finished Merkle sum tree from 2^16 entries (names user{i}, random 8-byte balances, two currencies), from the
Python list to a synchronized tree, in one process on one box:
  MerkleSumTree.from_entries         one sg_keccak256 call per user, balances to Montgomery bytes as Python integers, the
                                     tree built on the device and copied back (this path is the same at the parent commit);
  DeviceMerkleSumTree.from_entries   pack_entries on the host, sg_mst_entries_dev + sg_mst_build_dev, nothing comes back.
Both trees are compared bit for bit first.  Warm-up, then the median of several runs; with --out FILE the table is written
there as well.  No GPU: fails."""
import argparse
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from circuits_halo2_amd import ffi
from circuits_halo2_amd.merkle_sum_tree import DeviceMerkleSumTree, MerkleSumTree, pack_entries

N, NC = 1 << 16, 2


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
    args = ap.parse_args()
    ffi.check(ffi.lib().sg_init(0))
    rng = random.Random(1)
    entries = [(f"user{i}", [rng.randrange(1 << 64) for _ in range(NC)]) for i in range(N)]
    a, b = MerkleSumTree.from_entries(entries, NC), DeviceMerkleSumTree.from_entries(entries, NC)
    ah = b"".join(bytes(h) for level in a.nodes() for h, _ in level)
    ab = b"".join(bytes(v) for level in a.nodes() for _, v in level)
    assert b.d_h.cpu().numpy().tobytes() == ah and b.d_b.cpu().numpy().tobytes() == ab, "the two trees differ"
    host = timed(lambda: MerkleSumTree.from_entries(entries, NC), 1, 5)
    dev = timed(lambda: DeviceMerkleSumTree.from_entries(entries, NC), 2, 9)
    pack = timed(lambda: pack_entries(entries, NC), 1, 9)
    row = lambda name, t, note: f"{name:<36}median {statistics.median(t):8.1f} ms   min {min(t):8.1f} ms   max {max(t):8.1f} ms   {note}"
    lines = [f"# finished tree from 2^16 entries (user{{i}}, random 8-byte balances, {NC} currencies), Python list -> synchronized tree",
             f"# {torch.cuda.get_device_name(0)}, host clock, one process",
             row("MerkleSumTree.from_entries", host, f"{len(host)} runs after 1"),
             row("DeviceMerkleSumTree.from_entries", dev, f"{len(dev)} runs after 2"),
             row("  of which pack_entries (host)", pack, f"{len(pack)} runs after 1"),
             f"# medians: {statistics.median(host) / statistics.median(dev):.1f} x; the two trees are the same bytes"]
    print("\n".join(lines))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
