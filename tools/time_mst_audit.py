#!/usr/bin/env python3
"""Time the range audit of a device-resident Merkle sum tree (random usernames, random 5-byte balances, two currencies; n_bytes = 8)
of 2^16 and of 2^20 users, each with no plant, one plant and 1024 plants (2^64 at random leaves, by update_leaves_at), in one
process on one box:
  (a) tree.range_audit()               call to returned summary and list, host clock
  (b) its launches                     HIP events around ss_mst_range_audit_dev over preallocated buffers: the memset, the four
                                       kernels and the 16-byte copy
  (c) the same answer without it       the only way the parent commit offers, written out here so that it runs there too:
                                       sg_fr_from_montgomery_dev on a copy of d_b, the copy to the host, the high words compared
                                       and the paths walked in numpy
(c)'s masks are compared with (a)'s once per row where both exist.  Warm-up, then the median of --reps runs; beside them the
bytes the audit must read, 32 * n_currencies * (2^(depth + 1) - 1), and what they take at the 8 TB/s the project uses as HBM peak.
With --out FILE the table is written there as well.  No GPU: fails."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from circuits_halo2_amd import arithmetic as A, ffi
from circuits_halo2_amd.merkle_sum_tree import DeviceMerkleSumTree

NC, N_BYTES, HBM_PEAK = 2, 8, 8e12
DEPTHS, PLANTS = [16, 20], [0, 1, 1024]
HAS_AUDIT = hasattr(DeviceMerkleSumTree, "range_audit")


def host_clock(f, warm, reps):
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


def device_clock(f, warm, reps):
    for _ in range(warm):
        f()
    out = []
    for _ in range(reps):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        f()
        end.record()
        end.synchronize()
        out.append(start.elapsed_time(end))
    return out


def parents_way(tree):
    """-> (masks, unprovable leaves) from a host copy of the canonical balances"""
    depth, nc = tree.depth, tree.n_currencies
    words = A.fr_from_montgomery(tree.d_b.clone()).cpu().numpy().view(np.uint64).reshape(-1, nc, 4)
    flags = (words[:, :, N_BYTES // 8:] != 0).any(axis=(1, 2))
    idx = np.arange(1 << depth, dtype=np.int64)
    masks = flags[idx].astype(np.uint32)
    for level in range(depth):
        first = (2 << depth) - (2 << (depth - level))
        masks |= flags[first + ((idx >> level) ^ 1)].astype(np.uint32) << np.uint32(level + 1)
    return masks, np.flatnonzero(masks)


def row(label, ms):
    return f"  {label:<52} median {statistics.median(ms):10.4f} ms   min {min(ms):10.4f} ms   max {max(ms):10.4f} ms"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--depths", type=int, nargs="*", default=DEPTHS)
    args = ap.parse_args()
    ffi.check(ffi.lib().sg_init(0))
    lines = [f"# the range audit of a tree in HBM, {NC} currencies, n_bytes = {N_BYTES}; {torch.cuda.get_device_name(0)}, one process",
             f"# medians of {args.reps} runs after 3; (a) and (c) host clock, (b) HIP events"]
    rng = np.random.default_rng(3)
    for depth in args.depths:
        size = 1 << depth
        canon = np.zeros((size * NC, 32), dtype=np.uint8)
        canon[:, :5] = rng.integers(0, 256, (size * NC, 5), dtype=np.uint8)
        tree = DeviceMerkleSumTree(A.fr_random(bytes(range(32)), depth, size), A.fr_to_montgomery(torch.from_numpy(canon.reshape(-1)).cuda()),
                                   depth, NC)
        must_read = 32 * NC * (2 * size - 1)
        floor_us = must_read / HBM_PEAK * 1e6
        lines.append(f"# 2^{depth} users: the audit must read {must_read} bytes, {floor_us:.2f} us at {HBM_PEAK / 1e12:.0f} TB/s")
        planted = 0
        for plants in PLANTS:
            if plants > planted:
                spots = sorted(set(rng.integers(0, size, plants - planted).tolist()))
                tree.update_leaves_at(spots, [[1 << 64, 5]] * len(spots))
                planted = plants
            masks_c, bad_c = parents_way(tree)
            lines.append(f"2^{depth} users, {plants} plants: {bad_c.size} unprovable")
            if HAS_AUDIT:
                audit = tree.range_audit(N_BYTES)
                assert (audit.d_leaf_reasons.cpu().numpy().view(np.uint32) == masks_c).all() and (audit.unprovable == bad_c).all()
                lines.append(row("(a) tree.range_audit(), call to summary and list", host_clock(lambda: tree.range_audit(N_BYTES), 3, args.reps)))
                S = ffi.snapshot_lib()
                scratch = C.c_uint64(0)
                ffi.check(S.ss_mst_range_audit_scratch(depth, C.byref(scratch)))
                d_flags = torch.empty(2 * size - 1, dtype=torch.uint8, device="cuda")
                d_masks = torch.empty(size, dtype=torch.int32, device="cuda")
                d_bad = torch.empty(size, dtype=torch.int32, device="cuda")
                d_scratch = torch.empty(scratch.value // 4, dtype=torch.int32, device="cuda")
                summary = (C.c_uint64 * 4)()
                call = lambda: ffi.check(S.ss_mst_range_audit_dev(ffi.dev_ptr(tree.d_b), depth, NC, N_BYTES, ffi.dev_ptr(d_flags),
                                                                  ffi.dev_ptr(d_masks), ffi.dev_ptr(d_bad), size, ffi.dev_ptr(d_scratch),
                                                                  summary, ffi.current_stream_ptr()))
                dev = device_clock(call, 3, args.reps)
                lines.append(row("(b) its launches, HIP events", dev))
                lines.append(f"      = {statistics.median(dev) * 1e3 / floor_us:.1f} x the {floor_us:.2f} us of reading the balances once at HBM peak")
            lines.append(row("(c) from_montgomery, copy to the host, numpy", host_clock(lambda: parents_way(tree), 1, args.reps)))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
