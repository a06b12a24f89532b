#!/usr/bin/env python3
"""Time `DeviceMerkleSumTree.from_csv` from a file on disk to a tree whose root is on the host: 2^16 and 2^20 rows of two
currencies (names user{i}, random 8-byte balances), written to a temporary directory first.  Warm-up, then the median of
several runs, and which way the text went: `csv_ingest` is "device" where the device read it, "host" where the tree does not
say (every commit before the device reader: parse_csv_to_entries, pack_entries, sg_mst_entries_dev).

Only names that exist without the device reader are used, so the same script measures both sides of that change.  The rows
behind the totals say where the time goes: the file read and the upload as timed here on their own (numpy, one torch copy),
and -- where the library has them -- the two entry points, each of which ends in a wait, and the tree build with the root.
With --out FILE the table is written there as well.  No GPU: fails."""
import argparse
import ctypes as C
import os
import random
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from circuits_halo2_amd import ffi
from circuits_halo2_amd.merkle_sum_tree import DeviceMerkleSumTree, parse_csv_to_entries

NC = 2


def write_csv(path, n):
    rng = random.Random(n)
    with open(path, "w", newline="") as f:
        f.write("username,balance_ETH_ETH,balance_USDT_ETH\n")
        f.write("".join(f"user{i},{rng.randrange(1 << 64)},{rng.randrange(1 << 64)}\n" for i in range(n)))


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


def row(name, t, note=""):
    return f"{name:<52}median {statistics.median(t):9.2f} ms   min {min(t):9.2f} ms   max {max(t):9.2f} ms   {note}"


def parts(path):
    """the device reader's steps on their own, through the entry points: [] where the library has none"""
    L = ffi.lib()
    if not hasattr(L, "sg_mst_csv_scan_dev"):
        return []
    data = np.fromfile(path, dtype=np.uint8)
    size, body_off = int(data.size), data[:4096].tobytes().index(b"\n") + 1
    pad = -body_off % 16
    d_file = torch.empty(pad + size, dtype=torch.uint8, device="cuda")
    d_text = d_file[pad:]
    d_text.copy_(torch.from_numpy(data))
    tile = C.c_uint32(0)
    L.sg_mst_csv_geometry(C.byref(tile), None)
    d_tiles = torch.empty(-(-(size - body_off) // tile.value) + 2, dtype=torch.int32, device="cuda")
    n, flags, problem = C.c_uint64(0), C.c_uint32(0), C.c_uint64(0)
    stream = ffi.current_stream_ptr()
    scan = lambda: ffi.check(L.sg_mst_csv_scan_dev(ffi.dev_ptr(d_text), size, body_off, ffi.dev_ptr(d_tiles), C.byref(n), C.byref(flags), stream))
    scan()
    rows = 1 << max(0, (n.value - 1).bit_length())
    d_users = torch.empty(32 * rows, dtype=torch.uint8, device="cuda")
    d_bals = torch.empty(32 * rows * NC, dtype=torch.uint8, device="cuda")
    d_spans = torch.empty(n.value + 2 + 2 * n.value * (1 + NC), dtype=torch.int64, device="cuda")
    entries = lambda: ffi.check(L.sg_mst_csv_entries_dev(ffi.dev_ptr(d_text), size, body_off, ffi.dev_ptr(d_tiles), ord(","), NC, n.value, rows,
                                                         ffi.dev_ptr(d_spans), ffi.dev_ptr(d_users), ffi.dev_ptr(d_bals), C.byref(problem), stream))
    build = lambda: DeviceMerkleSumTree(d_users, d_bals, rows.bit_length() - 1, NC).root()
    return [row("  sg_mst_csv_scan_dev (classify, scan, wait)", timed(scan, 2, 9)),
            row("  sg_mst_csv_entries_dev (rows, split, wait, hash)", timed(entries, 2, 9)),
            row("  tree build + root", timed(build, 2, 9))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--logs", default="16,20", help="log2 of the row counts, comma-separated")
    args = ap.parse_args()
    ffi.check(ffi.lib().sg_init(0))
    lines = [f"# DeviceMerkleSumTree.from_csv(path, {NC}) + root(): file on disk -> tree in HBM, root on the host",
             f"# {torch.cuda.get_device_name(0)}, host clock, one process; user{{i}}, random 8-byte balances, {NC} currencies"]
    with tempfile.TemporaryDirectory() as d:
        for log in [int(x) for x in args.logs.split(",")]:
            n = 1 << log
            path = os.path.join(d, f"snapshot_{log}.csv")
            write_csv(path, n)
            tree = DeviceMerkleSumTree.from_csv(path, NC)
            took = getattr(tree, "csv_ingest", "host")
            want = DeviceMerkleSumTree.from_entries(parse_csv_to_entries(path, NC)[0], NC)     # the host parse, whatever from_csv does
            for a, b in ((tree.d_users, want.d_users), (tree.d_bals, want.d_bals), (tree.d_h, want.d_h), (tree.d_b, want.d_b)):
                assert torch.equal(a, b), "from_csv and from_entries of the parsed file differ"
            del want
            reps = 9 if log <= 16 else 3
            total = timed(lambda: DeviceMerkleSumTree.from_csv(path, NC).root(), 1, reps)
            read = timed(lambda: np.fromfile(path, dtype=np.uint8), 1, reps)
            data = np.fromfile(path, dtype=np.uint8)
            upload = timed(lambda: torch.from_numpy(data).cuda(), 1, reps)
            lines += [f"# 2^{log} rows, {os.path.getsize(path) / 1e6:.1f} MB, csv_ingest = {took}; the four arrays equal from_entries' of the parsed file",
                      row(f"from_csv + root, 2^{log} rows", total, f"{reps} runs after 1"),
                      row("  np.fromfile alone", read), row("  upload alone (pageable host -> device)", upload)] + parts(path)
            del tree
    print("\n".join(lines))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
