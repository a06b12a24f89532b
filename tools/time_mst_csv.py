#!/usr/bin/env python3
"""Time `DeviceMerkleSumTree.from_csv` from a file on disk to a tree whose root is on the host: 2^16 and 2^20 rows of two
currencies (names user{i}, random 8-byte balances), written to a temporary directory first.  Warm-up, then the median of
several runs, and which way the text went: `csv_ingest` is "device" where the device read it, "host" where the tree does not
say (every commit before the device reader: parse_csv_to_entries, pack_entries, sg_mst_entries_dev).

Only names that exist without the device reader are used, so the same script measures both sides of that change.  The rows
behind the totals say where the time goes: the file read and the upload as timed here on their own (numpy, one torch copy),
and -- where the library has them -- the two entry points, each of which ends in a wait, and the tree build with the root.
With --out FILE the table is written there as well.  No GPU: fails.

--sorted times `from_csv_sorted` the same way, on files whose names are in random order, after comparing the tree's four device
arrays with `from_entries` of the host-sorted entries; the parts are then the upload, the scan, ss_mst_csv_entries_sorted_dev
(split, sort, gather, hash) and the build.  It also times the lookup by name on a fresh tree: the first `index_of_username`,
and -- where the tree has it -- `indices_of_usernames` of 1024 names.  Again only names every commit has are required."""
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


def write_csv(path, n, shuffled=False):
    rng = random.Random(n)
    ids = list(range(n))
    if shuffled:
        rng.shuffle(ids)
    with open(path, "w", newline="") as f:
        f.write("username,balance_ETH_ETH,balance_USDT_ETH\n")
        f.write("".join(f"user{i},{rng.randrange(1 << 64)},{rng.randrange(1 << 64)}\n" for i in ids))


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


def parts(path, sorted_leaves=False):
    """the device reader's steps on their own, through the entry points: [] where the library has none"""
    L = ffi.lib()
    if not hasattr(L, "sg_mst_csv_scan_dev") or (sorted_leaves and not hasattr(ffi, "snapshot_lib")):
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
    if sorted_leaves:
        S = ffi.snapshot_lib()
        sort_bytes = C.c_uint64(0)
        ffi.check(S.ss_mst_sort_scratch(n.value, C.byref(sort_bytes)))
        d_spans2 = torch.empty(2 * (n.value + 1 + 2 * n.value * (1 + NC)), dtype=torch.int64, device="cuda")
        d_sort = torch.empty(sort_bytes.value, dtype=torch.uint8, device="cuda")
        d_order = torch.empty(n.value, dtype=torch.int32, device="cuda")
        d_names = torch.empty(2 * n.value, dtype=torch.int32, device="cuda")
        entries = lambda: ffi.check(S.ss_mst_csv_entries_sorted_dev(ffi.dev_ptr(d_text), size, body_off, ffi.dev_ptr(d_tiles), ord(","), NC, n.value,
                                                                    rows, ffi.dev_ptr(d_spans2), ffi.dev_ptr(d_sort), ffi.dev_ptr(d_order),
                                                                    ffi.dev_ptr(d_names), ffi.dev_ptr(d_users), ffi.dev_ptr(d_bals),
                                                                    C.byref(problem), stream))
    what = "ss_mst_csv_entries_sorted_dev (split, sort, hash)" if sorted_leaves else "sg_mst_csv_entries_dev (rows, split, wait, hash)"
    return [row("  sg_mst_csv_scan_dev (classify, scan, wait)", timed(scan, 2, 9)),
            row("  " + what, timed(entries, 2, 9)),
            row("  tree build + root", timed(build, 2, 9))]


def lookups(path, names):
    """lookup by name on fresh trees: the first index_of_username, a later one, and 1024 names at once where the tree can"""
    first, many = [], []
    for r in range(3):
        tree = DeviceMerkleSumTree.from_csv_sorted(path, NC)
        tree.root()
        first += timed(lambda: tree.index_of_username(names[r]), 0, 1)
        del tree
    tree = DeviceMerkleSumTree.from_csv_sorted(path, NC)
    later = timed(lambda: tree.index_of_username(names[7]), 1, 5)
    out = [row("  first index_of_username of a fresh tree", first, "3 trees"), row("  a later index_of_username", later)]
    if hasattr(tree, "indices_of_usernames"):
        fresh = DeviceMerkleSumTree.from_csv_sorted(path, NC)
        many = timed(lambda: fresh.indices_of_usernames(names), 1, 5)
        out.append(row(f"  indices_of_usernames of {len(names)} names", many, "a tree whose entries are unparsed"))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--logs", default="16,20", help="log2 of the row counts, comma-separated")
    ap.add_argument("--sorted", action="store_true", help="from_csv_sorted on files with the names in random order, and the lookup by name")
    args = ap.parse_args()
    ffi.check(ffi.lib().sg_init(0))
    ctor = "from_csv_sorted" if args.sorted else "from_csv"
    make = getattr(DeviceMerkleSumTree, ctor)
    lines = [f"# DeviceMerkleSumTree.{ctor}(path, {NC}) + root(): file on disk -> tree in HBM, root on the host",
             f"# {torch.cuda.get_device_name(0)}, host clock, one process; user{{i}}{' in random order' if args.sorted else ''}, "
             f"random 8-byte balances, {NC} currencies"]
    with tempfile.TemporaryDirectory() as d:
        for log in [int(x) for x in args.logs.split(",")]:
            n = 1 << log
            path = os.path.join(d, f"snapshot_{log}.csv")
            write_csv(path, n, shuffled=args.sorted)
            tree = make(path, NC)
            took = getattr(tree, "csv_ingest", None) or "host"
            parsed = parse_csv_to_entries(path, NC)[0]                                         # the host parse, whatever from_csv does
            if args.sorted:
                parsed.sort(key=lambda e: e[0].encode())
            want = DeviceMerkleSumTree.from_entries(parsed, NC)
            for a, b in ((tree.d_users, want.d_users), (tree.d_bals, want.d_bals), (tree.d_h, want.d_h), (tree.d_b, want.d_b)):
                assert torch.equal(a, b), f"{ctor} and from_entries of the parsed file differ"
            names = [parsed[(7919 * j) % n][0] for j in range(1024)]
            del want, parsed
            reps = 9 if log <= 16 else 3
            total = timed(lambda: make(path, NC).root(), 1, reps)
            read = timed(lambda: np.fromfile(path, dtype=np.uint8), 1, reps)
            data = np.fromfile(path, dtype=np.uint8)
            upload = timed(lambda: torch.from_numpy(data).cuda(), 1, reps)
            lines += [f"# 2^{log} rows, {os.path.getsize(path) / 1e6:.1f} MB, csv_ingest = {took}; the four arrays equal from_entries' of the parsed file",
                      row(f"{ctor} + root, 2^{log} rows", total, f"{reps} runs after 1"),
                      row("  np.fromfile alone", read), row("  upload alone (pageable host -> device)", upload)] + parts(path, args.sorted)
            del tree
            if args.sorted:
                lines += lookups(path, names)
    print("\n".join(lines))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
