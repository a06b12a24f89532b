#!/usr/bin/env python3
"""Time the name index beside a tree in file order and the duplicate-username report, on generated snapshot CSVs of 2^16 and 2^20
rows (two currencies, 16-byte hex names in random order, about 1 % of the rows carrying a name that another row has), in one
process on one box:
  (a) DeviceMerkleSumTree.from_csv + root()                    file on disk to tree in HBM, host clock
  (b) the same with name_index=True, and the extra HBM it keeps (the file's size plus 20 bytes a row)
  (c) ss_mst_csv_name_index_dev alone                          HIP events over preallocated buffers: the split again, the sort, the copy
  (d) the first index_of_username of a tree with the index     host clock, a fresh tree each time
  (e) indices_of_usernames of 1024 names on such a tree        host clock
  (f) the first index_of_username of a tree without it         the host parse: all a tree in file order can do at the parent commit
  (g) duplicate_names(cap=0), call to summary; duplicate_names(), everything listed; ss_mst_duplicate_names_dev alone, HIP events
  (h) the same report from `entries` on the host               the entries already parsed: (f) comes before it
A tree without the feature (the parent commit: copy this file there) runs (a) and (f) alone.  Warm-up, then the median of the
runs; --out FILE writes the table there as well.  No GPU: fails."""
import argparse
import ctypes as C
import inspect
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
from circuits_halo2_amd import merkle_sum_tree as M

NC = 2
LOGS = [16, 20]
HAS_INDEX = "name_index" in inspect.signature(M.DeviceMerkleSumTree.from_csv).parameters
HEAD = "username,balance_ETH_ETH,balance_USDT_ETH\n"


def write_csv(path, n, seed):
    """n rows; every hundredth row repeats the name of a random earlier row -> the names in file order"""
    rng = random.Random(seed)
    names = []
    for i in range(n):
        names.append(names[rng.randrange(i)] if i % 100 == 99 else rng.randbytes(8).hex())
    with open(path, "w") as f:
        f.write(HEAD + "".join(f"{nm},{10 ** 9 + 7 * i},{10 ** 8 + 3 * i}\n" for i, nm in enumerate(names)))
    return names


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


def row(label, ms):
    return f"  {label:<66} median {statistics.median(ms):10.4f} ms   min {min(ms):10.4f} ms   max {max(ms):10.4f} ms   ({len(ms)} runs)"


def first_lookup(make, name, reps):
    """the first index_of_username of a fresh tree, the tree's construction outside the clock"""
    out = []
    for _ in range(reps):
        tree = make()
        tree.root()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tree.index_of_username(name)
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def index_call(path, n):
    """-> a closure that runs ss_mst_csv_name_index_dev over preallocated buffers (the scan done once, outside)"""
    L, S = ffi.lib(), ffi.snapshot_lib()
    data = np.fromfile(path, dtype=np.uint8)
    size, body_off = int(data.size), len(HEAD)
    pad = -body_off % 16
    buf = torch.empty(pad + size, dtype=torch.uint8, device="cuda")
    buf[pad:].copy_(torch.from_numpy(data))
    text = buf[pad:]
    tiles = torch.empty(-(-(size - body_off) // 4096) + 2, dtype=torch.int32, device="cuda")
    rows, flags, problem, sort_bytes = C.c_uint64(0), C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
    ffi.check(L.sg_mst_csv_scan_dev(ffi.dev_ptr(text), size, body_off, ffi.dev_ptr(tiles), C.byref(rows), C.byref(flags), None))
    assert rows.value == n and not flags.value
    ffi.check(S.ss_mst_sort_scratch(n, C.byref(sort_bytes)))
    spans = torch.empty(2 * (n + 1 + 2 * n * (1 + NC)), dtype=torch.int64, device="cuda")
    sort = torch.empty(sort_bytes.value, dtype=torch.uint8, device="cuda")
    order, name_spans, leaf_spans = (torch.empty(k * n, dtype=torch.int32, device="cuda") for k in (1, 2, 2))
    keep = (buf, tiles, spans, sort, order, name_spans, leaf_spans)

    def call():
        ffi.check(S.ss_mst_csv_name_index_dev(ffi.dev_ptr(text), size, body_off, ffi.dev_ptr(tiles), ord(","), NC, n, ffi.dev_ptr(spans),
                                              ffi.dev_ptr(sort), ffi.dev_ptr(order), ffi.dev_ptr(name_spans), ffi.dev_ptr(leaf_spans),
                                              C.byref(problem), ffi.current_stream_ptr()))
        assert problem.value == 0 and keep
    return call


def report_call(tree, cap):
    S = ffi.snapshot_lib()
    d, n = tree._names_dev(), tree._names_dev()["n"]
    scratch_bytes = C.c_uint64(0)
    ffi.check(S.ss_mst_duplicate_names_scratch(n, C.byref(scratch_bytes)))
    scratch = torch.empty(scratch_bytes.value // 4, dtype=torch.int32, device="cuda")
    shadowed, first = (torch.empty(max(cap, 1), dtype=torch.int32, device="cuda") for _ in range(2))
    summary = (C.c_uint64 * 3)()
    return lambda: ffi.check(S.ss_mst_duplicate_names_dev(ffi.dev_ptr(d["text"]), d["size"], d["body_off"], ffi.dev_ptr(d["d_name_spans"]),
                                                          ffi.dev_ptr(d["d_order"]), n, ffi.dev_ptr(shadowed) if cap else None,
                                                          ffi.dev_ptr(first) if cap else None, cap, ffi.dev_ptr(scratch), summary,
                                                          ffi.current_stream_ptr()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--logs", type=int, nargs="*", default=LOGS)
    args = ap.parse_args()
    ffi.check(ffi.lib().sg_init(0))
    lines = [f"# names beside a tree in file order, {NC} currencies; {torch.cuda.get_device_name(0)}, one process; name index: "
             + ("yes" if HAS_INDEX else "no (the parent commit's tree)"),
             "# host clock but where HIP events are named; medians after warm-up"]
    with tempfile.TemporaryDirectory() as tmp:
        for log in args.logs:
            n = 1 << log
            path = os.path.join(tmp, f"rows_{log}.csv")
            names = write_csv(path, n, log)
            file_bytes = os.path.getsize(path)
            reps, slow = (9, 5) if log <= 16 else (5, 3)
            probe = names[n // 2]
            lines.append(f"2^{log} rows, {file_bytes} bytes, {n - len(set(names))} rows whose name an earlier row has")
            plain = lambda: M.DeviceMerkleSumTree.from_csv(path, NC, 8)
            lines.append(row("(a) from_csv + root()", host_clock(lambda: plain().root(), 1, reps)))
            if HAS_INDEX:
                indexed = lambda: M.DeviceMerkleSumTree.from_csv(path, NC, 8, name_index=True)
                lines.append(row("(b) from_csv(name_index=True) + root()", host_clock(lambda: indexed().root(), 1, reps)))
                tree = indexed()
                assert tree.has_name_index and tree.csv_ingest == "device"
                lines.append(f"      the index keeps {file_bytes + 20 * n} bytes of HBM: the file and 20 bytes a row")
                lines.append(row("(c) ss_mst_csv_name_index_dev alone, HIP events", device_clock(index_call(path, n), 2, 2 * reps)))
                lines.append(row("(d) first index_of_username, with the index", first_lookup(indexed, probe, reps)))
                rng = random.Random(5)
                batch = [names[rng.randrange(n)] for _ in range(1024)]
                first = {}
                for r, nm in enumerate(names):
                    first.setdefault(nm, r)
                assert tree.indices_of_usernames(batch) == [first[nm] for nm in batch]
                lines.append(row("(e) indices_of_usernames, 1024 names", host_clock(lambda: tree.indices_of_usernames(batch), 2, 2 * reps)))
            lines.append(row("(f) first index_of_username, without: the host parse", first_lookup(plain, probe, slow)))
            if HAS_INDEX:
                dups = tree.duplicate_names()
                lines.append(f"      the report: {dups.n_repeated_names} repeated names, {dups.n_shadowed} shadowed rows")
                lines.append(row("(g) duplicate_names(cap=0), call to summary", host_clock(lambda: tree.duplicate_names(cap=0), 2, 2 * reps)))
                lines.append(row("(g) duplicate_names(), everything listed", host_clock(lambda: tree.duplicate_names(), 2, 2 * reps)))
                lines.append(row("(g) ss_mst_duplicate_names_dev alone, cap 0, HIP events", device_clock(report_call(tree, 0), 2, 2 * reps)))
                lines.append(row("(g) ss_mst_duplicate_names_dev alone, all listed, HIP events", device_clock(report_call(tree, n), 2, 2 * reps)))
                assert tree._entries is None
                host = M._Tree.duplicate_names(tree)                 # parses: (f) once more, outside the clock
                assert (host.shadowed == dups.shadowed).all() and (host.first == dups.first).all() and host.n_repeated_names == dups.n_repeated_names
                lines.append(row("(h) the same from entries on the host, already parsed", host_clock(lambda: M._Tree.duplicate_names(tree), 0, slow)))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
