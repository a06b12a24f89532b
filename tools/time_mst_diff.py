#!/usr/bin/env python3
"""Time the next round's snapshot against a tree in HBM, on generated snapshot CSVs of 2^16 and 2^20 rows (two currencies, 16-byte
hex names; the new file B has the old file A's rows in A's order with 0 %, 1 % or 100 % of the rows carrying other balances), the
tree in file order with the name index, on one box:
  (1) diff     sr_mst_csv_diff_dev alone over preallocated buffers, HIP events and call to summary (host clock); and
               diff_csv(path): file on disk to report, host clock
  (2) apply    apply_csv(path): diff plus apply, file on disk to the tree updated, host clock; sr_mst_apply_diff_dev alone, HIP events
               and host clock.  A fresh tree each run (outside the clock); afterwards the root is from_csv(B)'s
  (3) host     the host way to the same report and update, all a tree can do at the parent commit: parse_csv_to_entries(B),
               indices_of_usernames, the leaf balances to the host and through _mont_to_int, compare, update_leaves_at
  (4) rebuild  from_csv(B, name_index=True) + root(): the other thing the parent commit can do
A tree without the feature (the parent commit: copy this file there) runs (3) and (4) alone.  Every step of every size and share
is a process of its own under `timeout`, one after the other, and the first that fails ends the run.  Warm-up, then the median,
the lowest and the highest of the runs; --out FILE writes the table there as well.  No GPU: fails."""
import argparse
import ctypes as C
import os
import random
import statistics
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NC = 2
LOGS = [16, 20]
SHARES = [0, 1, 100]
LIMIT = {"diff": 300, "apply": 420, "host": 900, "rebuild": 300}      # seconds a step's process may take
HEAD = "username,balance_ETH_ETH,balance_USDT_ETH\n"


def write_csvs(tmp, n, share):
    """A and B: the same names in the same order, every (100 / share)-th row of B with other balances -> paths, names, changed rows"""
    rng = random.Random(n)
    names = [rng.randbytes(8).hex() for _ in range(n)]
    step = 0 if not share else 100 // share
    changed = [i for i in range(n) if step and i % step == 0]
    mark = set(changed)
    pa, pb = os.path.join(tmp, "a.csv"), os.path.join(tmp, "b.csv")
    with open(pa, "w") as f:
        f.write(HEAD + "".join(f"{nm},{10 ** 9 + 7 * i},{10 ** 8 + 3 * i}\n" for i, nm in enumerate(names)))
    with open(pb, "w") as f:
        f.write(HEAD + "".join(f"{nm},{10 ** 9 + 7 * i + (5 if i in mark else 0)},{10 ** 8 + 3 * i}\n" for i, nm in enumerate(names)))
    return pa, pb, names, changed


def row(label, ms):
    return f"  {label:<72} median {statistics.median(ms):10.3f} ms   min {min(ms):10.3f} ms   max {max(ms):10.3f} ms   ({len(ms)} runs)"


def child(step, log, share):
    import numpy as np
    import torch
    from circuits_halo2_amd import ffi
    from circuits_halo2_amd import merkle_sum_tree as M
    ffi.check(ffi.lib().sg_init(0))
    n = 1 << log
    reps = 7 if log <= 16 else 5
    lines = []

    def host_clock(f, warm, runs, before=lambda: None):
        out = []
        for k in range(warm + runs):
            arg = before()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f(arg)
            torch.cuda.synchronize()
            if k >= warm:
                out.append((time.perf_counter() - t0) * 1e3)
        return out

    def device_clock(f, warm, runs, before=lambda: None):
        out = []
        for k in range(warm + runs):
            arg = before()
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            start.record()
            f(arg)
            end.record()
            end.synchronize()
            if k >= warm:
                out.append(start.elapsed_time(end))
        return out

    with tempfile.TemporaryDirectory() as tmp:
        pa, pb, names, changed = write_csvs(tmp, n, share)
        indexed = lambda: M.DeviceMerkleSumTree.from_csv(pa, NC, 8, name_index=True)
        if step == "rebuild":
            lines.append(row("(4) from_csv(B, name_index=True) + root()", host_clock(lambda _: M.DeviceMerkleSumTree.from_csv(pb, NC, 8, name_index=True).root(), 1, reps)))
        elif step == "host":
            parts = {"parse": [], "find": [], "balances": [], "update": []}

            def host_way(tree):
                t = [time.perf_counter()]
                entries, _ = M.parse_csv_to_entries(pb, NC)
                t.append(time.perf_counter())
                leaves = tree.indices_of_usernames([name for name, _ in entries])
                t.append(time.perf_counter())
                rows = tree.d_bals.cpu().numpy().reshape(-1, 32)
                at, new = [], []
                for (_, bal), leaf in zip(entries, leaves):
                    if [M._mont_to_int(rows[NC * leaf + c]) for c in range(NC)] != [v % M.R_MODULUS for v in bal]:
                        at.append(leaf)
                        new.append(bal)
                t.append(time.perf_counter())
                tree.update_leaves_at(at, new)
                torch.cuda.synchronize()
                t.append(time.perf_counter())
                assert sorted(at) == changed
                for key, a, b in zip(parts, t, t[1:]):
                    parts[key].append((b - a) * 1e3)
            total = host_clock(host_way, 0, 3, indexed)
            lines.append(row("(3) the host way: parse B, find, balances to the host, compare, update", total))
            lines += [row(f"      of which {key}", ms) for key, ms in parts.items()]
        else:
            R = ffi.rounds_lib()
            tree = indexed()
            assert tree.has_name_index and tree.csv_ingest == "device"
            t = tree._names_dev()
            scanned, reason = M.DeviceMerkleSumTree._csv_text_on_device(pb, NC)
            assert scanned is not None, reason
            text, size, body_off, delim, _, tiles, rows = scanned
            leaves, depth = 1 << tree.depth, tree.depth
            scratch = C.c_uint64(0)
            ffi.check(R.sr_mst_diff_scratch(rows, depth, C.byref(scratch)))
            i32 = lambda count: torch.empty(count, dtype=torch.int32, device="cuda")
            spans = torch.empty(rows + 2 + 2 * rows * (1 + NC), dtype=torch.int64, device="cuda")
            row_leaf, owner, listed, new, gone, work = i32(rows), i32(leaves), i32(min(rows, leaves)), i32(rows), i32(rows), i32(scratch.value // 4)
            row_state, leaf_state = (torch.empty(k, dtype=torch.uint8, device="cuda") for k in (rows, leaves))
            problem, summary = C.c_uint64(0), (C.c_uint64 * 8)()

            def diff_call(on):
                ffi.check(R.sr_mst_csv_diff_dev(ffi.dev_ptr(text), size, body_off, ffi.dev_ptr(tiles), ord(delim), NC, rows, ffi.dev_ptr(spans),
                                                ffi.dev_ptr(t["text"]), t["size"], t["body_off"], ffi.dev_ptr(t["d_name_spans"]), ffi.dev_ptr(t["d_order"]),
                                                t["n"], depth, ffi.dev_ptr(on.d_bals), ffi.dev_ptr(row_leaf), ffi.dev_ptr(row_state), ffi.dev_ptr(leaf_state),
                                                ffi.dev_ptr(owner), ffi.dev_ptr(listed), ffi.dev_ptr(new), ffi.dev_ptr(gone), rows, ffi.dev_ptr(work),
                                                C.byref(problem), summary, ffi.current_stream_ptr()))
                assert problem.value == 0 and summary[2] == len(changed) and summary[3] == n - len(changed)
            if step == "diff":
                lines.append(row("(1) sr_mst_csv_diff_dev alone, HIP events", device_clock(lambda _: diff_call(tree), 2, 2 * reps)))
                lines.append(row("(1) sr_mst_csv_diff_dev alone, call to summary", host_clock(lambda _: diff_call(tree), 2, 2 * reps)))
                lines.append(row("(1) diff_csv(B): file on disk to report", host_clock(lambda _: tree.diff_csv(pb), 1, reps)))
            else:
                want = M.DeviceMerkleSumTree.from_csv(pb, NC, 8).root()[0].tolist()

                def fresh():
                    made = indexed()
                    made.root()
                    return made

                def apply_csv(made):
                    made.apply_csv(pb)
                    assert made.root()[0].tolist() == want
                lines.append(row("(2) apply_csv(B): diff plus apply, file on disk to the new root", host_clock(apply_csv, 1, reps, fresh)))

                def diffed():
                    made = fresh()
                    diff_call(made)
                    return made

                def apply_call(made):
                    ffi.check(R.sr_mst_apply_diff_dev(ffi.dev_ptr(text), size, body_off, ffi.dev_ptr(spans), rows, ffi.dev_ptr(owner), ffi.dev_ptr(listed),
                                                      int(summary[2]), depth, NC, ffi.dev_ptr(made.d_users), ffi.dev_ptr(made.d_bals), ffi.dev_ptr(made.d_h),
                                                      ffi.dev_ptr(made.d_b), ffi.current_stream_ptr()))
                lines.append(row("(2) sr_mst_apply_diff_dev alone, HIP events", device_clock(apply_call, 1, reps, diffed)))
                lines.append(row("(2) sr_mst_apply_diff_dev alone, call to the stream's end", host_clock(apply_call, 1, reps, diffed)))
                lines.append(row("(2) both entry points, one after the other, HIP events",
                                 device_clock(lambda made: (diff_call(made), apply_call(made)), 1, reps, fresh)))
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--logs", type=int, nargs="*", default=LOGS)
    ap.add_argument("--shares", type=int, nargs="*", default=SHARES)
    ap.add_argument("--steps", nargs="*", default=None)
    ap.add_argument("--child", nargs=3, metavar=("STEP", "LOG", "SHARE"))
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], int(args.child[1]), int(args.child[2]))
    import torch
    from circuits_halo2_amd import merkle_sum_tree as M
    assert torch.cuda.is_available(), "no GPU"
    has_diff = hasattr(M.DeviceMerkleSumTree, "diff_csv")
    steps = args.steps or (["diff", "apply", "host", "rebuild"] if has_diff else ["host", "rebuild"])
    lines = [f"# the next round's CSV against a tree in HBM, {NC} currencies; {torch.cuda.get_device_name(0)}; diff_csv: "
             + ("yes" if has_diff else "no (the parent commit's tree)"),
             "# host clock but where HIP events are named; medians after warm-up; every step a process of its own"]
    print("\n".join(lines), flush=True)
    for log in args.logs:
        for share in args.shares:
            lines.append(f"2^{log} rows, {share} % of the rows with other balances")
            print(lines[-1], flush=True)
            for step in steps:
                cmd = ["timeout", "-k", "10", str(LIMIT[step]), sys.executable, os.path.abspath(__file__), "--child", step, str(log), str(share)]
                r = subprocess.run(cmd, capture_output=True, text=True)
                if r.returncode != 0:                         # a fault, a hang or a wrong result: nothing more is started
                    print(r.stdout + r.stderr[-3000:], flush=True)
                    sys.exit(f"step {step} at 2^{log}, {share} %: exit status {r.returncode}")
                lines.append(r.stdout.rstrip("\n"))
                print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
