#!/usr/bin/env python3
"""Time a round settled in full on a tree in HBM against the rebuild, on generated snapshot CSVs: a tree of 10^6 rows in file order
with the name index (two currencies, 16-byte hex names, from a file on disk), and the next round's file B with 1 % of the rows
carrying other balances, 0.5 % of the users gone and 1 % or 0.01 % new users spread over the file, on one box:
  (1) settle   apply_csv(B, admit_new=True, zero_gone=True): file on disk to the synchronized root, host clock.  A fresh tree each
               run (outside the clock); afterwards `to_csv` of the tree, read back by from_csv, has the tree's root
  (2) calls    the device time by step, HIP events and host clock: sr_mst_csv_diff_dev, sa_mst_admit_measure_dev (the lengths, the
               one wait, then the sort of B's names and the sorted NEW list) and sa_mst_settle_dev (merge, names, pack, leaves and
               levels), each alone over the buffers the step before left; and sa_mst_settle_dev once more with nobody admitted
               (pack, leaves and levels of the changed and gone leaves) and for the changed leaves alone: the differences are the
               shares of the merge with the names and of the gone leaves
  (3) rebuild  from_csv(B, name_index=True) + root() of the new round's own file: the other thing a caller can do, and all the
               parent commit can (copy this file there: it runs (3) alone)
Every step of every share is a process of its own under `timeout`; settle and rebuild alternate, --rounds times each, and the
first process that fails ends the run.  Warm-up, then the median, the lowest and the highest of the runs; --out FILE writes the
table there as well.  No GPU: fails."""
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
ROWS = 10 ** 6
CHANGED, GONE = 100, 200                                     # every 100th row changed, every 200th user gone
NEW_SHARES = ["1", "0.01"]                                   # per cent of ROWS
LIMIT = {"settle": 420, "calls": 420, "rebuild": 300}        # seconds a step's process may take
HEAD = "username,balance_ETH_ETH,balance_USDT_ETH\n"


def write_csvs(tmp, n, n_new):
    """A, and B: A's rows in A's order, every CHANGED-th with other balances, every GONE-th (offset 7) left out, n_new fresh names
    spread evenly -> paths, the counts (changed, gone, new)"""
    rng = random.Random(n)
    names = [rng.randbytes(8).hex() for _ in range(n)]
    fresh = [rng.randbytes(8).hex() + "n" for _ in range(n_new)]
    pa, pb = os.path.join(tmp, "a.csv"), os.path.join(tmp, "b.csv")
    with open(pa, "w") as f:
        f.write(HEAD + "".join(f"{nm},{10 ** 9 + 7 * i},{10 ** 8 + 3 * i}\n" for i, nm in enumerate(names)))
    every = max(1, n // max(1, n_new))
    changed = gone = k = 0
    with open(pb, "w") as f:
        f.write(HEAD)
        for i, nm in enumerate(names):
            if i % every == 0 and k < n_new:
                f.write(f"{fresh[k]},{k + 1},{2 * k + 1}\n")
                k += 1
            if i % GONE == 7:
                gone += 1
                continue
            bump = 5 if i % CHANGED == 0 else 0
            changed += bool(bump)
            f.write(f"{nm},{10 ** 9 + 7 * i + bump},{10 ** 8 + 3 * i}\n")
    assert k == n_new
    return pa, pb, (changed, gone, n_new)


def row(label, ms):
    return f"  {label:<78} median {statistics.median(ms):10.3f} ms   min {min(ms):10.3f} ms   max {max(ms):10.3f} ms   ({len(ms)} runs)"


def child(step, n, n_new, reps):
    import torch
    from circuits_halo2_amd import ffi
    from circuits_halo2_amd import merkle_sum_tree as M
    ffi.check(ffi.lib().sg_init(0))
    lines = []

    def clock(f, warm, runs, before=lambda: None, events=False):
        out = []
        for k in range(warm + runs):
            arg = before()
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            start.record()
            f(arg)
            end.record()
            torch.cuda.synchronize()
            if k >= warm:
                out.append(start.elapsed_time(end) if events else (time.perf_counter() - t0) * 1e3)
        return out

    with tempfile.TemporaryDirectory() as tmp:
        pa, pb, (n_changed, n_gone, _) = write_csvs(tmp, n, n_new)
        indexed = lambda: M.DeviceMerkleSumTree.from_csv(pa, NC, 8, name_index=True)

        def fresh():
            made = indexed()
            made.root()
            return made
        if step == "rebuild":
            lines.append(row("(3) from_csv(B, name_index=True) + root()", clock(lambda _: M.DeviceMerkleSumTree.from_csv(pb, NC, 8, name_index=True).root(), 1, reps)))
        elif step == "settle":
            def settle(made):
                diff = made.apply_csv(pb, admit_new=True, zero_gone=True)
                made.root()
                assert (diff.n_changed, diff.n_gone, diff.n_new) == (n_changed, n_gone, n_new) and diff.ingest == "device"
            lines.append(row("(1) apply_csv(B, admit_new, zero_gone): file on disk to the new root", clock(settle, 1, reps, fresh)))
            made = fresh()
            settle(made)
            out = os.path.join(tmp, "settled.csv")
            assert made.to_csv(out).n_rows == n + n_new
            assert M.DeviceMerkleSumTree.from_csv(out, NC, 8).root()[0].tolist() == made.root()[0].tolist()
        else:
            R, A = ffi.rounds_lib(), ffi.admit_lib()
            scanned, reason = M.DeviceMerkleSumTree._csv_text_on_device(pb, NC)
            assert scanned is not None, reason
            text, size, body_off, delim, _, tiles, rows = scanned
            tree = fresh()
            depth, leaves, n_tree = tree.depth, 1 << tree.depth, tree._names_dev()["n"]
            scratch, admit_scratch = C.c_uint64(0), C.c_uint64(0)
            ffi.check(R.sr_mst_diff_scratch(rows, depth, C.byref(scratch)))
            ffi.check(A.sa_mst_admit_scratch(rows, NC, n_new, C.byref(admit_scratch)))
            i32 = lambda count: torch.empty(count, dtype=torch.int32, device="cuda")
            u8 = lambda count: torch.empty(count, dtype=torch.uint8, device="cuda")
            spans = torch.empty(rows + 2 + 2 * rows * (1 + NC), dtype=torch.int64, device="cuda")
            row_leaf, owner, listed, new, gone, work = i32(rows), i32(leaves), i32(min(rows, leaves)), i32(rows), i32(leaves), i32(scratch.value // 4)
            row_state, leaf_state, admit_work = u8(rows), u8(leaves), u8(admit_scratch.value)
            problem, summary, name_bytes = C.c_uint64(0), (C.c_uint64 * 8)(), C.c_uint64(0)
            p = ffi.dev_ptr

            def diff_call(on):
                t = on._names_dev()
                ffi.check(R.sr_mst_csv_diff_dev(p(text), size, body_off, p(tiles), ord(delim), NC, rows, p(spans), p(t["text"]), t["size"],
                                                t["body_off"], p(t["d_name_spans"]), p(t["d_order"]), t["n"], depth, p(on.d_bals), p(row_leaf),
                                                p(row_state), p(leaf_state), p(owner), p(listed), p(new), p(gone), max(rows, leaves), p(work),
                                                C.byref(problem), summary, ffi.current_stream_ptr()))
                assert problem.value == 0 and (summary[2], summary[4], summary[0]) == (n_changed, n_gone, n_new)

            def measure_call(on):
                ffi.check(A.sa_mst_admit_measure_dev(p(text), size, body_off, p(spans), rows, NC, p(row_state), p(new), n_new, n_tree, depth,
                                                     p(admit_work), C.byref(name_bytes), C.byref(problem), ffi.current_stream_ptr()))
                assert problem.value == 0

            def settle_call(on):
                t, n_all = on._names_dev(), n_tree + n_new
                outs = (u8(t["size"] + name_bytes.value), i32(2 * n_all), i32(n_all), i32(2 * n_all))
                ffi.check(A.sa_mst_settle_dev(p(text), size, body_off, p(spans), rows, NC, p(owner), p(leaf_state), p(listed), n_changed, p(gone),
                                              n_gone, p(new), n_new, p(admit_work), p(t["text"]), t["size"], t["body_off"], p(t["d_name_spans"]),
                                              p(t["d_order"]), p(t["d_leaf_name_spans"]), n_tree, depth, p(outs[0]), name_bytes.value, p(outs[1]),
                                              p(outs[2]), p(outs[3]), p(on.d_users), p(on.d_bals), p(on.d_h), p(on.d_b), ffi.current_stream_ptr()))
                return outs

            def part_call(on, gone_count):
                """pack, leaves and levels alone: no merge, no names"""
                ffi.check(A.sa_mst_settle_dev(p(text), size, body_off, p(spans), rows, NC, p(owner), p(leaf_state), p(listed), n_changed,
                                              p(gone) if gone_count else None, gone_count, None, 0, None, None, 0, 0, None, None, None, n_tree, depth,
                                              None, 0, None, None, None, p(on.d_users), p(on.d_bals), p(on.d_h), p(on.d_b), ffi.current_stream_ptr()))
            for events, how in ((True, "HIP events"), (False, "host clock")):
                lines.append(row(f"(2) sr_mst_csv_diff_dev alone, {how}", clock(diff_call, 1, reps, lambda: tree, events)))
                lines.append(row(f"(2) sa_mst_admit_measure_dev alone (lengths, wait, sort, NEW list), {how}", clock(measure_call, 1, reps, lambda: tree, events)))

                def measured():
                    made = fresh()
                    diff_call(made)
                    measure_call(made)
                    return made
                lines.append(row(f"(2) sa_mst_settle_dev alone (merge, names, pack, leaves, levels), {how}", clock(settle_call, 1, reps, measured, events)))
                lines.append(row(f"(2)   the same call for the changed and gone leaves, nobody admitted, {how}", clock(lambda on: part_call(on, n_gone), 1, reps, measured, events)))
                lines.append(row(f"(2)   the same call for the changed leaves alone, {how}", clock(lambda on: part_call(on, 0), 1, reps, measured, events)))
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--rows", type=int, default=ROWS)
    ap.add_argument("--new", nargs="*", default=NEW_SHARES, help="new users in per cent of the rows")
    ap.add_argument("--steps", nargs="*", default=None)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--child", nargs=4, metavar=("STEP", "ROWS", "NEW", "REPS"))
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], int(args.child[1]), int(args.child[2]), int(args.child[3]))
    import torch
    from circuits_halo2_amd import merkle_sum_tree as M
    assert torch.cuda.is_available(), "no GPU"
    import inspect
    has_admit = "admit_new" in inspect.signature(M.DeviceMerkleSumTree.apply_csv).parameters if hasattr(M.DeviceMerkleSumTree, "apply_csv") else False
    steps = args.steps or (["settle", "rebuild"] * args.rounds + ["calls"] if has_admit else ["rebuild"] * args.rounds)
    lines = [f"# a round settled in full on a tree of {args.rows} rows in HBM against the rebuild, {NC} currencies; {torch.cuda.get_device_name(0)}; "
             "admit_new: " + ("yes" if has_admit else "no (the parent commit's tree)"),
             f"# B: every {CHANGED}th row changed, every {GONE}th user gone, new users as given; host clock but where HIP events are named; "
             "medians after warm-up; every step a process of its own, settle and rebuild alternating"]
    print("\n".join(lines), flush=True)
    for share in args.new:
        n_new = max(1, round(args.rows * float(share) / 100))
        lines.append(f"{args.rows} rows, {share} % new users ({n_new})")
        print(lines[-1], flush=True)
        for step in steps:
            cmd = ["timeout", "-k", "10", str(LIMIT[step]), sys.executable, os.path.abspath(__file__), "--child", step, str(args.rows), str(n_new),
                   str(args.reps)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:                             # a fault, a hang or a wrong result: nothing more is started
                print(r.stdout + r.stderr[-3000:], flush=True)
                sys.exit(f"step {step} at {share} % new: exit status {r.returncode}")
            lines.append(r.stdout.rstrip("\n"))
            print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
