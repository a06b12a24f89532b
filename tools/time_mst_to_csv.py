#!/usr/bin/env python3
"""Time a tree in HBM written back out as its snapshot CSV, on generated snapshot CSVs of 2^16 and 2^20 rows (two currencies, 16-byte
hex names), the tree in file order with the name index, un-updated or with 1 % of its leaves given other balances by
update_leaves_at, on one box:
  (1) device   sx_mst_csv_measure_dev alone and sx_mst_csv_write_dev alone over preallocated buffers, HIP events, each against the
               floor of the bytes it must move at HBM peak (measure: the balances and the spans in, the positions out; write: the
               balances, the spans, the positions and the names in, the text out); and to_csv(path): call to file on disk, host
               clock.  The file is checked once: from_csv of it has the tree's root
  (2) host     the only way the parent commit has to the same file: tree.entries (parse_csv_to_entries of the source on the host,
               the updated leaves put in), then a Python join and one write, host clock.  A fresh tree each run (outside the clock)
A tree without the feature (the parent commit: copy this file there) runs (2) alone.  Every step of every size and share is a
process of its own under `timeout`, one after the other, and the first that fails ends the run.  Warm-up, then the median, the
lowest and the highest of the runs; --out FILE writes the table there as well.  No GPU: fails."""
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

NC, HBM_PEAK = 2, 8e12
LOGS = [16, 20]
SHARES = [0, 1]
LIMIT = {"device": 300, "host": 600}      # seconds a step's process may take
HEAD = "username,balance_ETH_ETH,balance_USDT_ETH\n"


def write_csv(tmp, n):
    rng = random.Random(n)
    names = [rng.randbytes(8).hex() for _ in range(n)]
    path = os.path.join(tmp, "a.csv")
    with open(path, "w") as f:
        f.write(HEAD + "".join(f"{nm},{10 ** 9 + 7 * i},{10 ** 8 + 3 * i}\n" for i, nm in enumerate(names)))
    return path


def row(label, ms, floor_us=None):
    line = f"  {label:<64} median {statistics.median(ms):10.3f} ms   min {min(ms):10.3f} ms   max {max(ms):10.3f} ms   ({len(ms)} runs)"
    if floor_us is not None:
        line += f"   = {statistics.median(ms) * 1e3 / floor_us:6.1f} x the {floor_us:.2f} us of its bytes at HBM peak"
    return line


def child(step, log, share):
    import torch
    from circuits_halo2_amd import ffi
    from circuits_halo2_amd import merkle_sum_tree as M
    ffi.check(ffi.lib().sg_init(0))
    n = 1 << log
    reps = 9 if log <= 16 else 7
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

    def device_clock(f, warm, runs):
        out = []
        for k in range(warm + runs):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            start.record()
            f()
            end.record()
            end.synchronize()
            if k >= warm:
                out.append(start.elapsed_time(end))
        return out

    with tempfile.TemporaryDirectory() as tmp:
        src, out = write_csv(tmp, n), os.path.join(tmp, "out.csv")
        step_rows = 100 // share if share else 0
        at = [i for i in range(n) if step_rows and i % step_rows == 0]

        def fresh():
            tree = M.DeviceMerkleSumTree.from_csv(src, NC, 8, name_index=True)
            if at:
                tree.update_leaves_at(at, [[10 ** 9 + 7 * i + 5, 3] for i in at])
            tree.root()
            return tree
        if step == "host":
            def host_way(tree):
                rows = [",".join([name] + [str(v % M.R_MODULUS) for v in bal]) for name, bal in tree.entries if name is not None]
                with open(out, "w") as f:
                    f.write(HEAD + "".join(r + "\n" for r in rows))
            lines.append(row("(2) the parent's way: tree.entries, a Python join, one write", host_clock(host_way, 0, 3, fresh)))
        else:
            X = ffi.export_lib()
            tree = fresh()
            assert tree.has_name_index and tree.csv_ingest == "device"
            t = tree._names_dev()
            scratch, total = C.c_uint64(0), C.c_uint64(0)
            ffi.check(X.sx_mst_csv_scratch(n, C.byref(scratch)))
            row_off = torch.empty(n, dtype=torch.int32, device="cuda")
            work = torch.empty(scratch.value // 4, dtype=torch.int32, device="cuda")
            inputs = (ffi.dev_ptr(t["text"]), t["size"], t["body_off"], ffi.dev_ptr(t["d_leaf_name_spans"]), n, NC, ffi.dev_ptr(tree.d_bals))

            def measure():
                ffi.check(X.sx_mst_csv_measure_dev(*inputs, ffi.dev_ptr(row_off), ffi.dev_ptr(work), C.byref(total), ffi.current_stream_ptr()))
            measure()
            body = torch.empty(total.value, dtype=torch.uint8, device="cuda")

            def write():
                ffi.check(X.sx_mst_csv_write_dev(*inputs, ord(","), ffi.dev_ptr(row_off), total.value, ffi.dev_ptr(body), ffi.current_stream_ptr()))
            names = 16 * n
            measure_floor = (32 * NC * n + 8 * n + 4 * n) / HBM_PEAK * 1e6
            write_floor = (32 * NC * n + 8 * n + 4 * n + names + total.value) / HBM_PEAK * 1e6
            lines.append(f"  the body: {total.value} bytes")
            lines.append(row("(1) sx_mst_csv_measure_dev alone, HIP events (one 8-byte copy inside)", device_clock(measure, 3, 3 * reps), measure_floor))
            lines.append(row("(1) sx_mst_csv_write_dev alone, HIP events", device_clock(write, 3, 3 * reps), write_floor))
            lines.append(row("(1) both, call to the stream's end", host_clock(lambda _: (measure(), write()), 2, 2 * reps)))
            lines.append(row("(1) to_csv(path): call to file on disk", host_clock(lambda _: tree.to_csv(out), 1, reps)))
            back = M.DeviceMerkleSumTree.from_csv(out, NC, 8)
            assert all((a == b).all() for a, b in zip(back.root(), tree.root())), "the file does not read back to the tree's root"
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
    has_export = hasattr(M.DeviceMerkleSumTree, "to_csv")
    steps = args.steps or (["device", "host"] if has_export else ["host"])
    lines = [f"# a tree in HBM written back out as its snapshot CSV, {NC} currencies; {torch.cuda.get_device_name(0)}; to_csv: "
             + ("yes" if has_export else "no (the parent commit's tree)"),
             "# host clock but where HIP events are named; medians after warm-up; every step a process of its own"]
    print("\n".join(lines), flush=True)
    for log in args.logs:
        for share in args.shares:
            lines.append(f"2^{log} rows, {share} % of the leaves with other balances")
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
