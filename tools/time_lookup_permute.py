#!/usr/bin/env python3
"""Time the general lookup permutation (sg_lookup_permute_async_dev) on the GPU against what served such tables before it.

At rows 2^17 - 6 and 2^13 - 6, for a full-width pool of `rows` values, one of 2^16 values and an 8-bit range table:
  device     sg_lookup_permute_async_dev: HIP events around each of 20 calls after 5 warm-up calls, median per call;
  range path sg_lookup_permute_small_async_dev, the same way (range table only: it refuses the others);
  host route what the provers do for a table the range path refuses: both columns to canonical limbs on the host
             (prover._canonical_rows), prover.permute_expression_pair (the Python twin of the compiled host function), upload
             and conversion back; host clock around work that ends in a device synchronise, median of 3.
Every device result is compared with the rule (tests/lookup_permute_cases.py) before it is timed.  Prints a table; with
--out FILE also writes it there.  No GPU: fails."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import torch
    import lookup_permute_cases as lc
    import circuits_halo2_amd as sg
    from circuits_halo2_amd import arithmetic as A, ffi, prover
    assert torch.cuda.is_available(), "needs the GPU"
    ffi.check(sg.lib().sg_init(0))
    L = ffi.lib()
    stream = torch.cuda.Stream()
    status = torch.zeros(1, dtype=torch.int32, device="cuda")

    def dev(limbs):
        return A.fr_to_montgomery(torch.from_numpy(limbs.view(np.uint8).reshape(-1).copy()).cuda())

    def canon(t):
        return A.fr_from_montgomery(t).cpu().numpy().view(np.uint64).reshape(-1, 4)

    def device_ms(fn, d_inp, d_tab, rows, want):
        outs = [torch.empty(32 * rows, dtype=torch.uint8, device="cuda") for _ in range(2)]

        def call():
            ffi.check(fn(ffi.dev_ptr(d_inp), ffi.dev_ptr(d_tab), C.c_size_t(rows), ffi.dev_ptr(outs[0]), ffi.dev_ptr(outs[1]),
                         C.c_void_p(status.data_ptr()), C.c_void_p(stream.cuda_stream)))
        for _ in range(args.warmup):
            call()
        torch.cuda.synchronize()
        assert int(status.item()) == 0 and (canon(outs[0]) == want[0]).all() and (canon(outs[1]) == want[1]).all()
        events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.calls)]
        with torch.cuda.stream(stream):
            for a, b in events:
                a.record(stream)
                call()
                b.record(stream)
        torch.cuda.synchronize()
        return statistics.median(a.elapsed_time(b) for a, b in events)

    def host_ms(d_inp, d_tab, rows):
        times = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pa, ps = prover.permute_expression_pair(prover._canonical_rows(d_inp)[:rows], prover._canonical_rows(d_tab)[:rows])
            for limbs in (pa, ps):
                A.fr_to_montgomery(torch.from_numpy(limbs.view(np.uint8).reshape(-1)).cuda())
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(times)

    lines = [f"general lookup permutation, ms per call (device: median of {args.calls} event-timed calls after {args.warmup} warm-up calls; "
             "host route: median of 3, host clock)",
             "launches per device call: 103 (the head's memset, keys, 3 x 32 passes, 5 for the placement); range path: 3",
             f"{'rows':>8} {'case':<12} {'device':>9} {'range path':>11} {'host route':>11}"]
    for rows in ((1 << 17) - 6, (1 << 13) - 6):
        for name, spec in (("wide(rows)", ("wide", rows, rows, 1)), ("wide(2^16)", ("wide", rows, 1 << 16, 2)), ("range", ("range", rows, 3))):
            inp, table, want = lc.case(*spec)
            d_inp, d_tab = dev(inp), dev(table)
            t_dev = device_ms(L.sg_lookup_permute_async_dev, d_inp, d_tab, rows, want)
            t_small = device_ms(L.sg_lookup_permute_small_async_dev, d_inp, d_tab, rows, want) if name == "range" else None
            t_host = host_ms(d_inp, d_tab, rows) if name != "range" else None
            lines.append(f"{rows:>8} {name:<12} {t_dev:>9.3f} {'-' if t_small is None else format(t_small, '.3f'):>11} "
                         f"{'-' if t_host is None else format(t_host, '.1f'):>11}")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)


if __name__ == "__main__":
    main()
