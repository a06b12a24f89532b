#!/usr/bin/env python3
"""Time the batch verifier (verifier.verify_batch: sv_verify_batch) on the GPU against a loop of sp_verify_proof over the same
proofs, in the same process on the same box.

N = 64, 256 and 1024 copies of the three golden EVM proofs under the reference's key (tests/golden), cycled:
  loop     verify_proof_native on each proof in turn (one MSM launch, one host wait, one pairing check per proof);
  batch    verify_batch on all of them (one launch of 2 N small MSMs, one pairing check);
  one bad  verify_batch with one evaluation of proof N / 2 changed (bisected: about 2 log2 N pairing checks more).
Host clock around each call (every call returns its verdicts, so nothing is left in flight), median of 10 after 3 warm-up calls.
Verdicts are checked before anything is timed.  Prints a table; with --out FILE also writes it there.  No GPU: fails."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def median_ms(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--sizes", type=int, nargs="*", default=[64, 256, 1024])
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    import verify_batch_cases as VC
    from circuits_halo2_amd import ffi, verifier as V
    assert torch.cuda.is_available(), "needs the GPU"
    ffi.check(ffi.lib().sg_init(0))
    params, vk = VC.reference_key()
    lines = ["batch verifier against a loop of sp_verify_proof: golden EVM proofs (k = 11) cycled, host clock, median of "
             f"{args.calls} after {args.warmup}",
             f"{'N':>6} {'loop ms':>10} {'batch ms':>10} {'per proof us':>13} {'speed-up':>9} {'one bad ms':>11} {'pairings':>9}"]
    for n in args.sizes:
        proofs, insts = VC.cycled(n)
        bad_proofs = list(proofs)
        bad_proofs[n // 2] = VC.TAMPERS["evaluation"](proofs[n // 2], insts[n // 2])[0]
        stats = {}
        assert V.verify_batch(params, vk, proofs, insts, stats=stats) == [True] * n and stats["pairings"] == 1
        assert V.verify_batch(params, vk, bad_proofs, insts, stats=stats) == [i != n // 2 for i in range(n)]
        loop = median_ms(lambda: [V.verify_proof_native(params, vk, p, i, "evm") for p, i in zip(proofs, insts)], args.calls, args.warmup)
        batch = median_ms(lambda: V.verify_batch(params, vk, proofs, insts), args.calls, args.warmup)
        one_bad = median_ms(lambda: V.verify_batch(params, vk, bad_proofs, insts), args.calls, args.warmup)
        lines.append(f"{n:>6} {loop:>10.2f} {batch:>10.2f} {1e3 * batch / n:>13.1f} {loop / batch:>9.2f} {one_bad:>11.2f} {stats['pairings']:>9}")
        print(lines[-1], flush=True)
    params.free()
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)


if __name__ == "__main__":
    main()
