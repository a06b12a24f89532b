#!/usr/bin/env python3
"""The transform family's timings at the default parameters, one line per process (profiles/ntt_fold.txt alternates two builds of
the library with it): a lone transform at 2^11 (one pass), 2^17, 2^20 and 2^22 (sg_time_ntt_dev), and the shapes a k = 17 proof
issues -- the batched inverse transform of 5 columns and the 25 coset blocks of a phase (the timing code of tools/ab_ntt_radix4.py).
Device events around many repetitions after a warm-up call; microseconds per call.  The last field is a SHA-256 over the results
of one call of each kind on seeded inputs: two builds that compute the same print the same.  No GPU: fails."""
import ctypes as C
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import circuits_halo2_amd as sg
from circuits_halo2_amd import arithmetic as A, ffi
from circuits_halo2_amd.domain import EvaluationDomain
from circuits_halo2_amd.utils import random_fr_canonical

ffi.check(sg.lib().sg_init(0))
L = ffi.lib()
K = 17
LONE = ((11, 2000), (17, 500), (20, 100), (22, 40))     # (log_n, repetitions)


def timed(fn, reps=200):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def column(seed, k):
    return A.fr_to_montgomery(torch.from_numpy(random_fr_canonical(seed, 1 << k)).cuda())


def main():
    dom = EvaluationDomain(6, K)
    cols = [column(10 + i, K) for i in range(5)]
    digest = hashlib.sha256()
    for k, _ in LONE:
        digest.update(A.best_fft(column(50 + k, k), EvaluationDomain(2, k).get_omega(), k).cpu().numpy().tobytes())
    for out in dom.coeff_to_cosets_batch(cols):
        digest.update(out.cpu().numpy().tobytes())
    for out in A.best_fft_batch([c.clone() for c in cols], dom.get_omega_inv(), K, dom.ifft_divisor()):
        digest.update(out.cpu().numpy().tobytes())
    line = []
    for k, reps in LONE:
        a = column(90 + k, k)
        ms = C.c_float()
        ffi.check(L.sg_time_ntt_dev(ffi.dev_ptr(a), C.c_uint32(k), C.c_int(reps), C.byref(ms)))
        line.append(f"ntt_2^{k} {ms.value * 1e3:.2f}")
    line.append(f"intt_batch_5x2^{K} {timed(lambda: A.best_fft_batch(cols, dom.get_omega_inv(), K, dom.ifft_divisor())):.2f}")
    line.append(f"cosets_5_to_25x2^{K} {timed(lambda: dom.coeff_to_cosets_batch(cols)):.2f}")
    print("us:", " ".join(line), "sha256", digest.hexdigest()[:16], flush=True)


if __name__ == "__main__":
    main()
