"""GPU tests of the MSM sort front ends (csrc/msm.hip, msm_sort.cuh), all through the C ABI: the single-pass sort, the two-pass sort with
separate scans ("legacy", msm.fused_frontend = 0 or another job in flight) and the two-pass sort whose scans and task
histogram ride on its own kernels (msm.fused_frontend = 1 with the device to itself, 2 always), at the sizes they run at in
production, under skewed scalars, with jobs in flight beside them and back to back on one engine.

Every expected point comes from outside the library's MSM: the bases are s_i * G (g1_fixed_base_mul), so a generic MSM
must give <k, s> * G (oracle dot product and scalar multiplication); a commitment against ParamsKZG.setup(k, tau) must give
a(tau) * G.  Nothing compares one mode of the library with another."""
import threading

import numpy as np
import pytest

from msm_cases import _dev, _mont, case, make_pool, scalars

pytestmark = pytest.mark.gpu

N_POOL = (1 << 21) + 8
MODES = (0, 1, 2)


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    import circuits_halo2_amd as sg
    from circuits_halo2_amd import ffi
    ffi.check(sg.lib().sg_init(0))
    return sg


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def pool(gpu):
    """N_POOL bases s_i * G on the device and their discrete logs s_i (Montgomery, host); cases take slices"""
    return make_pool(N_POOL)


# ----------------------------------------------------------------------------- 1: each mode against exact answers
# (n, scalar distribution, parameters besides msm.fused_frontend, modes)
_U = [(n, "uniform", {}, MODES) for n in (1 << 15, 1 << 18, 1 << 19, 1 << 20, (1 << 20) - 1, (1 << 20) + 3, 1 << 21)]
# below 2^19 entries: the single-pass sort (msm_scatter), and the two-pass kernels forced onto it with tiny bins
_SINGLE_PASS = [(1 << 12, "uniform", {}, MODES), (1 << 14, "uniform", {}, MODES),
                (1 << 12, "equal", {}, MODES), (1 << 14, "byte", {}, MODES)]
_SMALL_TWO_PASS = [(1 << 12, "uniform", {"msm.two_pass": 2}, MODES), (1 << 14, "uniform", {"msm.two_pass": 2}, MODES),
                   (1 << 12, "equal", {"msm.two_pass": 2}, MODES), (1 << 14, "byte", {"msm.two_pass": 2}, MODES),
                   # c = 12, B = 4 bins of F = 512 buckets: a window's 2^14 equal digits share ONE bin, the smallest E > SORT_TILE
                   (1 << 14, "equal", {"msm.two_pass": 2}, MODES)]
_AT_2_20 = [(1 << 20, d, {}, MODES) for d in ("equal", "byte", "selector", "sparse", "tiled32", "pm_pairs", "s_neg_s")]
_SIGNED = [(1 << 20, "signed16", {"msm.window_bits": 16}, MODES),    # NBc = 16 windows x 256 bins = 4096
           (1 << 19, "signed13", {"msm.window_bits": 13}, MODES),    # 20 x 128 = 2560
           (1 << 20, "signed13", {"msm.window_bits": 13}, MODES),    # 20 x 256 = 5120: separate scans in every mode
           (1 << 15, "signed16", {"msm.window_bits": 16}, MODES)]
_EDGES = [(1 << 15, "equal", {}, MODES), (1 << 15, "byte", {}, MODES),
          ((1 << 20) + 3, "equal", {}, MODES), ((1 << 20) - 1, "byte", {}, MODES),
          (1 << 21, "equal", {}, (2,)), (1 << 21, "byte", {}, (2,))]    # NBc = 8192: mode 2 falls back
CASES = _U + _SINGLE_PASS + _SMALL_TWO_PASS + _AT_2_20 + _SIGNED + _EDGES


def _case_id(c):
    n, dist, extra, _ = c
    lg = (n - 1).bit_length()
    below, above = (1 << lg) - n, n - (1 << (lg - 1))
    size = f"2^{lg}" if not below else (f"2^{lg}-{below}" if below < above else f"2^{lg - 1}+{above}")
    return "-".join([size, dist] + [f"{k.split('.')[1]}{v}" for k, v in extra.items()])


@pytest.mark.parametrize("n,dist,extra,modes", CASES, ids=[_case_id(c) for c in CASES])
def test_msm_front_ends_known_answer(gpu, O, pool, n, dist, extra, modes):
    """one MSM per front-end mode (msm.fused_frontend 0 / 1 / 2) against <k, s> G: the single-pass sort below 2^19 entries,
    the two-pass sort with separate scans and with the fused ones, at the headline's NBc = 4096 bins and past it, at lengths
    that are not powers of two, under every skew the sort has a branch for (oversized bins, empty bins, deep buckets,
    cancelling points) and at the edges of the signed-digit recoding"""
    from circuits_halo2_amd import ffi
    from circuits_halo2_amd.arithmetic import best_multiexp
    seed = 1000 * len(dist) + n % 9973 + 17 * sum(extra.values())
    k, bases, want = case(O, pool, dist, n, seed, off=seed % 8)
    bad = []
    for mode in modes:
        with ffi.params({"msm.fused_frontend": mode, **extra}):
            got = best_multiexp(k, bases)
        if not (got == want).all():
            bad.append(mode)
    assert not bad, f"wrong point in mode(s) {bad}"


# ----------------------------------------------------------------------------- 2: other jobs in flight
def _overlapped(log):
    return any(r["jobs_in_flight"] >= 2 for r in log)


@pytest.mark.parametrize("mode", [1, 2])
def test_three_threads_in_flight(gpu, O, pool, mode):
    """three host threads, each with blocking MSMs of 2^20 on device tensors (the bench's three in flight), four rounds
    started together: mode 1 takes the separate scans while the others run, mode 2 the fused ones regardless"""
    import torch
    from circuits_halo2_amd import arithmetic as A, ffi
    n, rounds = 1 << 20, 4
    cases = [case(O, pool, d, n, 300 + i, off=i) for i, d in enumerate(("uniform", "equal", "sparse"))]
    barrier = threading.Barrier(len(cases))
    got = [[] for _ in cases]
    errors = []

    def run(i):
        try:
            ffi.bind_thread()
            with torch.cuda.stream(torch.cuda.Stream()):
                for _ in range(rounds):
                    barrier.wait(timeout=120)
                    got[i].append(A.best_multiexp(cases[i][0], cases[i][1]))
        except BaseException as e:   # (reported below)
            errors.append(e)
            barrier.abort()

    with ffi.params({"msm.fused_frontend": mode, "msm.acc_log": 1}):
        threads = [threading.Thread(target=run, args=(i,), daemon=True) for i in range(len(cases))]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=300)
        log = ffi.msm_launch_log()
    assert not any(t.is_alive() for t in threads) and not errors, errors
    for i, (_, _, want) in enumerate(cases):
        assert len(got[i]) == rounds and all((p == want).all() for p in got[i]), (i, mode)
    assert _overlapped(log), "the three threads never had two jobs in flight"


@pytest.mark.parametrize("mode", MODES)
def test_batch_in_flight_and_fused_groups(gpu, O, pool, mode):
    """best_multiexp_batch on device tensors: groups alternate between the lane's two engines, so each group's front end runs
    while the previous one is in flight; then 6 equal MSMs of 2^17 (one fused job of 6 x 20 windows x 32 bins = 3840 <= 4096
    bins) and 7 (4480: separate scans in every mode)"""
    from circuits_halo2_amd import arithmetic as A, ffi
    sizes = [1 << 20, 1 << 18, 1 << 20, 1 << 19, 1 << 15]
    dists = ["uniform", "selector", "equal", "byte", "sparse"]
    mixed = [case(O, pool, d, n, 400 + i, off=i) for i, (n, d) in enumerate(zip(sizes, dists))]
    members = ["uniform", "equal", "byte", "selector", "sparse", "tiled32", "uniform"]
    fused = [case(O, pool, d, 1 << 17, 500 + i, off=(1 << 17) * i) for i, d in enumerate(members)]
    with ffi.params({"msm.fused_frontend": mode, "msm.acc_log": 1}):
        got = A.best_multiexp_batch([(k, b) for k, b, _ in mixed])
        log = ffi.msm_launch_log()
        ffi.set_param("msm.acc_log", 1)
        got6 = A.best_multiexp_batch([(k, b) for k, b, _ in fused[:6]])
        got7 = A.best_multiexp_batch([(k, b) for k, b, _ in fused])
        log67 = ffi.msm_launch_log()
    for i, (g, (_, _, want)) in enumerate(zip(got, mixed)):
        assert (g == want).all(), ("mixed", i)
    for i, (g, (_, _, want)) in enumerate(zip(got6, fused)):
        assert (g == want).all(), ("6 x 2^17", i)
    for i, (g, (_, _, want)) in enumerate(zip(got7, fused)):
        assert (g == want).all(), ("7 x 2^17", i)
    assert sorted(r["n"] for r in log) == sorted(sizes)
    assert _overlapped(log), "the batch's groups never overlapped"
    assert [(r["n"], r["M"]) for r in log67] == [(1 << 17, 6), (1 << 17, 7)]   # one job each: the bin counts above hold


def test_back_to_back_jobs_on_one_engine(gpu, O, pool):
    """jobs of different sizes and skews one after the other on one engine, switching front-end modes on the way (2 -> 0 ->
    2 -> 1): the fused front end's two replica sets alternate by job, each job clears the other set for the next one even
    when that one has a different bin count, and msm_hist_prefix's finished-workgroup counter must be back at zero"""
    from circuits_halo2_amd import ffi
    from circuits_halo2_amd.arithmetic import best_multiexp
    seq = [(1 << 15, "uniform"), (1 << 20, "equal"), (1 << 17, "selector"), (1 << 20, "uniform"), (1 << 15, "byte")] * 2
    modes = [2, 2, 2, 0, 0, 2, 2, 2, 1, 1]
    cases = [case(O, pool, d, n, 600 + i, off=i % 8) for i, (n, d) in enumerate(seq)]
    bad = []
    for i, ((k, b, want), mode) in enumerate(zip(cases, modes)):
        with ffi.params({"msm.fused_frontend": mode}):
            if not (best_multiexp(k, b) == want).all():
                bad.append((i, seq[i], mode))
    # the same sequence once more with the default mode throughout: nothing stale from the switching above
    for i, (k, b, want) in enumerate(cases):
        if not (best_multiexp(k, b) == want).all():
            bad.append((i, seq[i], "default"))
    assert not bad, bad


# ----------------------------------------------------------------------------- fixed base (commitments) at k = 17
K_FIXED = 17


@pytest.fixture(scope="module")
def kzg(gpu, O):
    """ParamsKZG.setup(17, tau) and nine columns of 2^17 rows: column i is coefficients (i % 3 == 0), Lagrange (1) or a
    piecewise-constant Lagrange column committed in difference form (2); `want` from a(tau) G"""
    from circuits_halo2_amd.utils import random_fr_canonical
    n = 1 << K_FIXED
    tau = O.fr_to_mont(random_fr_canonical(0x7A0, 1))
    params = gpu.ParamsKZG.setup(K_FIXED, tau)
    rng = np.random.default_rng(17)
    dists = ["uniform", "byte", None, "selector", "uniform", None, "sparse", "equal", None]
    cols, kinds, want = [], [], []
    for i, d in enumerate(dists):
        if d is None:   # runs of equal values (a running balance): few non-zero differences
            runs = np.sort(rng.choice(n, size=40, replace=False))
            vals = random_fr_canonical(800 + i, 41).reshape(41, 32)
            canon = vals[np.searchsorted(runs, np.arange(n), side="right")].reshape(-1)
        else:
            canon = scalars(d, n, 800 + i)
        dev, host = _mont(canon)
        kind = i % 3
        coeffs = host if kind == 0 else O.lagrange_to_coeff(host, K_FIXED, O.ncpu())
        cols.append(dev)
        kinds.append(kind)
        want.append(O.g1_mul(O.g1_generator(), O.fr_eval_poly(coeffs, tau)))
    yield {"params": params, "cols": cols, "kinds": kinds, "want": want}
    params.free()


def _fixed_round(kzg, counts=(1, 5, 8, 9)):
    """commit, commit_lagrange, commit_batch (plain and difference form) and commit_batch_mixed of 1, 5, 8 (NBc = 8 x 512
    = 4096 once the window tables exist) and 9 (4608) columns; returns the failures"""
    p, cols, kinds, want = kzg["params"], kzg["cols"], kzg["kinds"], kzg["want"]
    bad = []
    if not (p.commit(cols[0]) == want[0]).all():
        bad.append("commit")
    if not (p.commit_lagrange(cols[1]) == want[1]).all():
        bad.append("commit_lagrange")
    lag = [i for i in range(len(cols)) if kinds[i]]
    coef = [i for i in range(len(cols)) if not kinds[i]]
    for name, idx, kw in (("batch coeff", coef, {}), ("batch lagrange", lag, {"lagrange": True}),
                          ("batch diff", lag, {"lagrange": True, "diff": True})):
        got = p.commit_batch([cols[i] for i in idx], **kw)
        bad += [(name, i) for g, i in zip(got, idx) if not (g == want[i]).all()]
    for m in counts:
        got = p.commit_batch_mixed(cols[:m], kinds[:m])
        bad += [("mixed", m, i) for i in range(m) if not (got[i] == want[i]).all()]
    return bad


@pytest.mark.parametrize("mode", MODES)
def test_fixed_base_commitments_at_k17(gpu, kzg, mode):
    """commitments of 2^17 rows against a(tau) G, first over the resident bases (generic fused jobs: 640 bins per column)
    and then over the window tables (fixed-base jobs: 512 bins per column, 8 columns = FE_MAX_BINS, 9 past it)"""
    from circuits_halo2_amd import ffi
    p = kzg["params"]
    p.free()                     # (a fresh upload: no window tables from an earlier test)
    with ffi.params({"msm.fused_frontend": mode}):
        bad = [("generic",) + (b if isinstance(b, tuple) else (b,)) for b in _fixed_round(kzg)]
        p.precompute()
        bad += [("fixed",) + (b if isinstance(b, tuple) else (b,)) for b in _fixed_round(kzg)]
    assert not bad, bad


def test_fixed_base_beside_generic_msm(gpu, O, pool, kzg):
    """mode 2: commitment jobs (fixed base, 8 columns: NBc = 4096) on one thread while another thread runs generic MSMs of
    2^20, both fused front ends at once on different lanes; rounds started together"""
    import torch
    from circuits_halo2_amd import arithmetic as A, ffi
    p, cols, kinds, want = kzg["params"], kzg["cols"], kzg["kinds"], kzg["want"]
    p.precompute()
    k, b, want_g = case(O, pool, "uniform", 1 << 20, 900, off=5)
    rounds = 4
    barrier = threading.Barrier(2)
    got_g, errors = [], []

    def generic():
        try:
            ffi.bind_thread()
            with torch.cuda.stream(torch.cuda.Stream()):
                for _ in range(rounds):
                    barrier.wait(timeout=120)
                    got_g.append(A.best_multiexp(k, b))
        except BaseException as e:
            errors.append(e)
            barrier.abort()

    got_f = []
    with ffi.params({"msm.fused_frontend": 2, "msm.acc_log": 1}):
        t = threading.Thread(target=generic, daemon=True)
        t.start()
        try:
            for _ in range(rounds):
                barrier.wait(timeout=120)
                got_f.append(p.commit_batch_mixed(cols[:8], kinds[:8]))
        finally:
            t.join(timeout=300)
        log = ffi.msm_launch_log()
    assert not t.is_alive() and not errors, errors
    assert len(got_g) == rounds and all((g == want_g).all() for g in got_g)
    assert all((g[i] == want[i]).all() for g in got_f for i in range(8))
    assert any(r["fixed"] == 1 for r in log) and any(r["fixed"] == 0 for r in log)
    assert _overlapped(log), "the fixed-base and generic jobs never overlapped"


@pytest.mark.parametrize("chunks", [2, 4])
def test_host_pointer_msm_in_chunks_fused(gpu, O, pool, chunks):
    """sg_msm_g1 from host memory at 2^19 in 2 and 4 chunks (jobs on the lane's two engines, declared in flight for the
    whole call) with the fused front end forced (mode 2), uniform and all-equal scalars"""
    import ctypes as C
    from circuits_halo2_amd import ffi
    L = ffi.lib()
    n = 1 << 19
    out = np.zeros(64, dtype=np.uint8)
    for i, dist in enumerate(("uniform", "equal")):
        k, b, want = case(O, pool, dist, n, 1000 + 10 * chunks + i, off=i)
        hk, hb = k.cpu().numpy().copy(), b.cpu().numpy().copy()
        with ffi.params({"msm.fused_frontend": 2, "msm.host_chunks": chunks, "msm.acc_log": 1}):
            ffi.check(L.sg_msm_g1(ffi.ptr(hk), ffi.ptr(hb), C.c_size_t(n), ffi.ptr(out)))
            log = ffi.msm_launch_log()
        assert (out == want).all(), (chunks, dist)
        assert len(log) == chunks and _overlapped(log)


# ----------------------------------------------------------------------------- 3: nothing left behind
def test_defaults_after_the_module(gpu, O):
    """(last in the file) every parameter reads back its documented default (include/summa_gpu.h), and a fresh MSM of 2^16
    still matches the oracle"""
    from param_doc import documented_defaults
    from circuits_halo2_amd import ffi
    from circuits_halo2_amd.arithmetic import best_multiexp
    defaults = documented_defaults()
    assert len(defaults) >= 40 and {"msm.acc_log", "msm.host_chunks", "msm.fused_frontend", "msm.two_pass"} <= set(defaults)
    assert {name: ffi.get_param(name) for name in defaults} == defaults
    n = 1 << 16
    sc = O.random_fr(0x16, n)
    bases = O.fixed_base_mul(O.random_fr(0x61, n), O.ncpu())
    assert (best_multiexp(_dev(sc), _dev(bases)) == O.best_multiexp(sc, bases, O.ncpu())).all()
