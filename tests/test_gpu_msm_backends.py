"""GPU tests of the MSM back end (csrc/msm.hip, msm_accumulate.cuh, msm_reduce.cuh), all through the C ABI: msm_accumulate at every workgroup size, wave count and
task length, the merge rounds, and every bucket-reduction path -- the scan reduction (msm_reduce_buckets<1> / <4> / _lean<1>,
msm_reduce_items<1> / <4>), the 2-D reduction with the powers of two on the host (msm_fold_buckets, msm_reduce2d_lines_folded,
msm_reduce2d_lines, msm_reduce2d_bits) and on the device (msm_reduce2d_combine) -- with the host tail behind each, forced by
runtime parameters where the defaults never go.  Each case says which path it is for; `expected_backend` (tests/msm_cases.py,
the decision rules of csrc/msm_plan.h restated) must agree before the MSM runs.

Every expected point comes from outside the library's MSM: the bases are s_i * G with known s_i, so an MSM must give
<k, s> * G (oracle dot product and scalar multiplication); a commitment against ParamsKZG.setup(k, tau) must give a(tau) * G.
Nothing compares one setting of the library with another.  Buckets with prescribed populations and the group-law edge cases
come from tests/msm_cases.py, where test_msm_cases_cpu.py checks them without a GPU."""
import ctypes as C
import itertools
import threading

import numpy as np
import pytest

import msm_cases as mc
from msm_cases import EDGE_WIDTHS, POPULATIONS, _dev, _ints, _mont, case_with_scalars, edge_cases, expected_backend

pytestmark = pytest.mark.gpu

N_POOL = (1 << 20) + 8
MQT_DEFAULT = 0x7fffffff
# how the reduction paths are forced (msm.*), and the level-0 / line-sum kernel each must dispatch
SCAN_PATHS = {"scan1": ({"red2d": 0, "quad": 0, "red_lean": 0}, "msm_reduce_buckets<1>"),
              "scan4": ({"red2d": 0, "quad": 2}, "msm_reduce_buckets<4>"),
              "lean": ({"red2d": 0, "quad": 0, "red_lean": 2}, "msm_reduce_buckets_lean<1>")}
DEVICE_2D = {"dev2d-fold1": ({"red2d": 2, "red2d_prefold": 1, "quad": 0}, "msm_reduce2d_lines_folded<1>"),
             "dev2d-fold4": ({"red2d": 2, "red2d_prefold": 1, "quad": 2}, "msm_reduce2d_lines_folded<4>"),
             "dev2d-lines1": ({"red2d": 2, "red2d_prefold": 0, "quad": 0}, "msm_reduce2d_lines<1>"),
             "dev2d-lines4": ({"red2d": 2, "red2d_prefold": 0, "quad": 2}, "msm_reduce2d_lines<4>")}
HOST_2D = {"host2d-fold1": ({"red2d": 1, "red2d_prefold": 1, "quad": 0}, "msm_reduce2d_lines_folded<1>"),
           "host2d-fold4": ({"red2d": 1, "red2d_prefold": 1, "quad": 2}, "msm_reduce2d_lines_folded<4>"),
           "host2d-lines1": ({"red2d": 1, "red2d_prefold": 0, "quad": 0}, "msm_reduce2d_lines<1>"),
           "host2d-lines4": ({"red2d": 1, "red2d_prefold": 0, "quad": 2}, "msm_reduce2d_lines<4>")}


def _p(d):
    return {f"msm.{k}": v for k, v in d.items()}


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
    return mc.make_pool(N_POOL)


@pytest.fixture(scope="module")
def cus(gpu):
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def cached(O, pool):
    """cases by (distribution, n, seed): built once for the module"""
    memo = {}

    def get(dist, n, seed, off=0):
        key = (dist, n, seed, off)
        if key not in memo:
            memo[key] = case_with_scalars(O, pool, dist, n, seed, off)
        return memo[key]
    return get


def explicit(O, pool, values, logs=None, off=0, pad_to=None):
    """(scalars on the device, bases on the device, expected point, canonical scalars, bases on the host or None) for scalars
    given as ints over pool bases, or over bases log_i * G (log 0: the identity point); zero scalars pad up to `pad_to`"""
    import torch
    from circuits_halo2_amd.arithmetic import g1_fixed_base_mul
    values = list(values) + [0] * ((pad_to or 0) - len(values))
    n = len(values)
    canon = _ints(values)
    k_dev, k_host = _mont(canon)
    if logs is None:
        bases, s_host = pool["bases"][64 * off:64 * (off + n)], pool["s"][32 * off:32 * (off + n)]
    else:
        s_dev, s_host = _mont(_ints(list(logs) + [1] * (n - len(logs))))
        bases = g1_fixed_base_mul(s_dev)
    want = O.g1_mul(O.g1_generator(), O.fr_dot(k_host, s_host))
    torch.cuda.synchronize()
    return k_dev, bases, want, canon


def srs_over(gpu, bases_dev, k, c):
    """the resident-SRS object over arbitrary bases (both bases the same), with the window table of width c: commitments
    against it are fixed-base jobs whose answer is still <k, s> G"""
    host = bases_dev.cpu().numpy()
    assert host.size == 64 << k
    p = gpu.ParamsKZG(k, host, host)
    p.precompute(0, window_bits=c)
    return p


def timed_msm(k, bases):
    from circuits_halo2_amd.arithmetic import best_multiexp
    return best_multiexp(k, bases, timings=True)


def timed_commit(params, poly, basis=0):
    from circuits_halo2_amd import ffi
    out, tm = np.zeros(64, dtype=np.uint8), ffi.MsmTimings()
    ffi.check(ffi.lib().sg_commit_dev_timed(C.c_uint64(params.handle()), C.c_int(basis), ffi.dev_ptr(poly), C.c_size_t(poly.numel() // 32),
                                            ffi.current_stream_ptr(), ffi.ptr(out), C.byref(tm)))
    return out, tm.as_dict()


def check_report(tm, canon, n, c, fixed, params, cus):
    """the job's own report against what the case was built for: window width and count, tasks = sum ceil(cnt_b / L), the
    largest bucket, and the accumulation's grid"""
    e = expected_backend(n, 1, fixed, c, params, 1)
    cnt = mc.bucket_counts(canon, c, fixed)
    tasks, biggest = mc.tasks_and_max(cnt, e["log_seg"])
    got = {k: tm[k] for k in ("window_bits", "windows", "tasks", "max_bucket", "accumulate_threads")}
    assert got == {"window_bits": c, "windows": e["windows"], "tasks": tasks, "max_bucket": biggest,
                   "accumulate_threads": mc.accumulate_threads(n, 1, fixed, c, params, 1, cus)}, (got, params)
    return tasks, biggest


# ----------------------------------------------------------------------------- 1: accumulation
_GRID = [(at, w) for at in (64, 128, 256) for w in (1, 2, 3, 7, 8)]
# (n, distribution, msm.* parameters)
ACC = [(1 << 17, "uniform", {"acc_threads": at, "acc_waves": w}) for at, w in _GRID]
ACC += [(1 << 20, d, {"acc_threads": at, "acc_waves": w}) for d, at, w in
        (("uniform", 64, 3), ("uniform", 128, 1), ("uniform", 256, 8), ("pm_pairs", 128, 7), ("signed16", 256, 2), ("uniform", 64, 8))]
ACC += [(1 << 17, "uniform", {"log_seg": s}) for s in (1, 2, 4, 6, 8, 9, 12)]
ACC += [(1 << 20, "tiled32", {"log_seg": s, "acc_threads": at}) for s, at in ((9, 64), (12, 256))]   # buckets of 2^15: full tasks beyond TASK_BINS
ACC += [((1 << 17) + 5, "uniform", {"acc_threads": 64, "acc_waves": 2}), ((1 << 17) - 3, "uniform", {"acc_threads": 256, "acc_waves": 7}),
        (1 << 17, "signed15", {"acc_threads": 256, "acc_waves": 1}), (1 << 17, "pm_pairs", {"acc_threads": 64, "acc_waves": 7}),
        (2, "uniform", {"window_bits": 16, "acc_threads": 256, "acc_waves": 3}),                       # fewer tasks than one wave
        (1 << 15, "equal", {"log_seg": 12, "acc_waves": 1}), (1 << 15, "byte", {"log_seg": 9, "acc_threads": 256, "acc_waves": 8})]


def _acc_id(a):
    n, dist, extra = a
    return f"{n}-{dist}-" + "-".join(f"{k}{v}" for k, v in extra.items())


@pytest.mark.parametrize("n,dist,extra", ACC, ids=[_acc_id(a) for a in ACC])
def test_accumulate_generic(gpu, O, cached, cus, n, dist, extra):
    """msm_accumulate at 64 / 128 / 256 threads per workgroup, 1 .. 8 waves per SIMD and task lengths 2 .. 4096 (beyond 256 all
    task lengths share the last histogram bin), at lengths whose task count is not a multiple of a ticket and with fewer
    tasks than one wave: the exact point, and the job's own report of windows, tasks, largest bucket and grid"""
    from circuits_halo2_amd import ffi
    params = _p(extra)
    k, bases, want, canon = cached(dist, n, 2000 + n % 977, off=n % 7)
    c = mc.generic_window_bits(n, False, params)
    with ffi.params(params):
        got, tm = timed_msm(k, bases)
    tasks, _ = check_report(tm, canon, n, c, False, params, cus)
    if n == 2:
        assert tasks < 64
    assert (got == want).all()


@pytest.mark.parametrize("c", (13, 16))
@pytest.mark.parametrize("log_seg,fold,log_G,extra", POPULATIONS, ids=[f"seg{p[0]}-fold{p[1]}-G{p[2]}" for p in POPULATIONS])
def test_accumulate_prescribed_populations(gpu, O, pool, cus, c, log_seg, fold, log_G, extra):
    """buckets of exactly 1, L - 1, L, L + 1, 2L, fold L, fold L + 1 and L^2 + 1 entries in the first, chunk-boundary and last
    bucket of a window and in the top window: the report must show exactly the tasks and the largest bucket prescribed"""
    from circuits_halo2_amd import ffi
    values, want_map = mc.populations(c, log_seg, fold, log_G, extra)
    k, bases, want, canon = explicit(O, pool, mc.interleave(values, c), off=c)
    L = 1 << log_seg
    bad = []
    for at, w in ((64, 1), (128, 3), (256, 8)):
        params = _p({"window_bits": c, "log_seg": log_seg, "acc_threads": at, "acc_waves": w, "red2d_fold": fold})
        with ffi.params(params):
            got, tm = timed_msm(k, bases)
        tasks, biggest = check_report(tm, canon, len(values), c, False, params, cus)
        assert tasks == sum(-(-m // L) for m in want_map.values()) and biggest == max(want_map.values())
        if not (got == want).all():
            bad.append((at, w))
    assert not bad, bad


# ----------------------------------------------------------------------------- fixed base: commitments at k = 17
K_FIXED = 17


@pytest.fixture(scope="module")
def kzg(gpu, O):
    """ParamsKZG.setup(17, tau) and six columns of 2^17 rows: column i is coefficients (i % 3 == 0), Lagrange (1) or a
    piecewise-constant Lagrange column committed in difference form (2); `want` from a(tau) G"""
    from circuits_halo2_amd.utils import random_fr_canonical
    n = 1 << K_FIXED
    tau = O.fr_to_mont(random_fr_canonical(0x7A1, 1))
    params = gpu.ParamsKZG.setup(K_FIXED, tau)
    rng = np.random.default_rng(18)
    cols, kinds, want, canons = [], [], [], []
    for i, d in enumerate(["uniform", "byte", None, "signed16", "uniform", None]):
        if d is None:
            runs = np.sort(rng.choice(n, size=40, replace=False))
            vals = random_fr_canonical(810 + i, 41).reshape(41, 32)
            canon = vals[np.searchsorted(runs, np.arange(n), side="right")].reshape(-1)
        else:
            canon = mc.scalars(d, n, 810 + i)
        dev, host = _mont(canon)
        coeffs = host if i % 3 == 0 else O.lagrange_to_coeff(host, K_FIXED, O.ncpu())
        cols.append(dev)
        kinds.append(i % 3)
        canons.append(canon)
        want.append(O.g1_mul(O.g1_generator(), O.fr_eval_poly(coeffs, tau)))
    params.precompute()
    yield {"params": params, "cols": cols, "kinds": kinds, "want": want, "canon": canons, "tau": tau}
    params.free()


@pytest.mark.parametrize("waves", (1, 2, 3, 8))
def test_accumulate_fixed_base(gpu, kzg, cus, waves):
    """commitments of 2^17 rows over the window tables (one bucket set per polynomial: every window's entries in it) at
    msm.acc_waves_fixed 1 / 2 / 3 / 8, coefficient and Lagrange columns, uniform and byte-valued and at the signed-digit edges"""
    from circuits_halo2_amd import ffi
    p = kzg["params"]
    for i, at in ((0, 64), (1, 256), (3, 128), (4, 0)):
        params = _p({"acc_waves_fixed": waves, "acc_threads": at})
        with ffi.params(params):
            got, tm = timed_commit(p, kzg["cols"][i], kzg["kinds"][i])
        check_report(tm, kzg["canon"][i], 1 << K_FIXED, 16, True, params, cus)
        assert (got == kzg["want"][i]).all(), (i, at)


@pytest.mark.parametrize("path", ["default"] + list(SCAN_PATHS) + list(DEVICE_2D))
def test_commitment_batch_mixing_plain_and_difference_form(gpu, kzg, path):
    """one fused fixed-base job of six columns, two of them in difference form (diff_mask), on every reduction path a job of
    six bucket sets can take"""
    from circuits_halo2_amd import ffi
    params = _p(({**SCAN_PATHS, **DEVICE_2D}[path][0]) if path != "default" else {})
    e = expected_backend(1 << K_FIXED, 6, True, 16, params, 1)
    assert path == "default" and e["red2d"] == 1 or {**SCAN_PATHS, **DEVICE_2D}[path][1] in e["kernels"]
    with ffi.params(params):
        got = kzg["params"].commit_batch_mixed(kzg["cols"], kzg["kinds"])
    assert [i for i in range(6) if not (got[i] == kzg["want"][i]).all()] == []


# ----------------------------------------------------------------------------- 2: merge rounds
def _heavy(O, pool, c, sizes, off):
    """buckets of exactly `sizes` entries (the largest first, in the last bucket of window 0) beside single entries"""
    spots = mc.population_spots(c, 2)
    order = [3, 0, 8, 1, 5, 10]
    values = []
    for i, m in enumerate(sizes):
        values += [mc.place(c, *spots[order[i]])[0]] * m
    values += [mc.place(c, *s)[0] for i, s in enumerate(spots) if i not in order[:len(sizes)]]
    return explicit(O, pool, mc.interleave(values, sum(sizes)), off=off)


# (log_seg, bucket sizes, merge rounds with fold = 1)
MERGE = [(4, (200, 17, 16), 1), (4, (257, 256, 31), 2), (2, (700, 5, 64), 4), (2, (16, 4, 3), 1), (2, (17, 16), 2)]


@pytest.mark.parametrize("quad,mqt", [(0, 0), (0, MQT_DEFAULT), (2, 0), (2, MQT_DEFAULT)])
@pytest.mark.parametrize("log_seg,sizes,rounds", MERGE, ids=[f"seg{m[0]}-{m[1][0]}" for m in MERGE])
def test_merge_rounds(gpu, O, pool, cus, quad, mqt, log_seg, sizes, rounds):
    """one, two and four merge rounds through msm_merge<1> (quad 0, or quad 2 with merge_quad_tasks 0: the fallback) and
    msm_merge<4>, behind each scan reduction"""
    from circuits_halo2_amd import ffi
    c = 13
    k, bases, want, canon = _heavy(O, pool, c, sizes, off=3)
    n = canon.size // 32
    bad = []
    for name, (force, _) in SCAN_PATHS.items():
        if force["quad"] != quad:
            continue
        params = _p({**force, "window_bits": c, "log_seg": log_seg, "merge_quad_tasks": mqt})
        e = expected_backend(n, 1, False, c, params, 1, max_bucket=max(sizes))
        assert e["merge_rounds"] == rounds
        assert e["kernels"][1:1 + rounds] == ["msm_merge<4>" if quad == 2 and mqt else "msm_merge<1>"] * rounds
        with ffi.params(params):
            got, tm = timed_msm(k, bases)
        assert tm["max_bucket"] == max(sizes)
        if not (got == want).all():
            bad.append(name)
    assert not bad, bad


@pytest.mark.parametrize("fold", (1, 8, 256))
@pytest.mark.parametrize("over", (0, 1))
def test_merge_loop_stops_at_fold(gpu, O, pool, fold, over):
    """the 2-D line sums add up to red2d_fold partial sums per bucket themselves: a largest bucket of exactly fold * L entries
    needs no merge round, one entry more needs one; 700 entries in tasks of 4 stop after three rounds at fold 8"""
    from circuits_halo2_amd import ffi
    c, log_seg = 13, 2
    for sizes in ((fold * 4 + over, 3, 2), (700, 33)) if fold == 8 and over else ((fold * 4 + over, 3, 2),):
        k, bases, want, canon = _heavy(O, pool, c, sizes, off=9)
        for name, (force, kernel) in DEVICE_2D.items():
            params = _p({**force, "window_bits": c, "log_seg": log_seg, "red2d_fold": fold})
            e = expected_backend(canon.size // 32, 1, False, c, params, 1, max_bucket=max(sizes))
            assert e["merge_rounds"] == (3 if sizes[0] == 700 else over) and kernel in e["kernels"] and e["fold"] == fold
            with ffi.params(params):
                got, tm = timed_msm(k, bases)
            assert tm["max_bucket"] == max(sizes)
            assert (got == want).all(), (name, sizes)


# ----------------------------------------------------------------------------- 3: the scan reduction
@pytest.mark.parametrize("c", (4, 5, 8, 13, 16))
@pytest.mark.parametrize("path", list(SCAN_PATHS))
def test_scan_reduction_matrix(gpu, O, cached, path, c):
    """msm_reduce_buckets<4> / <1> / _lean<1> at 64, 128 and 256 logical threads and 2^0 .. 2^8 buckets per thread, at window
    widths 4 .. 16: uniform scalars and the signed-digit edges of the width in use"""
    from circuits_halo2_amd import ffi
    from circuits_halo2_amd.arithmetic import best_multiexp
    n = 4096
    k, bases, want, _ = cached(f"signed{c}", n, 3000 + c, off=c)
    force, kernel = SCAN_PATHS[path]
    bad, shapes = [], set()
    for rt, chunk in itertools.product((64, 128, 256), (0, 1, 2, 4, 8)):
        params = _p({**force, "window_bits": c, "red_threads": rt, "log_red_chunk": chunk})
        e = expected_backend(n, 1, False, c, params, 1)
        assert e["kernels"][1] == kernel and e["red2d"] == 0
        shapes.add((e["blocks"] == 1, e["T1"]))
        with ffi.params(params):
            if not (best_multiexp(k, bases) == want).all():
                bad.append((rt, chunk, e["log_G"], e["blocks"]))
    assert not bad, bad
    if c == 16:
        assert any(t1 and t1 <= 64 for _, t1 in shapes) and (path == "scan4" or any(one for one, _ in shapes))
        assert (path == "scan4") != any(t1 == 256 for _, t1 in shapes)


# (name, n, window width, msm.* parameters, what expected_backend must say)
SCAN_NAMED = [
    ("one-block", 4096, 13, {"quad": 0, "red_threads": 256, "log_red_chunk": 4}, {"blocks": 1, "T1": None}),
    ("items4-T1-64", 4096, 16, {"quad": 0, "red_threads": 128, "log_red_chunk": 2}, {"blocks": 64, "T1": 64, "level1": "msm_reduce_items<4>"}),
    ("items1-T1-128", 4096, 16, {"quad": 0, "red_threads": 64, "log_red_chunk": 2}, {"blocks": 128, "T1": 128, "level1": "msm_reduce_items<1>"}),
    ("items1-256-blocks", 4096, 16, {"quad": 0, "red_threads": 64, "log_red_chunk": 1}, {"blocks": 256, "T1": 256, "level1": "msm_reduce_items<1>"}),
    ("items1-256-blocks-lean", 4096, 16, {"quad": 0, "red_lean": 2, "red_threads": 64, "log_red_chunk": 1}, {"blocks": 256, "T1": 256, "level1": "msm_reduce_items<1>"}),
    ("items1-full-size", 1 << 20, 16, {"quad": 0, "red_threads": 64, "log_red_chunk": 1}, {"blocks": 256, "T1": 256, "level1": "msm_reduce_items<1>"}),
    ("chunk-clamped", 4096, 5, {"quad": 0, "log_red_chunk": 8}, {"log_G": 4, "blocks": 1}),
    ("log_G-raised", 4096, 16, {"quad": 2, "log_red_chunk": 1}, {"log_G": 3, "blocks": 64, "level1": "msm_reduce_items<4>"}),
    ("scan1-full-size", 1 << 20, 16, {"quad": 0, "red_lean": 0}, {"blocks": 16, "level0": "msm_reduce_buckets<1>"}),
    ("scan4-full-size", 1 << 20, 16, {"quad": 2}, {"blocks": 64, "level0": "msm_reduce_buckets<4>"}),
    ("lean-full-size", 1 << 20, 16, {"quad": 0, "red_lean": 2}, {"blocks": 16, "level0": "msm_reduce_buckets_lean<1>"}),
]


@pytest.mark.parametrize("name,n,c,extra,expect", SCAN_NAMED, ids=[s[0] for s in SCAN_NAMED])
def test_scan_reduction_named_shapes(gpu, O, cached, name, n, c, extra, expect):
    """the corners of the scan reduction's shape: one workgroup per window (no level 1, no T term), level 1 in quads, the
    only road to msm_reduce_items<1> (256 level-0 workgroups), a chunk clamped to c - 1, a chunk the loop has to raise"""
    from circuits_halo2_amd import ffi
    from circuits_halo2_amd.arithmetic import best_multiexp
    params = _p({"red2d": 0, "window_bits": c, **extra})
    e = expected_backend(n, 1, False, c, params, 1)
    level1 = [x for x in e["kernels"] if x.startswith("msm_reduce_items")]
    got = {"log_G": e["log_G"], "blocks": e["blocks"], "T1": e["T1"], "level0": e["kernels"][1], "level1": level1[0] if level1 else None}
    assert {key: got[key] for key in expect} == expect
    for dist in ("uniform", f"signed{c}"):
        k, bases, want, _ = cached(dist, n, 3100 + c, off=1)
        with ffi.params(params):
            assert (best_multiexp(k, bases) == want).all(), dist


# ----------------------------------------------------------------------------- 4: the 2-D reduction, host weights
K_SMALL = 12


@pytest.fixture(scope="module")
def columns(O, pool):
    """seven columns of 2^12 scalars over the pool's first 2^12 bases: (device tensors, expected points) per window width"""
    n = 1 << K_SMALL
    memo = {}

    def get(c):
        if c not in memo:
            dists = [f"signed{c}", "uniform", "byte", "uniform", "sparse", "equal", "uniform"]
            made = [explicit_canon(O, pool, mc.scalars(d, n, 4000 + 10 * c + i)) for i, d in enumerate(dists)]
            memo[c] = ([m[0] for m in made], [m[1] for m in made])
        return memo[c]
    return get


def explicit_canon(O, pool, canon):
    k_dev, k_host = _mont(canon)
    n = canon.size // 32
    return k_dev, O.g1_mul(O.g1_generator(), O.fr_dot(k_host, pool["s"][:32 * n]))


@pytest.mark.parametrize("c", (4, 5, 6, 15, 16))
def test_reduce2d_host_weights_matrix(gpu, O, pool, columns, c):
    """fixed-base jobs of 1, 5, 6 and 7 polynomials on both sides of red2d_max_sets = 4, 6, 8, with the fold pass on and off, in
    quads and in lanes, at c - 1 = 4, 5, 14 and 15 bits; at width 4 the rule keeps the scan reduction even when asked"""
    from circuits_halo2_amd import ffi
    n = 1 << K_SMALL
    srs = srs_over(gpu, pool["bases"][:64 * n], K_SMALL, c)
    cols, want = columns(c)
    bad = []
    try:
        for M, max_sets, prefold, quad, pqb in itertools.product((1, 5, 6, 7), (4, 6, 8), (0, 1), (0, 2), (0, 1 << 15)):
            params = _p({"red2d": 1, "red2d_max_sets": max_sets, "red2d_prefold": prefold, "quad": quad, "prefold_quad_buckets": pqb})
            e = expected_backend(n, M, True, c, params, 1)
            assert e["red2d"] == (1 if c >= 5 and M <= max_sets else 0) and e["per_win"] == (c if e["red2d"] else 3)
            if e["red2d"]:
                q = "<4>" if quad else "<1>"
                lines = "msm_reduce2d_lines_folded" + q if prefold else "msm_reduce2d_lines" + q
                assert lines in e["kernels"] and any(x.startswith("msm_fold_buckets") for x in e["kernels"]) == bool(prefold)
            with ffi.params(params):
                got = srs.commit_batch(cols[:M])
            bad += [(M, max_sets, prefold, quad, pqb, i) for i in range(M) if not (got[i] == want[i]).all()]
    finally:
        srs.free()
    assert not bad, bad[:8]


# ----------------------------------------------------------------------------- 5: the 2-D reduction, device weights
@pytest.mark.parametrize("path", list(DEVICE_2D))
def test_reduce2d_device_weights(gpu, O, pool, cached, columns, path):
    """msm_reduce2d_combine and the one-term-per-window host tail: a generic MSM of 2^20 (16 bucket sets) and of 2^15 (20), a
    generic batch through sg_msm_g1_batch_dev, and a fixed-base job of nine polynomials (past red2d_max_sets)"""
    from circuits_halo2_amd import ffi
    from circuits_halo2_amd.arithmetic import best_multiexp, best_multiexp_batch
    force, kernel = DEVICE_2D[path]
    params = _p(force)
    for n, dist in ((1 << 20, "uniform"), (1 << 15, "uniform"), (1 << 15, "signed13")):
        c = mc.generic_window_bits(n, False)
        e = expected_backend(n, 1, False, c, params, 1)
        assert e["red2d"] == 2 and e["per_win"] == 1 and kernel in e["kernels"] and "msm_reduce2d_combine" in e["kernels"]
        k, bases, want, _ = cached(dist, n, 5000, off=2)
        with ffi.params(params):
            assert (best_multiexp(k, bases) == want).all(), (n, dist)
    batch = [cached(d, 1 << 15, 5100 + i, off=i) for i, d in enumerate(("uniform", "byte", "signed11", "uniform"))]
    assert expected_backend(1 << 15, 4, False, 11, params, 1)["red2d"] == 2
    with ffi.params(params):
        got = best_multiexp_batch([(b[0], b[1]) for b in batch])
    assert all((g == b[2]).all() for g, b in zip(got, batch))
    n = 1 << K_SMALL
    cols, want = columns(12)
    nine = (cols + cols[:2], want + want[:2])
    assert expected_backend(n, 9, True, 12, params, 1)["red2d"] == 2
    srs = srs_over(gpu, pool["bases"][:64 * n], K_SMALL, 12)
    try:
        with ffi.params(params):
            got = srs.commit_batch(nine[0])
    finally:
        srs.free()
    assert all((got[i] == nine[1][i]).all() for i in range(9))


# ----------------------------------------------------------------------------- 6: fused jobs on every reduction path
@pytest.mark.parametrize("path", list(SCAN_PATHS) + list(DEVICE_2D))
def test_fused_jobs(gpu, O, pool, cached, path):
    """a generic batch of 2 and of 4 MSMs of 2^15 (one fused job each) and a fixed-base batch of 64 polynomials of 2^10 rows
    (MAX_FUSED), per reduction path"""
    from circuits_halo2_amd import ffi
    from circuits_halo2_amd.arithmetic import best_multiexp_batch
    force, kernel = {**SCAN_PATHS, **DEVICE_2D}[path]
    params = _p(force)
    batch = [cached(d, 1 << 15, 5100 + i, off=i) for i, d in enumerate(("uniform", "byte", "signed11", "uniform"))]
    for M in (2, 4):
        assert kernel in expected_backend(1 << 15, M, False, 11, params, 1)["kernels"]
        with ffi.params({**params, "msm.acc_log": 1}):
            got = best_multiexp_batch([(b[0], b[1]) for b in batch[:M]])
            log = ffi.msm_launch_log()
        assert [(r["n"], r["M"]) for r in log] == [(1 << 15, M)]
        assert all((g == b[2]).all() for g, b in zip(got, batch))
    n, M = 1 << 10, 64
    assert kernel in expected_backend(n, M, True, 10, params, 1)["kernels"]
    polys = [explicit_canon(O, pool, mc.scalars(("uniform", "byte", "signed10", "sparse")[i % 4], n, 6000 + i)) for i in range(M)]
    srs = srs_over(gpu, pool["bases"][:64 * n], 10, 10)
    try:
        with ffi.params({**params, "msm.acc_log": 1}):
            got = srs.commit_batch([p[0] for p in polys])
            log = ffi.msm_launch_log()
    finally:
        srs.free()
    assert [(r["n"], r["M"], r["fixed"]) for r in log] == [(n, M, 1)]
    assert [i for i in range(M) if not (got[i] == polys[i][1]).all()] == []


# ----------------------------------------------------------------------------- 7: group-law edges on every reduction path
@pytest.mark.parametrize("c", EDGE_WIDTHS)
@pytest.mark.parametrize("path", list(SCAN_PATHS) + ["host2d-fold4", "host2d-fold1", "host2d-lines4", "host2d-lines1"] + list(DEVICE_2D))
def test_group_law_edges(gpu, O, pool, path, c):
    """equal, opposite and identity values inside the reductions: every bucket of a window the same point, P and -P in
    neighbouring buckets, only the first / only the last bucket, one window alone, a window that cancels beside one that does
    not, identity points among the bases of deep buckets -- at tasks of 4, so that the deep buckets own several partial sums"""
    from circuits_halo2_amd import ffi
    from circuits_halo2_amd.arithmetic import best_multiexp
    fixed = path in HOST_2D
    force, kernel = {**SCAN_PATHS, **HOST_2D, **DEVICE_2D}[path]
    params = _p({**force, "window_bits": c, "log_seg": 2})
    k_srs = c - 1 if c > 10 else 8
    bad = []
    for name, values, logs in edge_cases(c):
        n = 1 << k_srs if fixed else len(values)
        k, bases, want, _ = explicit(O, pool, values, logs, pad_to=n)
        assert want.any()
        assert kernel in expected_backend(n, 1, fixed, c, params, 1)["kernels"]
        if fixed:
            srs = srs_over(gpu, bases, k_srs, c)
            try:
                with ffi.params(params):
                    got = srs.commit(k)
            finally:
                srs.free()
        else:
            with ffi.params(params):
                got = best_multiexp(k, bases)
        if not (got == want).all():
            bad.append(name)
    assert not bad, bad


# ----------------------------------------------------------------------------- 8: other jobs in flight
def test_three_threads_in_flight_on_the_lean_path(gpu, O, cached, cus):
    """three host threads with blocking MSMs of 2^20, rounds started together, scan reduction in lanes: with another job in
    flight a job takes two waves per SIMD, 16 buckets per thread and the lean level 0 (red_lean = 1) -- branches that exist
    only then; every result against its exact answer"""
    import torch
    from circuits_halo2_amd import arithmetic as A, ffi
    n, rounds = 1 << 20, 3
    cases = [cached(d, n, 7000 + i, off=i) for i, d in enumerate(("uniform", "signed16", "sparse"))]
    e = expected_backend(n, 1, False, 16, _p({"red2d": 0, "quad": 0}), 2)
    assert e["kernels"][1] == "msm_reduce_buckets_lean<1>" and e["log_G"] == 4
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
        except BaseException as exc:   # (reported below)
            errors.append(exc)
            barrier.abort()

    with ffi.params(_p({"red2d": 0, "quad": 0, "acc_log": 1})):
        threads = [threading.Thread(target=run, args=(i,), daemon=True) for i in range(len(cases))]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=300)
        log = ffi.msm_launch_log()
    assert not any(t.is_alive() for t in threads) and not errors, errors
    for i, c_ in enumerate(cases):
        assert len(got[i]) == rounds and all((p == c_[2]).all() for p in got[i]), i
    assert any(r["jobs_in_flight"] >= 2 for r in log), "the three threads never had two jobs in flight"
    two_waves = mc.accumulate_threads(n, 1, False, 16, {}, 2, cus)
    assert {r["threads"] for r in log} <= {two_waves, mc.accumulate_threads(n, 1, False, 16, {}, 1, cus)}
    assert any(r["threads"] == two_waves for r in log), "no accumulation took the two-wave grid"


# ----------------------------------------------------------------------------- 9: nothing left behind
def test_defaults_after_the_module(gpu, O):
    """(last in the file) every parameter reads back its documented default (include/summa_gpu.h), and a fresh MSM of 2^16
    still matches the oracle"""
    from param_doc import documented_defaults
    from circuits_halo2_amd import ffi
    from circuits_halo2_amd.arithmetic import best_multiexp
    defaults = documented_defaults()
    assert len(defaults) >= 40 and {f"msm.{k}" for k in mc.BACKEND_DEFAULTS} <= set(defaults)
    assert {name: ffi.get_param(name) for name in defaults} == defaults
    n = 1 << 16
    sc = O.random_fr(0x17, n)
    bases = O.fixed_base_mul(O.random_fr(0x71, n), O.ncpu())
    assert (best_multiexp(_dev(sc), _dev(bases)) == O.best_multiexp(sc, bases, O.ncpu())).all()
