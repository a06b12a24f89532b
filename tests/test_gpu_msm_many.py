"""sg_msm_g1_many_* (csrc/msm_many.hip: many small MSMs in one launch, kept on the device; sums over ranges of them) bit-exact
against the oracle's MSM of each job and the oracle's point additions: job counts at the sum kernel's stride edges, every job size
class mixed inside one call, scalars at the window boundaries, the group law's special cases inside a job and across jobs, every
kind of range, every rejected argument, and the memory accounting of begin / end."""
import ctypes as C

import numpy as np
import pytest

import msm_cases as MC

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 8, 9, 37, 63, 64)          # points per job, mixed inside one call
JOB_COUNTS = (1, 2, 255, 256, 257, 513)   # around the 256 jobs one pass of the sum kernel takes
R = MC.R


def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from circuits_halo2_amd import ffi
    ffi.check(ffi.lib().sg_init(0))


def _fold(O, points):
    acc = np.zeros(64, dtype=np.uint8)
    for p in points:
        acc = O.g1_add(acc, p)
    return acc


@pytest.fixture(scope="module")
def pool():
    """513 jobs of SIZES[(i + 1) % 7] points (job 0: one point, job 1: eight) over 64 random bases, uniform scalars with 0, 1, r - 1
    and window-boundary scalars sprinkled in, and the oracle's MSM of every job -- computed once, read by every test below"""
    _gpu()
    from conftest import fr_np
    from oracle import oracle as O
    bases = O.fixed_base_mul(O.random_fr(4100, 64), 4).reshape(64, 64)
    special = fr_np([0, 1, R - 1] + MC.signed_digit_specials(4)).reshape(-1, 32)
    rng = np.random.default_rng(41)
    jobs, want = [], []
    for i in range(max(JOB_COUNTS)):
        n = SIZES[(i + 1) % len(SIZES)]
        sc = O.random_fr(4200 + i, max(n, 1)).reshape(-1, 32)[:n].copy()
        for j in range(0, n, 5):
            sc[j] = special[(i + j) % special.shape[0]]
        bs = bases[rng.permutation(64)[:n]].copy()
        jobs.append((sc.reshape(-1), bs.reshape(-1)))
        want.append(O.best_multiexp(sc.reshape(-1), bs.reshape(-1), 1) if n else np.zeros(64, dtype=np.uint8))
    assert {s.size // 32 for s, _ in jobs[:7]} == set(SIZES)
    return {"jobs": jobs, "want": want}


@pytest.mark.parametrize("count", JOB_COUNTS)
def test_every_job_and_every_kind_of_range(pool, count):
    """one begin over the first `count` jobs; then the whole range, single jobs, empty ranges, eight ranges in one call, and ranges
    that start and end off the 256 stride, each against the oracle's sum of the jobs' MSMs"""
    from circuits_halo2_amd.arithmetic import MultiexpMany
    from oracle import oracle as O
    want = pool["want"][:count]
    expect = lambda a, b: _fold(O, want[a:b])
    with MultiexpMany(pool["jobs"][:count]) as many:
        assert many.jobs == count
        singles = sorted({0, count - 1, count // 2, min(count - 1, 255), min(count - 1, 256), min(count - 1, 6), min(count - 1, 7)})
        for i in range(0, len(singles), 8):
            got = many.sums([(j, j + 1) for j in singles[i:i + 8]])
            for j, g in zip(singles[i:i + 8], got):
                assert (g == want[j]).all(), (count, j)
        ranges = [(0, count), (0, 0), (count, count), (count // 2, count // 2), (0, count // 2), (count // 2, count), (0, min(count, 256)),
                  (min(count, 1), count)]
        assert len(ranges) == 8                                            # the most one call takes
        for (a, b), g in zip(ranges, many.sums(ranges)):
            assert (g == expect(a, b)).all(), (count, a, b)
        assert not many.sums([(0, 0)])[0].any() and many.sums([]) == []
        if count > 256:                                                    # thread t's second job; a range that straddles the stride
            ranges = [(3, min(259, count)), (3, min(260, count)), (255, 257), (256, count), (1, 256), (250, count - 1), (min(257, count - 1), min(258, count))]
            for (a, b), g in zip(ranges, many.sums(ranges)):
                assert (g == expect(a, b)).all(), (count, a, b)
        assert (many.sums([(0, count)])[0] == expect(0, count)).all()      # again: nothing was consumed


def test_scalars_at_the_window_boundaries_and_the_group_law(pool):
    """inside a job: 0, 1, r - 1 and the signed-digit edges of c = 4 (one job holding them all, and one job each); the same point
    twice with equal scalars (P + P in a bucket); P and -P with equal scalars (a bucket returns to the identity); the identity among
    the bases; one point 64 times (equal partial sums in the suffix scan).  Across jobs: two jobs with equal results in one range (a
    doubling in the sum kernel), two with opposite results (64 zero bytes), identities beside them."""
    from conftest import fr_np, point_np
    from circuits_halo2_amd.arithmetic import MultiexpMany
    from oracle import oracle as O, pyref as P
    bases = O.fixed_base_mul(O.random_fr(4300, 64), 4).reshape(64, 64)
    g = bases[0]
    neg = point_np(P.g1_neg(P.g1_from_bytes(g.tobytes())))
    ident = np.zeros(64, dtype=np.uint8)
    vals = [0, 1, R - 1] + MC.signed_digit_specials(4)
    k = O.random_fr(4301, 4).reshape(4, 32)
    jobs = [(fr_np(vals), bases[:len(vals)].reshape(-1))]
    jobs += [(fr_np([v]), bases[i + 1]) for i, v in enumerate(vals)]
    first_law = len(jobs)
    jobs += [
        (np.concatenate([k[0], k[0]]), np.concatenate([g, g])),                              # P twice, equal scalars
        (np.concatenate([k[1], k[1], k[2]]), np.concatenate([g, neg, bases[5]])),            # P and -P cancel, one point stays
        (np.concatenate([k[1], k[1]]), np.concatenate([g, neg])),                            # ... nothing stays
        (np.concatenate([k[0], k[1], k[2]]), np.concatenate([ident, bases[6], ident])),      # identity bases
        (np.tile(k[3], 64), np.tile(g, 64)),                                                 # one point, one scalar, 64 times
        (fr_np([3, 3, 3, 3, 5, 5, 5]), np.tile(g, 7)),                                       # deep equal buckets
        (k[2].copy(), bases[7].copy()), (k[2].copy(), bases[7].copy()),                      # two jobs with equal results
        (k[3].copy(), bases[8].copy()), (k[3].copy(), point_np(P.g1_neg(P.g1_from_bytes(bases[8].tobytes())))),   # opposite results
        (fr_np([0, 0]), bases[:2].reshape(-1)), (np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint8)),       # identities
    ]
    want = [O.best_multiexp(np.ascontiguousarray(s), np.ascontiguousarray(b), 1) if s.size else ident for s, b in jobs]
    assert not want[first_law + 2].any() and not want[-1].any() and not want[-2].any() and want[first_law + 1].any()
    n = len(jobs)
    eq, op = first_law + 6, first_law + 8
    with MultiexpMany(jobs) as many:
        for i in range(0, n, 8):
            got = many.sums([(j, j + 1) for j in range(i, min(n, i + 8))])
            for j, gj in zip(range(i, n), got):
                assert (gj == want[j]).all(), j
        got = many.sums([(eq, eq + 2), (op, op + 2), (op, n), (eq, op + 1), (0, n), (first_law + 2, first_law + 3), (eq + 1, op + 2)])
        assert (got[0] == O.g1_add(want[eq], want[eq])).all() and got[0].any()
        assert not got[1].any() and not got[2].any() and not got[5].any()
        assert (got[3] == _fold(O, want[eq:op + 1])).all()
        assert (got[4] == _fold(O, want)).all()
        assert (got[6] == want[eq]).all()


def test_rejected_arguments():
    """`first` that decreases, a job above 64 points, more than 2^14 jobs, null pointers; ranges that end before they start or
    beyond the last job, more than eight of them; an unknown handle, for sums and for end -- SG_ERR_INVALID each, and the handle
    keeps working afterwards"""
    _gpu()
    from circuits_halo2_amd import ffi
    from oracle import oracle as O
    L = ffi.lib()
    u32 = lambda v: np.array(v, dtype=np.uint32)
    sc = O.random_fr(4400, 130)
    bs = O.fixed_base_mul(O.random_fr(4401, 130), 4)
    h = C.c_uint64(0)
    begin = lambda first, jobs: L.sg_msm_g1_many_begin(ffi.ptr(sc), ffi.ptr(bs), ffi.ptr(u32(first)), C.c_uint32(jobs), C.byref(h))
    assert begin([0, 5, 4], 2) == -1 and begin([0, 65], 1) == -1 and begin([0, 64, 129], 2) == -1
    assert begin([0] * ((1 << 14) + 2), (1 << 14) + 1) == -1
    assert L.sg_msm_g1_many_begin(None, ffi.ptr(bs), ffi.ptr(u32([0, 1])), C.c_uint32(1), C.byref(h)) == -1
    assert L.sg_msm_g1_many_begin(ffi.ptr(sc), ffi.ptr(bs), None, C.c_uint32(1), C.byref(h)) == -1
    assert L.sg_msm_g1_many_begin(ffi.ptr(sc), ffi.ptr(bs), ffi.ptr(u32([0, 1])), C.c_uint32(1), None) == -1
    ffi.check(begin([0, 64, 128, 130], 3))                                  # jobs of 64, 64 and 2 points: the limit itself
    handle = C.c_uint64(h.value)
    out = np.zeros(64 * 9, dtype=np.uint8)
    sums = lambda hd, ranges, count: L.sg_msm_g1_many_sums(hd, ffi.ptr(u32(ranges)), C.c_uint32(count), ffi.ptr(out))
    try:
        assert sums(handle, [2, 1], 1) == -1 and sums(handle, [0, 4], 1) == -1 and sums(handle, [4, 4], 1) == -1
        assert sums(handle, [0, 3, 0, 4], 2) == -1
        assert sums(handle, [0, 1] * 9, 9) == -1
        assert sums(C.c_uint64(h.value + 1000), [0, 1], 1) == -1 and b"unknown handle" in L.sg_last_error()
        assert L.sg_msm_g1_many_sums(handle, None, C.c_uint32(1), ffi.ptr(out)) == -1
        assert L.sg_msm_g1_many_sums(handle, ffi.ptr(u32([0, 1])), C.c_uint32(1), None) == -1
        assert L.sg_msm_g1_many_end(C.c_uint64(h.value + 1000)) == -1
        ffi.check(sums(handle, [0, 3, 3, 3, 2, 3], 3))
        assert (out[:64] == O.best_multiexp(sc, bs, 1)).all() and not out[64:128].any()
        assert (out[128:192] == O.best_multiexp(sc[32 * 128:], bs[64 * 128:], 1)).all()
    finally:
        ffi.check(L.sg_msm_g1_many_end(handle))
    assert L.sg_msm_g1_many_end(handle) == -1 and sums(handle, [0, 1], 1) == -1   # ended: unknown from now on


def test_begin_and_end_leave_the_device_memory_where_it_was(pool):
    """begin / end twice over with 4096 jobs (32 MiB of window sums each): after sg_collect_retired the device has the memory it
    had after a first, warming round (within 16 MiB: a leaked S would be 64)"""
    import torch
    from circuits_halo2_amd import ffi
    from circuits_halo2_amd.arithmetic import MultiexpMany
    jobs = [pool["jobs"][i % 7] for i in range(4096)]
    whole = None

    def one_round():
        nonlocal whole
        with MultiexpMany(jobs) as many:
            got = many.sums([(0, len(jobs))])[0]
        assert whole is None or (got == whole).all()
        whole = got
        ffi.check(ffi.lib().sg_collect_retired())
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        return torch.cuda.mem_get_info()[0] / 2 ** 20

    base = one_round()
    one_round()
    after = one_round()
    assert abs(after - base) <= 16, (base, after)
    assert whole.any()
