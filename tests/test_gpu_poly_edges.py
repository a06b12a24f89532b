"""The polynomial helpers of csrc/poly.hip and csrc/poly_scan.cuh (evaluation, batch inversion, prefix product, Kate division,
grand products, linear combinations, element-wise product) at the sizes where their launch geometry changes and on the inputs uniform sampling never
gives, against the oracle.

tests/poly_cases.py restates the geometry and lists the cases; tests/test_poly_cases_cpu.py asserts, without a GPU, that they
reach every class of launch (each width of the Kate scan exactly full and just entered, out[n] alone in an extra block of the
prefix product, 1024 blocks and the first refused size, both instantiations of the batched evaluation, the mid-sum reduction of
a linear combination, every zero pattern of a batch-inversion chunk).

Every expected word comes from the CPU oracle or from a closed form in Python integers (a single coefficient c at degree n - 1
evaluates to c x^(n-1) and divides to q_i = c b^(n-2-i); a tiled polynomial is a geometric sum); nothing compares one library
path with another, and every comparison is bit for bit on canonical words."""
import ctypes as C

import numpy as np
import pytest

import poly_cases as pc

pytestmark = pytest.mark.gpu

R = pc.R
_REF = {}


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    import circuits_halo2_amd as sg
    from circuits_halo2_amd import ffi
    ffi.check(sg.lib().sg_init(0))
    yield sg
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()      # (a copy: the shared inputs are read only)


def _host(t):
    return t.cpu().numpy()


def _same(got, want, what):
    """bit for bit; on a mismatch say how many rows differ and where the first one is"""
    g = _host(got) if hasattr(got, "cpu") else np.asarray(got).reshape(-1)
    assert g.size == want.size, f"{what}: {g.size} bytes, {want.size} expected"
    if g.size % 32 or (g != want).any():
        bad = (g.reshape(-1, 32) != want.reshape(-1, 32)).any(axis=1)
        assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} rows differ, first at row {int(np.argmax(bad))}"


def _vec(O, name, n, seed):
    """one input vector (shared, read only)"""
    key = ("vec", name, n, seed)
    if key not in _REF:
        for old in [k for k in _REF if k[0] == "vec" and k[2] > 1 << 18 and k[2] != n]:
            del _REF[old]                                # the long vectors of one size at a time
        v = pc.vector(O, name, n, seed)
        v.setflags(write=False)
        _REF[key] = v
    return _REF[key]


def _row(v, i):
    return np.array(v[32 * i:32 * i + 32])


def _garbage(n_bytes):
    import torch
    return torch.full((n_bytes,), 0x5A, dtype=torch.uint8, device="cuda")


def _L():
    from circuits_halo2_amd import ffi
    return ffi, ffi.lib()


# ============================================================================= prefix product
@pytest.mark.parametrize("n", pc.PREFIX_SIZES)
def test_prefix_product(gpu, O, n):
    """sg_fr_prefix_product_dev, n + 1 outputs: at the 2048 j boundaries out[n] falls alone into an extra block; 2^21 - 1 elements
    fill the 1024-thread scan.  `first` (one element, then zeros): out = 1, c, 0, 0, ...; the same element followed by ones:
    out = 1, c, c, ..., the one element carried across every block"""
    from circuits_halo2_amd.arithmetic import prefix_product
    c = pc.mont([pc.single_value(11)])
    for name in (pc.PREFIX_CLASSES if n <= 4096 else pc.LARGE_CLASSES):
        a = _vec(O, name, n, 11)
        want = O.fr_prefix_product(a)
        if name == "first" and n:
            assert (want == np.concatenate([pc.mont([1]), c, np.zeros(32 * (n - 1), dtype=np.uint8)])).all()
        got = prefix_product(_dev(a))
        _same(got, want, f"prefix product n={n} {name}")
    if n:
        a = np.concatenate([c, _vec(O, "one", n - 1, 11)])
        want = np.concatenate([pc.mont([1]), np.tile(c, n)])
        assert n > 4096 or (want == O.fr_prefix_product(a)).all()
        _same(prefix_product(_dev(a)), want, f"prefix product n={n}, one element then ones")


def test_prefix_product_refuses_2_21(gpu, O):
    import torch
    from circuits_halo2_amd.arithmetic import prefix_product
    assert pc.prefix_blocks(pc.PREFIX_REFUSED, pc.PREFIX_REFUSED + 1) is None
    with pytest.raises(gpu.SummaGpuError):
        prefix_product(torch.zeros(32 * pc.PREFIX_REFUSED, dtype=torch.uint8, device="cuda"))
    a = _vec(O, "random", 1000, 12)
    _same(prefix_product(_dev(a)), O.fr_prefix_product(a), "prefix product after a refused call")


# ============================================================================= batch inversion
@pytest.mark.parametrize("n", pc.INVERT_SIZES)
def test_batch_invert(gpu, O, n):
    """sg_fr_batch_invert_dev under every zero pattern of a chunk of eight (zeros stay zero, their neighbours are inverted as if
    the zero were not there), on random words, ones and the word r - 1; the row behind the vector is not touched"""
    import torch
    from circuits_halo2_amd.arithmetic import batch_invert
    guard = np.full(32, 0xA5, dtype=np.uint8)
    for name in pc.INVERT_VALUES:
        for pat in pc.ZERO_PATTERNS:
            a = np.array(_vec(O, name, n, 21)).reshape(n, 32)
            a[pc.zero_rows(pat, n)] = 0
            a = a.reshape(-1)
            buf = _dev(np.concatenate([a, guard]))
            batch_invert(buf[:32 * n])
            torch.cuda.synchronize()
            got = _host(buf)
            _same(got[:32 * n], O.fr_batch_invert(a), f"batch inversion n={n} {name}, zeros: {pat}")
            assert (got[32 * n:] == guard).all(), f"batch inversion n={n} {name}, zeros: {pat}: the row behind the vector changed"


# ============================================================================= Kate division
def _kate_want(O, name, n, b, seed):
    """-> n quotient slots (the last one zero) and the remainder; for `last` the closed form is checked at every block edge"""
    a = _vec(O, name, n, seed)
    q, rem = O.fr_kate_division(a, b)
    if name == "last":
        c, bv = pc.single_value(seed), pc.value_of(b)
        at = sorted({0, n - 2} | {pc.KD_BLOCK * j - 1 for j in range(1, pc.kate_blocks(n))} | {pc.KD_BLOCK * j for j in range(1, pc.kate_blocks(n)) if pc.KD_BLOCK * j < n - 1})
        at = [i for i in at if 0 <= i < n - 1]           # (n = 1: the quotient is empty)
        assert (q.reshape(-1, 32)[at] == pc.mont([pc.kate_of_last(c, bv, n, i) for i in at]).reshape(-1, 32)).all()
        assert (rem == pc.mont([pc.kate_of_last(c, bv, n, -1)])).all()
    return np.concatenate([q, np.zeros(32, dtype=np.uint8)]), rem


def _kate_single_and_rem(O, n, name, points):
    """sg_fr_kate_division_dev and sg_fr_kate_division_rem_dev on one input class at every point of `points`: quotient, zero
    padding slot, remainder on the host and on the device; the input is unchanged"""
    import torch
    ffi, L = _L()
    nblk = pc.kate_blocks(n)
    d_a = _dev(_vec(O, name, n, 31))
    for point in points:
        b = pc.scalar(O, point, 32)
        want_q, want_rem = _kate_want(O, name, n, b, 31)
        q1, q2, rem_dev, rem = _garbage(32 * n), _garbage(32 * n), _garbage(32), np.zeros(32, dtype=np.uint8)
        ffi.check(L.sg_fr_kate_division_dev(ffi.dev_ptr(d_a), C.c_size_t(n), ffi.ptr(b), ffi.dev_ptr(q1), ffi.ptr(rem), ffi.current_stream_ptr()))
        ffi.check(L.sg_fr_kate_division_rem_dev(ffi.dev_ptr(d_a), C.c_size_t(n), ffi.ptr(b), ffi.dev_ptr(q2), ffi.dev_ptr(rem_dev),
                                                ffi.current_stream_ptr()))
        torch.cuda.synchronize()
        what = f"Kate division n={n} ({nblk} blocks, scan of {pc.kate_scan_threads(nblk)}) {name} by {point if point == 'random' else point % R}"
        d_want = _dev(want_q)
        for entry, q in (("sg_fr_kate_division_dev", q1), ("sg_fr_kate_division_rem_dev", q2)):
            if not torch.equal(q, d_want):
                _same(q, want_q, f"{what}, {entry}")
        _same(rem, want_rem, what + ", remainder on the host")
        _same(rem_dev, want_rem, what + ", remainder on the device")
    torch.cuda.synchronize()
    assert (_host(d_a) == _vec(O, name, n, 31)).all(), f"Kate division n={n} {name}: the input changed"


@pytest.mark.parametrize("n", pc.KATE_SIZES)
def test_kate_division(gpu, O, n):
    """sg_fr_kate_division_dev and sg_fr_kate_division_rem_dev at every width of the block scan (64 .. 1024 threads), exactly full
    (n = 2048 b) and just entered (one coefficient in block b), by b = random, 0, 1 and r - 1: quotient, zero padding slot and
    remainder.  `last`: one coefficient at degree n - 1, so every quotient coefficient is that value times a power of b and a
    wrong weight in any block carry shows"""
    nblk = pc.kate_blocks(n)
    assert nblk in pc.KATE_BLOCK_COUNTS
    small = n <= pc.KATE_ALL_CLASSES_UP_TO
    for name in pc.kate_classes(n):
        _kate_single_and_rem(O, n, name, pc.SCALARS if small or name == "last" else ("random", R - 1))


@pytest.mark.parametrize("n", pc.KATE_SMALL_SIZES)
def test_kate_division_of_one_block(gpu, O, n):
    """the same two entry points where the division is one launch without carries: a constant (n = 1: no quotient coefficient,
    only the padding slot and the remainder), n = 2, and 2047 and 2048 coefficients, the last sizes of one block"""
    assert pc.kate_blocks(n) == 1
    for name in pc.KATE_SMALL_CLASSES:
        _kate_single_and_rem(O, n, name, pc.KATE_SMALL_POINTS)


def test_kate_division_refuses_2_21_plus_1(gpu, O):
    import torch
    ffi, L = _L()
    n = pc.KATE_REFUSED
    a, q, rem_dev, rem = torch.zeros(32 * n, dtype=torch.uint8, device="cuda"), _garbage(32 * n), _garbage(32), np.zeros(32, dtype=np.uint8)
    b = pc.scalar(O, "random", 33)
    assert L.sg_fr_kate_division_dev(ffi.dev_ptr(a), C.c_size_t(n), ffi.ptr(b), ffi.dev_ptr(q), ffi.ptr(rem), ffi.current_stream_ptr()) != 0
    assert L.sg_fr_kate_division_rem_dev(ffi.dev_ptr(a), C.c_size_t(n), ffi.ptr(b), ffi.dev_ptr(q), ffi.dev_ptr(rem_dev), ffi.current_stream_ptr()) != 0
    assert L.sg_fr_kate_division_batch_dev((C.c_void_p * 1)(a.data_ptr()), C.c_size_t(n), ffi.ptr(b), C.c_uint32(1), (C.c_void_p * 1)(q.data_ptr()),
                                           ffi.current_stream_ptr()) != 0
    torch.cuda.synchronize()
    assert bool((q == 0x5A).all())


@pytest.mark.parametrize("blocks", pc.KATE_BATCH_BLOCKS)
def test_kate_division_batch(gpu, O, blocks):
    """sg_fr_kate_division_batch_dev with two divisions of ONE input by different points, at a scan of 128 threads just entered
    and of 1024 threads exactly full"""
    import torch
    ffi, L = _L()
    n = pc.KD_BLOCK * blocks
    for name in ("random", "last"):
        d_a = _dev(_vec(O, name, n, 41))
        pts = np.concatenate([pc.scalar(O, "random", 42), pc.scalar(O, "random" if name == "random" else R - 1, 43)])
        outs = [_garbage(32 * n) for _ in range(2)]
        ffi.check(L.sg_fr_kate_division_batch_dev((C.c_void_p * 2)(d_a.data_ptr(), d_a.data_ptr()), C.c_size_t(n), ffi.ptr(pts), C.c_uint32(2),
                                                  (C.c_void_p * 2)(*[o.data_ptr() for o in outs]), ffi.current_stream_ptr()))
        torch.cuda.synchronize()
        for j, q in enumerate(outs):
            want_q, _ = _kate_want(O, name, n, pts[32 * j:32 * j + 32].copy(), 41)
            _same(q, want_q, f"Kate division batch n={n} {name}, division {j}")


@pytest.mark.parametrize("m", pc.KATE_BATCH_M)
@pytest.mark.parametrize("n", pc.KATE_BATCH_SMALL_SIZES)
def test_kate_division_batch_of_one_and_two_blocks(gpu, O, n, m):
    """sg_fr_kate_division_batch_dev where it runs the write step alone (one block: no carries) and where the first carry
    appears (two blocks, full and with one coefficient in the second): one division, and sixteen divisions of ONE input at
    sixteen different points, into outputs pre-filled with garbage; the input is unchanged"""
    import torch
    ffi, L = _L()
    assert pc.kate_blocks(n) in (1, 2) and m <= pc.KATE_BATCH_MAX
    for name in pc.KATE_SMALL_CLASSES:
        d_a = _dev(_vec(O, name, n, 45))
        drawn = O.random_fr(46, m)
        pts = [drawn[32 * j:32 * j + 32].copy() for j in range(m)]
        if name == "last":
            pts[-1] = pc.scalar(O, R - 1, 0)
        assert len({bytes(p) for p in pts}) == m
        outs = [_garbage(32 * n) for _ in range(m)]
        ffi.check(L.sg_fr_kate_division_batch_dev((C.c_void_p * m)(*[d_a.data_ptr()] * m), C.c_size_t(n), ffi.ptr(np.concatenate(pts)), C.c_uint32(m),
                                                  (C.c_void_p * m)(*[o.data_ptr() for o in outs]), ffi.current_stream_ptr()))
        torch.cuda.synchronize()
        for j, q in enumerate(outs):
            want_q, _ = _kate_want(O, name, n, pts[j], 45)
            _same(q, want_q, f"Kate division batch n={n} m={m} {name}, division {j}")
        assert (_host(d_a) == _vec(O, name, n, 45)).all(), f"Kate division batch n={n} m={m} {name}: the input changed"


# ============================================================================= evaluation
@pytest.mark.parametrize("n", pc.EVAL_SIZES)
def test_eval_polynomial(gpu, O, n):
    """sg_fr_eval_poly_dev around one workgroup's 8192 coefficients, and at 2^21 + 1, where the second level has 257 elements and
    one thread two rows; at x = random, 0, 1 and r - 1"""
    from circuits_halo2_amd.arithmetic import eval_polynomial
    assert len(pc.eval_levels(n)) == (1 if n <= 8192 else 2)
    small = n <= pc.FAST_ABOVE
    for name in pc.EVAL_CLASSES:
        d_a = _dev(_vec(O, name, n, 51))
        for point in (pc.SCALARS if small or name != "max" else ("random",)):
            x = pc.scalar(O, point, 52)
            if name == "last":
                want = pc.mont([pc.eval_of_last(pc.single_value(51), pc.value_of(x), n)])
                assert not small or (want == O.fr_eval_poly(_vec(O, name, n, 51), x)).all()
            else:
                want = O.fr_eval_poly(_vec(O, name, n, 51), x)
            _same(eval_polynomial(d_a, x), want, f"evaluation n={n} {name} at {point if point == 'random' else point % R}")


@pytest.mark.parametrize("n", pc.EVAL_NONCANONICAL_SIZES)
def test_eval_polynomial_of_noncanonical_words(gpu, O, n):
    """the coefficient loader takes any 256-bit word: r, r + 1, 2^256 - 1 and uniform 256-bit words evaluate to what the same
    words reduced mod r (in Python integers) evaluate to in the oracle"""
    from circuits_halo2_amd.arithmetic import eval_polynomial
    w = pc.noncanonical_words(53, n)
    red = pc.reduced(w)
    for point in ("random", 1, R - 1):
        x = pc.scalar(O, point, 54)
        _same(eval_polynomial(_dev(w), x), O.fr_eval_poly(red, x), f"evaluation of non-canonical words n={n} at {point}")


@pytest.mark.parametrize("n,m", pc.EVAL_BATCH_SHAPES)
def test_eval_polynomial_batch(gpu, O, n, m):
    """sg_fr_eval_poly_batch_dev: one and several partials per polynomial, 40 polynomials in one launch and 41 in two"""
    from circuits_halo2_amd.arithmetic import eval_polynomial_batch
    ch, blocks, launches = pc.eval_batch_plan(n, m)
    assert ch == 16 and launches == ([40, 1] if m == 41 else [m])
    names = [pc.EVAL_CLASSES[j % 3] for j in range(m)]
    points = [pc.SCALARS[(j // 3) % 4] if n <= pc.FAST_ABOVE else ("random", R - 1, "random")[j] for j in range(m)]
    devs = {name: _dev(_vec(O, name, n, 61)) for name in set(names)}
    xs = [pc.scalar(O, p, 62 + j) for j, p in enumerate(points)]
    got = eval_polynomial_batch([devs[name] for name in names], np.concatenate(xs))
    for j, (name, x) in enumerate(zip(names, xs)):
        want = O.fr_eval_poly(_vec(O, name, n, 61), x)
        if name == "last":
            assert (want == pc.mont([pc.eval_of_last(pc.single_value(61), pc.value_of(x), n)])).all()
        _same(got[j], want, f"batched evaluation n={n} m={m}, polynomial {j} ({name})")


@pytest.mark.parametrize("n", pc.EVAL_BATCH_TILED)
def test_eval_polynomial_batch_of_a_tiled_polynomial(gpu, O, n):
    """2^24 coefficients are the last full second level of the 16-per-thread kernel (4096 partials), 2^24 + 1 the first size of
    the 32-per-thread instantiation.  The coefficients repeat a random period of 4099 on the device; the expected value is the
    geometric sum P(x) (x^(Lq) - 1) / (x^L - 1) + x^(Lq) P_tail(x) with P and P_tail from the oracle on one period"""
    import torch
    from circuits_halo2_amd.arithmetic import eval_polynomial_batch
    L = pc.EVAL_TILE_PERIOD
    ch, blocks, _ = pc.eval_batch_plan(n, 2)
    assert (ch, blocks) == ((16, 4096) if n == 1 << 24 else (32, 2049))
    period = _vec(O, "random", L, 71)
    d = _dev(period).repeat(n // L + 1)[:32 * n]
    assert d.is_contiguous() and d.numel() == 32 * n
    xs = [pc.scalar(O, "random", 72), pc.scalar(O, R - 1, 0)]
    got = eval_polynomial_batch([d, d], np.concatenate(xs))
    for j, x in enumerate(xs):
        full, tail = pc.value_of(O.fr_eval_poly(period, x)), pc.value_of(O.fr_eval_poly(np.array(period[:32 * (n % L)]), x))
        _same(got[j], pc.mont([pc.eval_of_tiled(full, tail, pc.value_of(x), L, n)]), f"batched evaluation of a tiled polynomial n={n}, point {j}")
    del d
    torch.cuda.empty_cache()


def test_eval_polynomial_batch_refusal_and_noncanonical_words(gpu, O):
    import torch
    from circuits_halo2_amd.arithmetic import eval_polynomial_batch
    assert pc.eval_batch_plan(pc.EVAL_BATCH_REFUSED, 1) is None
    big = torch.empty(32 * pc.EVAL_BATCH_REFUSED, dtype=torch.uint8, device="cuda")
    with pytest.raises(gpu.SummaGpuError):
        eval_polynomial_batch([big], pc.scalar(O, "random", 81))
    del big
    torch.cuda.empty_cache()
    n = pc.EVAL_BATCH_NONCANONICAL
    w = pc.noncanonical_words(82, n)
    red, d = pc.reduced(w), _dev(w)
    xs = [pc.scalar(O, "random", 83), pc.scalar(O, R - 1, 0)]
    got = eval_polynomial_batch([d, d], np.concatenate(xs))
    for j, x in enumerate(xs):
        _same(got[j], O.fr_eval_poly(red, x), f"batched evaluation of non-canonical words, point {j}")


# ============================================================================= linear combinations, element-wise product
def _lincomb_pool(O, name):
    """32 polynomials of 257 rows, their device copies, 32 coefficients and 8 low coefficients of one class; for `noncanonical`
    the polynomials hold any 256-bit words and the oracle gets them reduced mod r"""
    key = ("lincomb", name)
    if key not in _REF:
        n = max(pc.LINCOMB_N)
        if name == "max":
            polys = [pc.vector(O, "max", n, 0)] * pc.LINCOMB_MAX
            coeffs, low = pc.vector(O, "max", pc.LINCOMB_MAX, 0), pc.vector(O, "max", pc.LINCOMB_LOW_MAX, 0)
        else:
            polys = [pc.noncanonical_words(900 + j, n) if name == "noncanonical" else O.random_fr(900 + j, n) for j in range(pc.LINCOMB_MAX)]
            coeffs, low = O.random_fr(940, pc.LINCOMB_MAX), O.random_fr(941, pc.LINCOMB_LOW_MAX)
        ref = [pc.reduced(p) for p in polys] if name == "noncanonical" else polys
        _REF[key] = (ref, [_dev(p) for p in polys], coeffs, low)
    return _REF[key]


@pytest.mark.parametrize("m", pc.LINCOMB_M)
def test_lincomb(gpu, O, m):
    """sg_fr_lincomb_low_dev (and sg_fr_lincomb_dev where there is no low polynomial) around the mid-sum reduction at term 31 and
    around one workgroup's 256 rows; `max`: every polynomial word and every coefficient is r - 1, so each of the products is
    maximal; n_low beyond n is refused"""
    import torch
    from circuits_halo2_amd.arithmetic import lincomb
    ffi, L = _L()
    for name in pc.LINCOMB_CLASSES:
        ref, devs, coeffs, low = _lincomb_pool(O, name)
        cw = np.array(coeffs[:32 * m])
        for n in pc.LINCOMB_N:
            views = [d[:32 * n] for d in devs[:m]]
            base = O.fr_lincomb([np.array(p[:32 * n]) for p in ref[:m]], cw) if m else np.zeros(32 * n, dtype=np.uint8)
            pp = (C.c_void_p * m)(*[v.data_ptr() for v in views]) if m else None
            for n_low in pc.LINCOMB_N_LOW:
                nl = n if n_low == "n" else n_low
                if nl > pc.LINCOMB_LOW_MAX:
                    continue
                out = _garbage(32 * n)
                rc = L.sg_fr_lincomb_low_dev(pp, ffi.ptr(cw) if m else None, C.c_uint32(m), C.c_size_t(n), ffi.ptr(low) if nl else None, C.c_uint32(nl),
                                             ffi.dev_ptr(out), ffi.current_stream_ptr())
                what = f"linear combination {name} m={m} n={n} n_low={nl}"
                if nl > n:
                    assert rc != 0, what + ": accepted"
                    continue
                ffi.check(rc)
                want = base.copy()
                for i in range(nl):
                    want[32 * i:32 * i + 32] = O.fr_add(_row(base, i), _row(low, i))
                _same(out, want, what)
                if m and not nl:
                    _same(lincomb(views, cw), want, what + " (sg_fr_lincomb_dev)")
    torch.cuda.synchronize()


@pytest.mark.parametrize("name,n,sizes,lows", [
    ("prover", 1 << 17, [5, 25, 3, 2, 4], [2, 3, 4, 2, 3]),
    ("limits", 5000, [32, 0, 3, 3, 3, 3, 2, 2], [1, 4, 0, 2, 3, 4, 1, 0]),
    ("n=1", 1, [3, 1, 0], [1, 0, 1]),
    ("n=3", 3, [2, 5, 0], [3, 1, 2]),
    ("n=2^17+1", (1 << 17) + 1, [32, 1, 0, 4], [4, 0, 3, 2]),
])
def test_lincomb_sets_of_maximal_words(gpu, O, name, n, sizes, lows):
    """sg_fr_lincomb_sets_dev at the shapes of test_lincomb_sets_against_the_oracle with every polynomial word, coefficient and
    low coefficient equal to r - 1"""
    import torch
    from circuits_halo2_amd import arithmetic as A
    poly = _vec(O, "max", n, 0)
    d_poly = _dev(poly)
    sets, want = [], []
    for m, nl in zip(sizes, lows):
        coeffs, low = pc.vector(O, "max", m, 0), pc.vector(O, "max", nl, 0)
        out = O.fr_lincomb([poly] * m, coeffs) if m else np.zeros(32 * n, dtype=np.uint8)
        for i in range(nl):
            out[32 * i:32 * i + 32] = O.fr_add(_row(out, i), _row(low, i))
        sets.append(([d_poly] * m, coeffs, low if nl else None))
        want.append(out)
    outs = [_garbage(32 * n) for _ in sets]
    A.fr_lincomb_sets(sets, n, outs)
    torch.cuda.synchronize()
    for s, (got, w) in enumerate(zip(outs, want)):
        _same(got, w, f"{name} set {s}")


@pytest.mark.parametrize("n", pc.MUL_SIZES)
def test_fr_mul_of_maximal_words(gpu, O, n):
    from circuits_halo2_amd.arithmetic import fr_mul
    mx, one = _vec(O, "max", n, 0), _vec(O, "one", n, 0)
    _same(fr_mul(_dev(mx), _dev(mx)), O.fr_mul_n(mx, mx), f"max * max n={n}")
    _same(fr_mul(_dev(mx), _dev(one)), O.fr_mul_n(mx, one), f"max * one n={n}")
    _same(fr_mul(_dev(one), _dev(mx)), mx, f"one * max n={n}")


# ============================================================================= grand products
def _vanish_permutation(vals, sig, beta, gamma, rows):
    """v = -(beta sigma + gamma) at `rows`: the denominator's factor of this column vanishes there"""
    bv, gv = pc.value_of(beta), pc.value_of(gamma)
    for r in rows:
        vals[32 * r:32 * r + 32] = pc.mont([-(bv * pc.value_of(sig[32 * r:32 * r + 32]) + gv)])


def _vanish_lookup(ap, beta, rows):
    for r in rows:
        ap[32 * r:32 * r + 32] = pc.mont([-pc.value_of(beta)])


@pytest.mark.parametrize("k,ncols", [(11, 2), (21, 1)])
def test_permutation_product(gpu, O, k, ncols):
    """sg_permutation_product_dev where n is exactly one block, and at k = 21: 1024 blocks, which the block count computed
    from n + 1 refused ("grand product") although only n rows are written; z[0] = z0 is carried through every block"""
    from circuits_halo2_amd.arithmetic import permutation_product
    n = 1 << k
    assert pc.prefix_blocks(n, n) == (1 if k == 11 else 1024) and (k != 21 or pc.prefix_blocks_before_the_fix(n, n) is None)
    vals = [pc.random_words(O, 1100 + c, n) for c in range(ncols)]
    sig = [pc.random_words(O, 1200 + c, n) for c in range(ncols)]
    beta, gamma, z0 = pc.scalar(O, "random", 1301), pc.scalar(O, "random", 1302), pc.scalar(O, "random", 1303)
    d_vals, d_sig = [_dev(v) for v in vals], [_dev(s) for s in sig]
    for init in ((z0, None) if k == 11 else (z0,)):
        want = O.permutation_product(vals, sig, beta, gamma, pc.mont([1]), k, init)
        _same(permutation_product(d_vals, d_sig, beta, gamma, pc.mont([1]), k, init), want, f"permutation product k={k}, z0 {'given' if init is not None else 'absent'}")


def test_lookup_product_at_2_21_minus_1(gpu, O):
    from circuits_halo2_amd.arithmetic import lookup_product
    n = (1 << 21) - 1
    assert pc.prefix_blocks(n, n) == 1024
    cols = [pc.fast_words(1400 + i, n) for i in range(4)]
    beta, gamma = pc.scalar(O, "random", 1411), pc.scalar(O, "random", 1412)
    _same(lookup_product(*[_dev(c) for c in cols], beta, gamma), O.lookup_product(*cols, beta, gamma), "lookup product n=2^21-1")


def test_products_with_vanishing_denominators(gpu, O):
    """a zero denominator's inverse stays zero (ff::BatchInvert), so z is zero behind such a row: at row 0, at a row in the middle
    and at the last row (tests/test_poly_cases_cpu.py checks the oracle's side against Python integers)"""
    from circuits_halo2_amd.arithmetic import lookup_product, permutation_product
    k, n = 11, 2048
    beta, gamma = pc.scalar(O, "random", 1501), pc.scalar(O, "random", 1502)
    for rows in (pc.vanishing_rows(n), pc.vanishing_rows(n, "late rows")):
        vals, sig = [O.random_fr(1510 + c, n) for c in range(2)], [O.random_fr(1520 + c, n) for c in range(2)]
        _vanish_permutation(vals[1], sig[1], beta, gamma, rows)
        want = O.permutation_product(vals, sig, beta, gamma, pc.mont([1]), k)
        assert not want[32 * (rows[0] + 1):].any() and want[32 * rows[0]:32 * rows[0] + 32].any()
        _same(permutation_product([_dev(v) for v in vals], [_dev(s) for s in sig], beta, gamma, pc.mont([1]), k), want, f"permutation product, rows {rows}")
        a, s, ap, sp = (O.random_fr(1530 + i, n) for i in range(4))
        _vanish_lookup(ap, beta, rows)
        want = O.lookup_product(a, s, ap, sp, beta, gamma)
        assert not want[32 * (rows[0] + 1):].any() and want[32 * rows[0]:32 * rows[0] + 32].any()
        _same(lookup_product(_dev(a), _dev(s), _dev(ap), _dev(sp), beta, gamma), want, f"lookup product, rows {rows}")


@pytest.mark.parametrize("k,chunks,n_lookups,usable,vanishing", pc.GRAND_CASES, ids=[f"k{c[0]}-{'+'.join(map(str, c[1]))}-{c[2]}-u{c[3]}" + (f"-vanishing {c[4]}" if c[4] else "") for c in pc.GRAND_CASES])
def test_grand_products_batched(gpu, O, k, chunks, n_lookups, usable, vanishing):
    """sg_grand_products_closing_dev (and sg_grand_products_dev up to k = 18) against the oracle's products chained by hand: chunk
    j starts from chunk j - 1's value at row `usable`; closing[p] = z_p[usable].  k = 18 .. 21 (21: 1024 blocks per product),
    usable rows 0, n - 1 and on a 2048 boundary, vanishing denominators in a permutation chunk and in a lookup"""
    import torch
    from oracle import pyref
    from circuits_halo2_amd.arithmetic import grand_products
    ffi, L = _L()
    n = 1 << k
    assert pc.grand_blocks(n) == n // pc.PP_BLOCK
    beta, gamma = pc.scalar(O, "random", 2301 + k), pc.scalar(O, "random", 2302 + k)
    perm, want, col, z0 = [], [], 0, None
    for j, nc in enumerate(chunks):
        vals = [pc.random_words(O, 2100 + 100 * k + col + c, n) for c in range(nc)]
        sig = [pc.random_words(O, 2200 + 100 * k + col + c, n) for c in range(nc)]
        if vanishing and j == 0:
            _vanish_permutation(vals[0], sig[0], beta, gamma, pc.vanishing_rows(n, vanishing))
        z = O.permutation_product(vals, sig, beta, gamma, pc.mont([pow(pyref.DELTA, col, R)]), k, z0)
        want.append(z)
        z0 = _row(z, usable)
        perm.append(([_dev(v) for v in vals], [_dev(s) for s in sig]))
        col += nc
    lookups = []
    for l in range(n_lookups):
        cols = [pc.random_words(O, 2400 + 10 * l + i + k, n) for i in range(4)]
        if vanishing:
            _vanish_lookup(cols[2], beta, pc.vanishing_rows(n, vanishing))
        want.append(O.lookup_product(*cols, beta, gamma))
        lookups.append(tuple(_dev(c) for c in cols))
    if vanishing:
        r0 = pc.vanishing_rows(n, vanishing)[0]
        assert all(not w[32 * (r0 + 1):].any() and _row(w, r0).any() for w in (want[0], want[-1]))
    total = len(chunks) + n_lookups
    vals_, sigs_ = [v for ch in perm for v in ch[0]], [s for ch in perm for s in ch[1]]
    zs = [_garbage(32 * n) for _ in range(total)]
    closing = _garbage(32 * total)
    arr = lambda ts: (C.c_void_p * max(1, len(ts)))(*[t.data_ptr() for t in ts])
    ffi.check(L.sg_grand_products_closing_dev(arr(vals_), arr(sigs_), (C.c_uint32 * len(chunks))(*chunks), C.c_uint32(len(chunks)),
                                              arr([t for lu in lookups for t in lu]), C.c_uint32(n_lookups), ffi.ptr(beta), ffi.ptr(gamma), C.c_uint32(k),
                                              C.c_size_t(usable), arr(zs), ffi.dev_ptr(closing), ffi.current_stream_ptr()))
    torch.cuda.synchronize()
    got_closing = _host(closing)
    for p, (z, w) in enumerate(zip(zs, want)):
        _same(z, w, f"grand products k={k} {chunks} + {n_lookups}, usable {usable}: product {p}")
        _same(got_closing[32 * p:32 * p + 32], _row(w, usable), f"grand products k={k}: closing value of product {p}")
    if k <= 18:
        got_z, got_l = grand_products(perm, lookups, beta, gamma, k, usable)
        for p, (z, w) in enumerate(zip(got_z + got_l, want)):
            _same(z, w, f"sg_grand_products_dev k={k} {chunks} + {n_lookups}, usable {usable}: product {p}")


def test_grand_products_refuse_k_22(gpu, O):
    from circuits_halo2_amd.arithmetic import grand_products
    import torch
    col = torch.zeros(32 << 22, dtype=torch.uint8, device="cuda")
    with pytest.raises(gpu.SummaGpuError, match="1 <= k <= 21"):
        grand_products([([col], [col])], [], pc.scalar(O, "random", 1), pc.scalar(O, "random", 2), 22, 10)
