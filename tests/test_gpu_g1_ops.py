"""The set-up time operations on G1 (csrc/g1_ops.hip: fixed-base products, the FFT over G1, prefix sums of a basis, the fixed-base
window table, the on-curve check) and the scalar half of the KZG set-up (kzg_setup_scalars, csrc/summa_gpu.hip) against the
oracle, at the block edges of their launches and on the inputs where the group law leaves its generic branch.

tests/g1_cases.py restates the geometry and lists the cases; tests/test_g1_cases_cpu.py asserts, without a GPU, that they reach
every shape of the scan's level list and the doubling, cancelling and identity operand pairs at the stages and kernels claimed.

Every input point is s * G for a known scalar s, so every expected point is O.fixed_base_mul of a scalar computed in Fr (by
O.best_fft, O.fr_dot, O.fr_mul_n or Python integers); every comparison is byte for byte on 64-byte points."""
import ctypes as C

import numpy as np
import pytest

import g1_cases as gc

pytestmark = pytest.mark.gpu

R = gc.R
_POINTS = {}          # scalar -> the 64 bytes of scalar * G, from the oracle (shared by every test, read only)


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
    return torch.from_numpy(np.array(a)).cuda()


def _points(O, scalars):
    """scalars[i] * G from the oracle, n x 64 bytes; every distinct scalar is multiplied once per module"""
    keys = [v % R for v in scalars]
    new = sorted(set(keys) - set(_POINTS))
    if new:
        pts = O.fixed_base_mul(gc.mont(new), O.ncpu()).reshape(-1, 64)
        _POINTS.update(zip(new, (bytes(p) for p in pts)))
    return np.frombuffer(b"".join(_POINTS[v] for v in keys), dtype=np.uint8).copy()


def _scalar_points(O, fr_bytes):
    """the same for scalars that arrive as Montgomery words"""
    return O.fixed_base_mul(np.ascontiguousarray(fr_bytes), O.ncpu())


def _same_points(got, want, what):
    g = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    g, want = g.reshape(-1), np.asarray(want).reshape(-1)
    assert g.size == want.size and g.size % 64 == 0, f"{what}: {g.size} bytes, {want.size} expected"
    bad = (g.reshape(-1, 64) != want.reshape(-1, 64)).any(axis=1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} points differ, first at {int(np.argmax(bad))}"


def _logged(ffi, fn):
    """fn() with the launch log on -> (result, records)"""
    with ffi.params({"msm.acc_log": 1}):
        out = fn()
        log = ffi.msm_launch_log()
    return out, log


# ============================================================================= 1: fixed-base products
@pytest.mark.parametrize("n", gc.FIXED_BASE_SIZES)
def test_fixed_base_mul_at_block_edges(gpu, O, n):
    """sg_g1_fixed_base_mul (host) and sg_g1_fixed_base_mul_dev at n = 1, 255, 256, 257, 513 with 0, 1, 2, r - 1, r - 2, the two
    halves of r, every 2^b and the full low words at the end of the last block (n = 1: the named values, the bits next to a word
    boundary and the top bit, one launch each); the row behind the output stays untouched"""
    import torch
    from circuits_halo2_amd import ffi
    from circuits_halo2_amd.arithmetic import g1_fixed_base_mul
    guard = np.full(64, 0xA5, dtype=np.uint8)
    for v, vec in enumerate(gc.fixed_base_vectors(n)):
        want = _points(O, vec)
        if vec[-1] == 0:
            assert not want[-64:].any()
        sc = gc.mont(vec)
        _same_points(g1_fixed_base_mul(sc), want, f"fixed-base products n={n} vector {v}, host entry")
        out = _dev(np.concatenate([np.zeros(64 * n, dtype=np.uint8), guard]))
        ffi.check(ffi.lib().sg_g1_fixed_base_mul_dev(ffi.dev_ptr(_dev(sc)), C.c_size_t(n), ffi.dev_ptr(out), ffi.current_stream_ptr()))
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        _same_points(got[:64 * n], want, f"fixed-base products n={n} vector {v}, device entry")
        assert (got[64 * n:] == guard).all(), f"fixed-base products n={n} vector {v}: the row behind the output changed"


def test_fixed_base_mul_of_unreduced_words(gpu, O):
    """Montgomery words m~ + r (the same residue, not below r): the product is that of the reduced twin"""
    from circuits_halo2_amd.arithmetic import g1_fixed_base_mul
    values = gc.fixed_base_unreduced_values()
    want = _points(O, values)
    _same_points(g1_fixed_base_mul(gc.unreduced(values)), want, "fixed-base products of unreduced words, host entry")
    _same_points(g1_fixed_base_mul(_dev(gc.unreduced(values))), want, "fixed-base products of unreduced words, device entry")


# ============================================================================= 2: FFT over G1
def _g1_fft(points, w, scale, log_n):
    import torch
    from circuits_halo2_amd import ffi
    d_in = _dev(points)
    d_out = torch.full((64 << log_n,), 0x5A, dtype=torch.uint8, device="cuda")
    sc = gc.mont([scale]) if scale is not None else None
    ffi.check(ffi.lib().sg_g1_fft_dev(ffi.dev_ptr(d_in), ffi.dev_ptr(d_out), ffi.ptr(gc.mont([w])), ffi.ptr(sc) if sc is not None else None,
                                      C.c_uint32(log_n), ffi.current_stream_ptr()))
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


@pytest.mark.parametrize("log_n", gc.FFT_LOGS)
def test_g1_fft(gpu, O, log_n):
    """sg_g1_fft_dev over in[i] = s_i G against fixed_base_mul(scale * best_fft(s)): both roots, scale NULL / 1/n / 1 / 0, and the
    scalar patterns that make a butterfly double, cancel or carry the identity (g1_cases.fft_claims; g1_cases.fft_cases pairs
    them); the inverse transform must also be what sg_g1_to_lagrange returns"""
    from circuits_halo2_amd import ffi
    n = 1 << log_n
    cases = [c[1:] for c in gc.fft_cases() if c[0] == log_n]
    for pattern in gc.FFT_PATTERNS:
        for root in gc.FFT_ROOTS:
            w = gc.fft_root(root, log_n)
            s = gc.fft_scalars(pattern, log_n, root)
            points = _points(O, s)
            spectrum = O.best_fft(gc.mont(s), gc.mont([w]), log_n)
            for scale_name in [sc for r, sc, p in cases if (r, p) == (root, pattern)]:
                scale = gc.fft_scale(scale_name, log_n)
                e = spectrum if scale is None else O.fr_mul_n(spectrum, np.tile(gc.mont([scale]), n))
                want = _scalar_points(O, e)
                if scale == 0:
                    assert not want.any()
                _same_points(_g1_fft(points, w, scale, log_n), want, f"G1 FFT log_n={log_n} {pattern} {root} scale={scale_name}")
                if root == "omega_inv" and scale_name == "n_inv":
                    gl = np.zeros(64 * n, dtype=np.uint8)
                    ffi.check(ffi.lib().sg_g1_to_lagrange(ffi.ptr(points), C.c_uint32(log_n), ffi.ptr(gl)))
                    _same_points(gl, want, f"sg_g1_to_lagrange k={log_n} {pattern}")


# ============================================================================= 3: prefix sums and window tables
@pytest.mark.parametrize("pattern", gc.PREFIX_PATTERNS)
@pytest.mark.parametrize("k", list(gc.PREFIX_KS))
def test_prefix_sums(gpu, O, k, pattern):
    """sg_srs_precompute(basis 2) over g_lagrange[i] = s_i G: Q_j = (s_0 + .. + s_j) G is read through the difference-form
    commitment of the step column (1 on rows 0..j), at the chunk and level boundaries; then a random and a piecewise-constant
    column in difference form against fixed_base_mul(<col, s>).  Only the prefix table exists, so a fixed-base record in the
    launch log is a job that read it"""
    from circuits_halo2_amd import ffi
    n = 1 << k
    assert gc.prefix_levels(n) == gc.PREFIX_KS[k]
    s = gc.prefix_scalars(pattern, k)
    gl = _points(O, s)
    q = gc.running_sums(s)
    rows = gc.prefix_probe_rows(n)
    params = gpu.ParamsKZG(k, gl, gl)
    try:
        params.precompute(2)
        got, log = _logged(ffi, lambda: params.commit_batch([_dev(gc.step_column(j, n)) for j in rows], lagrange=True, diff=True))
        assert log and all(r["fixed"] == 1 and r["n"] == n for r in log) and sum(r["M"] for r in log) == len(rows), log
        want = _points(O, [q[j] for j in rows])
        if pattern == "cancel32" and n > 32:
            assert not want[64 * rows.index(32):64 * rows.index(32) + 64].any()
        _same_points(got, want, f"prefix sums k={k} {pattern}, Q_j at j={rows}")
        s_mont = gc.mont(s)
        cols = [O.random_fr(0x91 + k, n), gc.mont(gc.piecewise_values(n))]
        want = np.concatenate([_scalar_points(O, O.fr_dot(c, s_mont)) for c in cols])
        got, log = _logged(ffi, lambda: params.commit_batch([_dev(c) for c in cols], lagrange=True, diff=True))
        assert [(r["fixed"], r["n"], r["M"]) for r in log] == [(1, n, 2)], log
        _same_points(got, want, f"difference-form commitments k={k} {pattern}")
        got, log = _logged(ffi, lambda: np.concatenate([params._commit(2, _dev(c)) for c in cols]))
        assert [(r["fixed"], r["n"], r["M"]) for r in log] == [(1, n, 1)] * 2, log
        _same_points(got, want, f"difference-form commitments k={k} {pattern}, one at a time")
    finally:
        params.free()


@pytest.mark.parametrize("window_bits", gc.TABLE_WINDOW_BITS)
@pytest.mark.parametrize("k", gc.TABLE_KS)
def test_window_tables(gpu, O, k, window_bits):
    """sg_srs_precompute(basis 0 and 1) at window widths 4, 7, 13, 16 and the default: 254 columns that hold 2^b in one row read
    one table row each (msm_table_step row by row); a column of r - 1; a random column -- over a basis with identities, repeated
    and opposite points (g) and a generic one (g_lagrange).  The launch log shows fixed-base jobs only"""
    from circuits_halo2_amd import ffi
    n = 1 << k
    c = window_bits or gc.default_window_bits(n)
    assert {gc.table_row_of_bit(c, b) for b in gc.TABLE_BITS} == set(range(len(gc.window_widths(c))))
    t = [gc.table_basis_scalars(k, basis) for basis in (0, 1)]
    bases = [_points(O, t[0]), _points(O, t[1])]
    one, minus_one = gc.mont([1]), gc.mont([R - 1])
    params = gpu.ParamsKZG(k, bases[0], bases[1])
    try:
        for basis in (0, 1):
            params.precompute(basis, window_bits=window_bits)
            cols = np.zeros((len(gc.TABLE_BITS), n, 32), dtype=np.uint8)
            for b in gc.TABLE_BITS:
                cols[b, gc.table_bit_row(b, n)] = gc.mont([1 << b])
            d_cols = _dev(cols.reshape(len(gc.TABLE_BITS), -1))
            got, log = _logged(ffi, lambda: params.commit_batch([d_cols[b] for b in gc.TABLE_BITS], lagrange=bool(basis)))
            assert log and all(r["fixed"] == 1 and r["n"] == n for r in log) and sum(r["M"] for r in log) == len(gc.TABLE_BITS), log
            want = _points(O, [t[basis][gc.table_bit_row(b, n)] << b for b in gc.TABLE_BITS])
            _same_points(got, want, f"window table k={k} c={c} basis {basis}, single-entry columns 2^b")
            t_mont = gc.mont(t[basis])
            cols2 = [np.tile(minus_one, n), O.random_fr(0x77 + k + basis, n), np.tile(one, n)]
            want = np.concatenate([_scalar_points(O, O.fr_dot(col, t_mont)) for col in cols2])
            assert (want[:64] == _points(O, [-sum(t[basis])])).all()
            assert (want == np.concatenate([O.best_multiexp(col, bases[basis], O.ncpu()) for col in cols2])).all()
            got, log = _logged(ffi, lambda: np.concatenate([params._commit(basis, _dev(col)) for col in cols2]))
            assert [(r["fixed"], r["n"], r["M"]) for r in log] == [(1, n, 1)] * 3, log
            _same_points(got, want, f"window table k={k} c={c} basis {basis}, columns of r - 1, random, 1")
            got, log = _logged(ffi, lambda: np.concatenate([params._commit(basis, col) for col in cols2]))
            assert [(r["fixed"], r["n"], r["M"]) for r in log] == [(1, n, 1)] * 3, log
            _same_points(got, want, f"window table k={k} c={c} basis {basis}, host entry")
    finally:
        params.free()


# ============================================================================= 4: on-curve check
@pytest.fixture(scope="module")
def curve_bases(O):
    return {k: [_points(O, s) for s in gc.curve_scalars(k)] for k in gc.CURVE_KS}


@pytest.mark.parametrize("name,k,spoiled", gc.curve_cases(), ids=[c[0] for c in gc.curve_cases()])
def test_srs_check_counts_the_bad_points(gpu, O, curve_bases, name, k, spoiled):
    """ParamsKZG.check() / sg_srs_check at k = 1, 8, 9 (two points, one block, two blocks): identities and (x, -y) are good; a
    point with y + 1, with x and y swapped, or with a coordinate stored as x~ + q / y~ + q (on the curve as a residue, refused by
    halo2curves' from_raw_bytes because the words are not below q) is bad, wherever it sits, and the count is exact"""
    from circuits_halo2_amd import ffi
    bases = [b.copy() for b in curve_bases[k]]
    for basis, idx, how in spoiled:
        bases[basis][64 * idx:64 * idx + 64] = gc.spoil(bases[basis][64 * idx:64 * idx + 64], how)
    params = gpu.ParamsKZG(k, bases[0], bases[1])
    try:
        bad = C.c_uint64(123)
        ffi.check(ffi.lib().sg_srs_check(C.c_uint64(params.handle()), C.byref(bad)))
        assert bad.value == len(spoiled), f"{name}: {bad.value} points reported, {len(spoiled)} spoiled"
        if spoiled:
            with pytest.raises(ValueError, match=f"Failed to read params: {len(spoiled)} points"):
                params.check()
        else:
            params.check()
    finally:
        params.free()


# ============================================================================= 5: KZG set-up
@pytest.mark.parametrize("k", gc.SETUP_KS)
def test_kzg_setup_against_the_definition(gpu, O, k):
    """ParamsKZG.setup at k = 0, 1, 5, 8 for tau random, 0, 1, omega^3 and r - 1: g[i] = tau^i G, g_lagrange[i] = L_i(tau) G with
    L from Python integers -- L_j(omega^j) = 1 and 0 elsewhere when tau lies in the domain -- and g_lagrange is the inverse G1
    FFT of g, as upstream derives it"""
    from circuits_halo2_amd import ffi
    n = 1 << k
    for name, tau in gc.setup_taus(k):
        params = gpu.ParamsKZG.setup(k, gc.mont([tau]))
        _same_points(params.g, _scalar_points(O, O.fr_powers(gc.mont([tau]), n)), f"setup k={k} tau={name}: g")
        _same_points(params.g_lagrange, _points(O, gc.lagrange_at(tau, k)), f"setup k={k} tau={name}: g_lagrange")
        gl = np.zeros(64 * n, dtype=np.uint8)
        ffi.check(ffi.lib().sg_g1_to_lagrange(ffi.ptr(params.g), C.c_uint32(k), ffi.ptr(gl)))
        _same_points(params.g_lagrange, gl, f"setup k={k} tau={name}: g_lagrange against sg_g1_to_lagrange(g)")
