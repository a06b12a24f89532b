"""GPU tests of the quotient's coset pipeline at every coset count the C ABI accepts (1 .. 8, at most 2^(ext_k - k)): the forward
transform sg_coeff_to_cosets_batch_dev with the shift folded into the first NTT pass and in a pass of its own, the coset-major
sg_quotient_*_cosets_dev kernels, and the closing sg_cosets_to_pieces_dev -- on 8, 32, 128, 256 and 512 rows per coset, and once
at 2^19.

Every expected value comes from tests/coset_cases.py (the oracle and Python integers; tests/test_coset_cases_cpu.py ties it to
halo2's extended-domain functions); nothing here compares one library setting with another, and no expected value passes
through the library."""
import ctypes as C

import numpy as np
import pytest

import coset_cases as cc

pytestmark = pytest.mark.gpu

# documented defaults of the parameters set here, restored by value
DEFAULTS = {"quotient.fused_numerator": 1, "ntt.coset_scale_pass": 0}
SG_ERR_INVALID = -1
LAST_ROT = 6                 # blinding factors + 1
SHAPES = cc.shapes()
_ids = lambda s: "k%d-ext%d-nc%d" % (s[0] if isinstance(s[0], tuple) else s)


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    import circuits_halo2_amd as sg
    from circuits_halo2_amd import ffi
    ffi.check(sg.lib().sg_init(0))
    _restore_defaults()
    yield sg
    _restore_defaults()


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    oracle.set_quotient_threads(cc.threads())
    yield oracle
    oracle.set_quotient_threads(1)


def _restore_defaults():
    from circuits_halo2_amd import ffi
    for name, value in DEFAULTS.items():
        ffi.set_param(name, value)


def _set(name, value):
    from circuits_halo2_amd import ffi
    ffi.set_param(name, value)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _domain(shape, how):
    from circuits_halo2_amd.domain import EvaluationDomain
    k, ext, nc = shape
    j, arg = how
    dom = EvaluationDomain(j, k)
    assert dom.extended_k == k + ext and (dom.quotient_poly_degree if arg is None else arg) == nc
    return dom, arg


def _mismatch(got, want, what):
    """None, or how many rows differ and where the first one is"""
    g = got.cpu().numpy() if hasattr(got, "cpu") else got
    if g.size != want.size:
        return f"{what}: {g.size} bytes, {want.size} expected"
    bad = (g.reshape(-1, 32) != want.reshape(-1, 32)).any(axis=1)
    return f"{what}: {int(bad.sum())} of {bad.size} rows differ, first at row {int(np.argmax(bad))}" if bad.any() else None


def _assert_rows(got, want, what=""):
    """bit for bit; on a mismatch say how many rows differ and where the first one is"""
    msg = _mismatch(got, want, what)
    assert msg is None, msg


# ============================================================================= a. cosets_to_pieces from known pieces
@pytest.mark.parametrize("shape,how", SHAPES, ids=[_ids(s) for s, _ in SHAPES])
def test_cosets_to_pieces_returns_known_pieces(gpu, O, shape, how):
    """random pieces -> the coset-major values of h (X^n - 1) by the oracle (cc.numerator_from_pieces) -> sg_cosets_to_pieces_dev
    gives the pieces back: coset_combine_kernel<5> at 5 cosets, coset_combine_any_kernel at every other count (8 cosets: all 64
    matrix entries staged; k < 8: a partly idle workgroup); k = 19: the transforms of the blocks one by one"""
    import torch
    k, ext, nc = shape
    dom, arg = _domain(shape, how)
    pieces = [O.random_fr(21000 + 100 * k + 10 * ext + nc + 1000 * t, 1 << k) for t in range(nc)]
    values = _dev(cc.numerator_from_pieces(pieces, k, ext, nc))
    got = dom.cosets_to_pieces(values, arg)
    torch.cuda.synchronize()
    assert len(got) == nc
    for t in range(nc):
        _assert_rows(got[t], pieces[t], f"piece {t}")


# ============================================================================= b. cosets_to_pieces of arbitrary values
_B_SHAPES = [(s, h) for s, h in SHAPES if s[0] in (3, 5, 8)]


@pytest.mark.parametrize("shape,how", _B_SHAPES, ids=[_ids(s) for s, _ in _B_SHAPES])
def test_cosets_to_pieces_of_arbitrary_values(gpu, O, shape, how):
    """values that are the image of no pieces (random words, zeros, the word r - 1, -1, a single non-zero last row): the pieces
    equal cc.ref_cosets_to_pieces (inverse transform per block, c_b^-i, Vandermonde solve with Python integers)"""
    import torch
    k, ext, nc = shape
    dom, arg = _domain(shape, how)
    rows = nc << k
    failures = []
    for name, fill in cc.value_fills():
        values = fill(rows, 22000 + 100 * k + 10 * ext + nc)
        want = cc.ref_cosets_to_pieces(values, k, ext, nc)
        got = dom.cosets_to_pieces(_dev(values), arg)
        torch.cuda.synchronize()
        assert len(got) == nc
        failures += [_mismatch(got[t], want[t], f"{name}, piece {t}") for t in range(nc)]
    failures = [f for f in failures if f]
    assert not failures, "; ".join(failures)


@pytest.mark.parametrize("case", ["pieces_overlap_values", "n_cosets_0", "n_cosets_9", "n_cosets_above_2^ext", "ext_k_equals_k"])
def test_cosets_to_pieces_refuses_and_writes_nothing(gpu, O, case):
    """the documented refusals of sg_cosets_to_pieces_dev through the C ABI: SG_ERR_INVALID each, and neither the values nor
    the pieces are touched; the valid call next to it still works"""
    import torch
    from circuits_halo2_amd import ffi
    k, ext, nc = 5, 2, 3
    n = 1 << k
    pattern = O.random_fr(23000, 9 * n)                        # room for nine blocks: no refused call could run past it
    piece_fill = np.full(32 * n, 0xA5, dtype=np.uint8)
    values = _dev(pattern)
    pieces = [_dev(piece_fill) for _ in range(9)]
    ptrs = [p.data_ptr() for p in pieces]
    ext_k, count = k + ext, nc
    if case == "pieces_overlap_values":
        ptrs[2] = values.data_ptr() + 32 * n * nc - 32         # its first row is the values' last row
    elif case == "n_cosets_0":
        count = 0
    elif case == "n_cosets_9":
        ext_k, count = k + 4, 9
    elif case == "n_cosets_above_2^ext":
        ext_k, count = k + 1, 3
    elif case == "ext_k_equals_k":
        ext_k, count = k, 1
    pp = (C.c_void_p * 9)(*ptrs)
    torch.cuda.synchronize()
    rc = ffi.lib().sg_cosets_to_pieces_dev(ffi.dev_ptr(values), pp, C.c_uint32(k), C.c_uint32(ext_k), C.c_uint32(count),
                                           ffi.current_stream_ptr())
    torch.cuda.synchronize()
    assert rc == SG_ERR_INVALID, f"{case}: status {rc}"
    _assert_rows(values, pattern, f"{case}: a refused call wrote the values")
    for t, p in enumerate(pieces):
        _assert_rows(p, piece_fill, f"{case}: a refused call wrote piece {t}")
    from circuits_halo2_amd.domain import EvaluationDomain
    known = [O.random_fr(23100 + t, n) for t in range(nc)]
    got = EvaluationDomain(nc + 1, k).cosets_to_pieces(_dev(cc.numerator_from_pieces(known, k, ext, nc)))
    torch.cuda.synchronize()
    for t in range(nc):
        _assert_rows(got[t], known[t], f"valid call after a refused one, piece {t}")


# ============================================================================= c. forward transform
_FWD_WANT = {}


def _columns(O, k, count, seed):
    """`count` coefficient columns: random, but for one of all r - 1 words and one of all zero (count 1: a batch each)"""
    n = 1 << k
    cols = [O.random_fr(seed + j, n) for j in range(count)]
    if count == 1:
        return [cols, [cc.max_word(n)], [np.zeros(32 * n, dtype=np.uint8)]]
    cols[1 if count == 3 else 5] = cc.max_word(n)
    cols[count - 1] = np.zeros(32 * n, dtype=np.uint8)                 # 17 columns: one in either chunk of the scale pass
    return [cols]


def _forward(O, shape, how, count, scale_pass):
    import torch
    k, ext, nc = shape
    dom, arg = _domain(shape, how)
    key = (shape, count)
    if key not in _FWD_WANT:
        batches = _columns(O, k, count, 24000 + 100 * k + 10 * ext + nc)
        _FWD_WANT[key] = (batches, [[cc.gather(O.coeff_to_extended(c, k, k + ext, cc.threads()), k, ext, nc) for c in b] for b in batches])
    batches, wants = _FWD_WANT[key]
    for host, want in zip(batches, wants):
        cols = [_dev(c) for c in host]
        try:
            _set("ntt.coset_scale_pass", scale_pass)
            outs = dom.coeff_to_cosets_batch(cols, arg)
            torch.cuda.synchronize()
        finally:
            _restore_defaults()
        assert len(outs) == len(host)
        for j, (got, w) in enumerate(zip(outs, want)):
            _assert_rows(got, w, f"column {j} of {len(host)}")
        for j, (c, c0) in enumerate(zip(cols, host)):
            _assert_rows(c, c0, f"input {j} was written")


_C_SHAPES = [(s, h) for s, h in SHAPES if s[0] <= 9]


@pytest.mark.parametrize("scale_pass", [0, 1])
@pytest.mark.parametrize("count", [1, 3])
@pytest.mark.parametrize("shape,how", _C_SHAPES, ids=[_ids(s) for s, _ in _C_SHAPES])
def test_forward_transform_against_the_oracle(gpu, O, shape, how, count, scale_pass):
    """sg_coeff_to_cosets_batch_dev = the coset-major gather of the oracle's coeff_to_extended, with the shift on the load of
    the first NTT pass (ntt.coset_scale_pass = 0) and in coset_scale_kernel (1); the inputs are read only"""
    _forward(O, shape, how, count, scale_pass)


_C17 = [(s, h) for s, h in SHAPES if s[0] in (5, 8) and s[2] == 8]


@pytest.mark.parametrize("scale_pass", [0, 1])
@pytest.mark.parametrize("shape,how", _C17, ids=[_ids(s) for s, _ in _C17])
def test_forward_transform_of_17_columns(gpu, O, shape, how, scale_pass):
    """17 columns on 8 cosets: two chunks of the scale pass (COSET_BATCH_MAX = 16), and 136 blocks on the folded path: more
    than one batched launch"""
    _forward(O, shape, how, 17, scale_pass)


def test_forward_transform_at_2_19(gpu, O):
    """k = 19: one column on 2 cosets; above k = 18 the scale pass and one transform per block run whatever the parameter says"""
    (shape, how), = [(s, h) for s, h in SHAPES if s[0] == 19]
    import torch
    k, ext, nc = shape
    dom, arg = _domain(shape, how)
    host = O.random_fr(24900, 1 << k)
    col = _dev(host)
    out, = dom.coeff_to_cosets_batch([col], arg)
    torch.cuda.synchronize()
    _assert_rows(out, cc.gather(O.coeff_to_extended(host, k, k + ext, cc.threads()), k, ext, nc), "column 0")
    _assert_rows(col, host, "the input was written")


# ============================================================================= d. the coset-major quotient kernels
NCOLS = 6


def _graphs():
    """a small gate program that is not the reference circuit's (q (a b(omega X) - c) folded into the previous value), and a
    lookup input expression of its own (a theta + c): the generic interpreter and the separate kernels run"""
    from circuits_halo2_amd import arithmetic as A
    gates = A.GraphEvaluator()
    prod = gates.add_calculation(A.MUL, gates.query(A.ADVICE, 0, 0), gates.query(A.ADVICE, 1, 1))
    gate = gates.add_calculation(A.MUL, gates.query(A.FIXED, 0, 0), gates.add_calculation(A.SUB, prod, gates.query(A.ADVICE, 2, 0)))
    gates.add_calculation(A.HORNER, (A.PREVIOUS_VALUE, 0, 0), (A.Y, 0, 0), [gate])
    inp = A.GraphEvaluator()
    comp = inp.add_calculation(A.ADD, inp.add_calculation(A.MUL, inp.query(A.ADVICE, 0, 0), (A.THETA, 0, 0)), inp.query(A.ADVICE, 2, -1))
    inp.add_calculation(A.STORE, comp)
    return gates, inp


class _Columns:
    """every input of the numerator drawn on the oracle's extended domain of 2^(k + ext) rows"""
    NAMES = ["fixed", "advice", "zs", "cols", "sigmas", "sel", "look", "start"]

    def __init__(self, O, k, ext, nsets, seed):
        rows = 1 << (k + ext)
        s = seed
        for name, cnt in zip(self.NAMES, [1, 3, nsets, NCOLS, NCOLS, 3, 5, 1]):
            setattr(self, name, [O.random_fr(s + i, rows) for i in range(cnt)])
            s += cnt

    def device(self, k, ext, nc):
        d = _Columns.__new__(_Columns)
        for name in self.NAMES:
            setattr(d, name, [_dev(cc.gather(c, k, ext, nc)) for c in getattr(self, name)])
        return d


def _quotient_case(O, shape, chunk_len, host, seed):
    """the separate coset kernels one after the other over a non-zero start, and the one entry point over garbage under
    quotient.fused_numerator = 0, against the oracle's three blocks on the extended domain, gathered"""
    import torch
    from circuits_halo2_amd import arithmetic as A
    k, ext, nc = shape
    ek = k + ext
    nsets = -(-NCOLS // chunk_len)
    gates, inp = _graphs()
    beta, gamma, theta, y = (O.random_fr(seed + i, 1) for i in range(4))
    none = np.zeros(0, dtype=np.uint8)
    l0, l_last, l_active = host.sel
    lz, pin, ptab, a_in, table = host.look

    def oracle_blocks(start, lookup_input):
        v = O.quotient_gates(start, gates.as_dict(), host.fixed, host.advice, [], none, beta, gamma, theta, y, k, ek)
        v = O.quotient_permutation(v, host.zs, host.cols, host.sigmas, chunk_len, l0, l_last, l_active, beta, gamma, y, k, ek, LAST_ROT)
        v = O.quotient_lookup(v, lz, pin, ptab, lookup_input, table, l0, l_last, l_active, beta, gamma, y, k, ek)
        return cc.gather(v, k, ext, nc)

    d = host.device(k, ext, nc)
    d_l0, d_ll, d_la = d.sel
    d_lz, d_pin, d_ptab, d_ain, d_table = d.look
    # 1. one kernel per block, values read and written in between
    values = d.start[0].clone()
    A.quotient_gates_cosets(values, gates, d.fixed, d.advice, [], none, beta, gamma, theta, y, k, nc)
    A.quotient_permutation_cosets(values, d.zs, d.cols, d.sigmas, chunk_len, d_l0, d_ll, d_la, beta, gamma, y, k, ek, nc, LAST_ROT)
    A.quotient_lookup_cosets(values, d_lz, d_pin, d_ptab, d_ain, d_table, d_l0, d_ll, d_la, beta, gamma, y, k, nc)
    torch.cuda.synchronize()
    _assert_rows(values, oracle_blocks(host.start[0], a_in), "gates, permutation, lookup one after the other")
    # 2. the one entry point: previous value zero, the lookup input from its own program, `values` full of garbage on entry
    zeros = np.zeros(32 << ek, dtype=np.uint8)
    want_input = O.quotient_gates(zeros, inp.as_dict(), host.fixed, host.advice, [], none, beta, gamma, theta, y, k, ek)
    values = _dev(O.random_fr(seed + 9, nc << k))
    try:
        _set("quotient.fused_numerator", 0)
        A.quotient_numerator_cosets(values, gates, inp, d.fixed, d.advice, [], none, d.zs, d.cols, d.sigmas, chunk_len, d_l0, d_ll, d_la,
                                    d_lz, d_pin, d_ptab, d_table, beta, gamma, theta, y, k, ek, nc, LAST_ROT)
        torch.cuda.synchronize()
    finally:
        _restore_defaults()
    _assert_rows(values, oracle_blocks(zeros, want_input), "sg_quotient_numerator_cosets_dev, separate kernels")


@pytest.mark.parametrize("chunk_len", [2, 4])
@pytest.mark.parametrize("shape", [(5, 1, 2), (5, 3, 8), (7, 2, 3), (7, 3, 7), (8, 4, 8), (9, 2, 4)], ids=_ids)
def test_coset_quotient_kernels_against_the_oracle(gpu, O, shape, chunk_len):
    """quot_perm_kernel, quot_lookup_kernel and the gate interpreter in coset mode on random data.  k = 5 and 7: a workgroup
    spans several blocks (every thread takes its own block's shift and power; 8 cosets at k = 5: one workgroup holds all of
    them); k = 8 and 9: a workgroup lies inside one block (shift and first power per workgroup).  6 permutation columns in
    chunks of 2 (3 sets) and 4 (2 sets, the last one short)"""
    k, ext, nc = shape
    host = _Columns(O, k, ext, -(-NCOLS // chunk_len), 25000 + 1000 * k + 100 * ext + 10 * nc + chunk_len)
    _quotient_case(O, shape, chunk_len, host, 26000 + 10 * k + nc)


def test_coset_quotient_kernels_at_extreme_words(gpu, O):
    """(7, 3, 7) with z, sigma and the selectors all zero, all the word r - 1 or all -1: the lazy-reduction bounds that random
    data rarely reaches, on the per-thread branch"""
    shape = k, ext, nc = (7, 3, 7)
    rows = 1 << (k + ext)
    host = _Columns(O, k, ext, 2, 27000)
    zero, top, m1 = np.zeros(32 * rows, dtype=np.uint8), cc.max_word(rows), cc.minus_one(rows)
    host.zs = [zero, top]
    host.sigmas = [zero, top, m1, host.sigmas[3], top, zero]
    host.sel = [top, m1, top]                               # l0, l_last, l_active
    host.look = [top, zero, top, host.look[3], m1]          # lookup z, permuted input, permuted table, input, table
    host.fixed = [top]
    host.advice = [top, host.advice[1], m1]
    host.cols = [top, zero, m1, *host.cols[3:]]
    _quotient_case(O, shape, 4, host, 27100)
