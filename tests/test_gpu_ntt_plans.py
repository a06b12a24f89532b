"""The NTT engine under every plan, tile shape and pass variant its ten parameters reach, against the oracle.

tests/ntt_cases.py lists the (configuration, shape) cases; tests/test_ntt_cases_cpu.py asserts, without a GPU, that they reach every
variant of a pass (1, 2 and 3 passes; the transposing store of either multi-pass plan; every count of skipped stages and the
general zero-fill load of a zero-padded first pass; both kernels with odd and even stage counts; tiles wider and narrower than
the thread count, thread counts that are no multiple of 64; either way to the throughput shape; the scale in the twiddle table
and on the store; fold29 with and without post factors; pre factors; the table on the load; more than 32 vectors in one call).

Every expected word comes from the CPU oracle (best_fft, ifft / lagrange_to_coeff, coeff_to_extended, extended_to_coeff, and
the coset de-interleaving of test_gpu_round5_oracle.py); nothing here compares one library setting with another.  Each case
runs its transform on uniform random words and on the vectors uniform sampling never gives: all zero, a single non-zero element
at position 0 and at position n - 1, every element r - 1, the ramp r - 1 - i."""
import ctypes as C

import numpy as np
import pytest

import ntt_cases as nc
from conftest import fr_np

pytestmark = pytest.mark.gpu

CASES = nc.gpu_cases()
DEGREE = {1: 3, 2: 5, 3: 6}       # EvaluationDomain(j, k) with extended_k = k + ext
INPUTS = ("random", "zero", "first", "last", "max", "ramp")
BIG_INPUTS = ("random", "max")    # the one size above 2^14
_REF = {}


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    import circuits_halo2_amd as sg
    from circuits_halo2_amd import ffi
    ffi.check(sg.lib().sg_init(0))
    before = {name: ffi.get_param(name) for name in nc.DEFAULTS}
    yield sg
    assert {name: ffi.get_param(name) for name in nc.DEFAULTS} == before


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def _R():
    from oracle import pyref
    return pyref.R


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()      # (a copy: the shared inputs are read only)


def _host(t):
    return t.cpu().numpy()


def _input(O, name, log_n):
    """one input vector of 2^log_n Montgomery words (shared, read only)"""
    key = ("in", name, log_n)
    if key not in _REF:
        n, r = 1 << log_n, _R()
        if name == "random":
            v = O.random_fr(0x4E5454 + 131 * log_n, n)
        elif name == "zero":
            v = np.zeros(32 * n, dtype=np.uint8)
        elif name == "max":
            v = np.tile(fr_np([r - 1]), n)
        elif name == "ramp":
            v = fr_np([r - 1 - i for i in range(n)])
        else:
            v = np.zeros(32 * n, dtype=np.uint8)
            at = 0 if name == "first" else n - 1
            v[32 * at:32 * at + 32] = fr_np([0x1234567 + log_n])
        v.setflags(write=False)
        _REF[key] = v
    return _REF[key]


def _names(log_n):
    return INPUTS if log_n <= 14 else BIG_INPUTS


def _ref(O, kind, name, k, ext=0):
    """the oracle's answer for one (operation, input, size), computed once"""
    key = (kind, name, k, ext)
    if key not in _REF:
        T = min(8, O.ncpu())
        if kind == "fft":
            v = O.best_fft(_input(O, name, k), O.omega(k), k, T)
        elif kind == "fft_root":
            v = O.best_fft(_input(O, name, k), _root(k), k, T)
        elif kind == "ifft":
            v = O.ifft(_input(O, name, k), O.omega_inv(k), O.n_inv(k), k, T)
            assert (v == O.lagrange_to_coeff(_input(O, name, k), k, T)).all()
        elif kind == "c2e":
            v = O.coeff_to_extended(_input(O, name, k), k, k + ext, T)
        elif kind == "e2c":      # of an arbitrary extended vector, not only of the image of coeff_to_extended
            v = O.extended_to_coeff(_input(O, name, k + ext), k, k + ext, T)
        else:
            raise AssertionError(kind)
        v.setflags(write=False)
        _REF[key] = v
    return _REF[key]


def _root(k):
    """a primitive 2^k-th root of unity that is not the domain's generator"""
    from oracle import pyref
    return fr_np([pow(pyref.omega_for(k), 5, pyref.R)])


def _same(got, want, what):
    """bit for bit; on a mismatch say how many rows differ and where the first one is"""
    g = _host(got) if hasattr(got, "cpu") else got
    assert g.size == want.size, what
    bad = (g.reshape(-1, 32) != want.reshape(-1, 32)).any(axis=1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} rows differ, first at row {int(np.argmax(bad))}"


def _constant_closed_form(got, log_n, what):
    """the transform of the constant vector r - 1: n (r - 1) mod r at output 0, zero elsewhere -- stated directly"""
    g = _host(got) if hasattr(got, "cpu") else got
    n, r = 1 << log_n, _R()
    assert (g[:32] == fr_np([n * (r - 1) % r])).all() and not g[32:].any(), what


def _ptrs(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _run(gpu, O, case):
    """the case's operation on every input, under whatever parameters are in effect; returns [(what, got, want)] and checks
    the closed form and the untouched inputs on the way"""
    import torch
    from circuits_halo2_amd import ffi
    from circuits_halo2_amd.arithmetic import best_fft_batch
    L = ffi.lib()
    op, k, ext, count = case["op"], case["k"], case.get("ext", 0), case.get("count", 0)
    out = []
    if op in ("fft_dev", "fft_host", "fft_root"):
        for name in _names(k):
            a = _input(O, name, k)
            w = _root(k) if op == "fft_root" else O.omega(k)
            got = gpu.best_fft(a, w, k) if op == "fft_host" else gpu.best_fft(_dev(a), w, k)
            out.append((name, got, _ref(O, "fft_root" if op == "fft_root" else "fft", name, k)))
            if name == "max":
                torch.cuda.synchronize()
                _constant_closed_form(got, k, f"{case['name']}: constant vector")
    elif op == "intt_dev":
        for name in _names(k):
            d = _dev(_input(O, name, k))
            ffi.check(L.sg_intt_fr_dev(ffi.dev_ptr(d), ffi.ptr(O.omega_inv(k)), ffi.ptr(O.n_inv(k)), C.c_uint32(k), ffi.current_stream_ptr()))
            out.append((name, d, _ref(O, "ifft", name, k)))
    elif op == "l2c_dev":
        dom = gpu.EvaluationDomain(2, k)
        for name in _names(k):
            out.append((name, dom.lagrange_to_coeff(_dev(_input(O, name, k))), _ref(O, "ifft", name, k)))
    elif op in ("batch", "batch_oop"):
        names = [INPUTS[i % len(INPUTS)] for i in range(count)]
        inverse = case.get("divisor", False)
        w = O.omega_inv(k) if inverse else O.omega(k)
        vecs = [_dev(_input(O, name, k)) for name in names]
        if op == "batch":
            outs = best_fft_batch(vecs, w, k, O.n_inv(k) if inverse else None)
        else:
            outs = [torch.empty_like(v) for v in vecs]
            dv = ffi.ptr(O.n_inv(k)) if inverse else None
            ffi.check(L.sg_ntt_fr_batch_oop_dev(_ptrs(vecs), _ptrs(outs), C.c_size_t(count), ffi.ptr(w), dv, C.c_uint32(k),
                                                ffi.current_stream_ptr()))
            torch.cuda.synchronize()
            for name, v in zip(names, vecs):
                assert (_host(v) == _input(O, name, k)).all(), f"{case['name']}: input {name} changed"
        for i, (name, got) in enumerate(zip(names, outs)):
            out.append((f"vector {i} ({name})", got, _ref(O, "ifft" if inverse else "fft", name, k)))
            if name == "max" and not inverse:
                torch.cuda.synchronize()
                _constant_closed_form(got, k, f"{case['name']}: constant vector")
    elif op == "c2e":
        dom = gpu.EvaluationDomain(DEGREE[ext], k)
        assert dom.extended_k == k + ext
        for name in _names(k + ext):
            src = _dev(_input(O, name, k))
            out.append((name, dom.coeff_to_extended(src), _ref(O, "c2e", name, k, ext)))
            torch.cuda.synchronize()
            assert (_host(src) == _input(O, name, k)).all(), f"{case['name']}: input {name} changed"
    elif op == "c2e_batch":
        dom = gpu.EvaluationDomain(DEGREE[ext], k)
        names = [INPUTS[i % len(INPUTS)] for i in range(count)]
        srcs = [_dev(_input(O, name, k)) for name in names]
        outs = dom.coeff_to_extended_batch(srcs)
        torch.cuda.synchronize()
        for i, (name, src, got) in enumerate(zip(names, srcs, outs)):
            assert (_host(src) == _input(O, name, k)).all(), f"{case['name']}: input {name} changed"
            out.append((f"vector {i} ({name})", got, _ref(O, "c2e", name, k, ext)))
    elif op == "e2c":
        dom = gpu.EvaluationDomain(DEGREE[ext], k)
        keep = 32 * dom.n * dom.quotient_poly_degree
        for name in INPUTS:
            # an arbitrary extended vector (post factors on the last pass), then the round trip of a polynomial
            got = dom.extended_to_coeff(_dev(_input(O, name, k + ext)))
            out.append((f"{name}, extended_to_coeff", got, _ref(O, "e2c", name, k, ext)[:keep]))
            back = dom.extended_to_coeff(dom.coeff_to_extended(_dev(_input(O, name, k))))
            whole = np.concatenate([_input(O, name, k), np.zeros(keep - 32 * dom.n, dtype=np.uint8)])
            assert (O.extended_to_coeff(_ref(O, "c2e", name, k, ext), k, k + ext, 4)[:keep] == whole).all()
            out.append((f"{name}, round trip", back, whole))
    elif op == "cosets":
        from test_gpu_round5_oracle import _gather
        dom = gpu.EvaluationDomain(6, k)
        assert dom.extended_k == k + nc.COSET_EXT and dom.quotient_poly_degree == nc.COSETS
        names = [INPUTS[i % len(INPUTS)] for i in range(count)]
        srcs = [_dev(_input(O, name, k)) for name in names]
        outs = dom.coeff_to_cosets_batch(srcs)
        torch.cuda.synchronize()
        for i, (name, src, got) in enumerate(zip(names, srcs, outs)):
            assert (_host(src) == _input(O, name, k)).all(), f"{case['name']}: input {name} changed"
            key = ("cosets", name, k)
            if key not in _REF:
                _REF[key] = _gather(_ref(O, "c2e", name, k, nc.COSET_EXT), k)
            out.append((f"column {i} ({name})", got, _REF[key]))
    else:
        raise AssertionError(op)
    return out


def test_a_transform_of_one_element_is_that_element_times_the_scale(gpu):
    """log_n = 0 runs no pass at all: by the definition the element itself (sg_ntt_fr_dev), times the divisor (sg_intt_fr_dev, and
    every vector of sg_ntt_fr_batch_dev with a divisor)"""
    import torch
    from circuits_halo2_amd import ffi
    L, r = ffi.lib(), _R()
    one, d = fr_np([1]), 0x1234567
    xs = [r - 1, 0x89ABCDEF0123, 0]
    zero, stream = C.c_uint32(0), ffi.current_stream_ptr()
    plain, inverse, batch = [_dev(fr_np([x])) for x in xs], [_dev(fr_np([x])) for x in xs], [_dev(fr_np([x])) for x in xs]
    for a, b in zip(plain, inverse):
        ffi.check(L.sg_ntt_fr_dev(ffi.dev_ptr(a), ffi.ptr(one), zero, stream))
        ffi.check(L.sg_intt_fr_dev(ffi.dev_ptr(b), ffi.ptr(one), ffi.ptr(fr_np([d])), zero, stream))
    ffi.check(L.sg_ntt_fr_batch_dev(_ptrs(batch), C.c_size_t(len(batch)), ffi.ptr(one), ffi.ptr(fr_np([d])), zero, stream))
    torch.cuda.synchronize()
    for x, a, b, c in zip(xs, plain, inverse, batch):
        _same(a, fr_np([x]), f"sg_ntt_fr_dev, log_n = 0, x = {x:#x}")
        _same(b, fr_np([x * d % r]), f"sg_intt_fr_dev, log_n = 0, x = {x:#x}")
        _same(c, fr_np([x * d % r]), f"sg_ntt_fr_batch_dev, log_n = 0, x = {x:#x}")


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_ntt_case_against_the_oracle(gpu, O, case):
    import torch
    from circuits_halo2_amd import ffi
    with ffi.params(case["params"]):
        assert all(ffi.get_param(name) == value for name, value in case["params"].items()), "a parameter was clamped"
        try:
            results = _run(gpu, O, case)
        finally:
            torch.cuda.synchronize()
    for what, got, want in results:
        _same(got, want, f"{case['name']}: {what}")
