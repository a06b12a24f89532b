"""sg_lookup_permute_dev / sg_lookup_permute_async_dev / arithmetic.lookup_permute on the GPU, bit for bit against the rule that
tests/lookup_permute_cases.py states with Python integers (never against the host twin's general branch): row counts at the
workgroup (256) and sort tile (1024) edges and the smallest ones, full-width pools, keys that differ in one 32-bit word only,
equal columns, bijections, range tables (the same words as the range-table path), one-limb values that path refuses, every kind
of missing value, and the wait-free form call after call on one stream and on two."""
import ctypes as C

import numpy as np
import pytest

import lookup_permute_cases as lc

pytestmark = pytest.mark.gpu

SG_ERR_WITNESS = -6


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    import circuits_halo2_amd as sg
    from circuits_halo2_amd import ffi
    ffi.check(sg.lib().sg_init(0))
    yield sg
    torch.cuda.synchronize()


def _to_dev_mont(limbs):
    import torch
    from circuits_halo2_amd import arithmetic as A
    return A.fr_to_montgomery(torch.from_numpy(limbs.view(np.uint8).reshape(-1).copy()).cuda())


def _canon(t):
    from circuits_halo2_amd import arithmetic as A
    return A.fr_from_montgomery(t).cpu().numpy().view(np.uint64).reshape(-1, 4)


def _same(got, want, what):
    g = _canon(got)
    assert g.shape == want.shape, what
    bad = (g != want).any(axis=1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {len(bad)} rows differ, first at {int(np.argmax(bad))}"


def _run_blocking(spec):
    from circuits_halo2_amd import arithmetic as A
    inp, table, want = lc.case(*spec)
    got = A.lookup_permute(_to_dev_mont(inp), _to_dev_mont(table), len(inp))
    assert got is not None and want is not None
    _same(got[0], want[0], f"{lc.describe(spec)} A'")
    _same(got[1], want[1], f"{lc.describe(spec)} S'")
    return got


SMALL = [("wide", rows, d, 100 + rows) for rows in (1, 2, 7, 255, 256, 257, 1023, 1024, 1025) for d in sorted({3, rows})]
MIDDLE = [c for rows in (4090, 8186) for c in
          [("wide", rows, 17, 200 + rows), ("wide", rows, rows, 201 + rows), ("equal", rows), ("bijection", rows, 202 + rows)]
          + [("one_word", rows, w, 210 + rows + w) for w in range(8)]]


@pytest.mark.parametrize("spec", SMALL + MIDDLE + [("wide", lc.USABLE_17, 1 << 16, 300)], ids=lc.describe)
def test_blocking_form_is_the_rule(gpu, spec):
    _run_blocking(spec)


@pytest.mark.parametrize("rows", [7, 4090, lc.USABLE_17])
def test_range_tables_give_the_words_of_the_range_path(gpu, rows):
    from circuits_halo2_amd import arithmetic as A
    spec = ("range", rows, 400 + rows % 100)
    got = _run_blocking(spec)
    inp, table, _ = lc.case(*spec)
    small = A.lookup_permute_small(_to_dev_mont(inp), _to_dev_mont(table), rows)
    assert small is not None
    for g, s, name in zip(got, small, ("A'", "S'")):
        assert (g.cpu().numpy() == s.cpu().numpy()).all(), (rows, name)       # the Montgomery words themselves


def test_one_limb_values_the_range_path_refuses(gpu):
    from circuits_halo2_amd import arithmetic as A
    spec = ("word32", 4090, 500)
    inp, table, _ = lc.case(*spec)
    assert A.lookup_permute_small(_to_dev_mont(inp), _to_dev_mont(table), 4090) is None
    _run_blocking(spec)


def test_words_at_or_above_r_count_as_their_residue(gpu):
    """0 and 1 arrive as the words r and r + 1 in the input column: same A', S' as for the canonical words"""
    import torch
    from circuits_halo2_amd import arithmetic as A
    spec = ("wide", 257, 3, 101 + 256)
    inp, table, want = lc.case(*spec)
    d_inp = _to_dev_mont(inp).cpu().numpy().reshape(-1, 32).copy()
    ints = lc.to_ints(inp)
    for i, v in enumerate(ints):
        if v in (0, 1):                                  # Montgomery word of v is v * 2^256 mod r; + r keeps the residue
            word = int.from_bytes(d_inp[i].tobytes(), "little") + lc.R
            assert word < 1 << 256
            d_inp[i] = np.frombuffer(word.to_bytes(32, "little"), dtype=np.uint8)
    assert any(v in (0, 1) for v in ints)
    got = A.lookup_permute(torch.from_numpy(d_inp.reshape(-1)).cuda(), _to_dev_mont(table), 257)
    _same(got[0], want[0], "A'")
    _same(got[1], want[1], "S'")


@pytest.mark.parametrize("variant", lc.MISSING)
@pytest.mark.parametrize("rows", [7, 4090])
def test_missing_value_is_a_witness_error_and_the_next_call_is_right(gpu, rows, variant):
    import torch
    from circuits_halo2_amd import arithmetic as A, ffi
    inp, table, want = lc.case("missing", rows, variant, 600 + rows % 10)
    assert want is None
    d_inp, d_tab = _to_dev_mont(inp), _to_dev_mont(table)
    outs = [torch.empty(32 * rows, dtype=torch.uint8, device="cuda") for _ in range(2)]
    rc = ffi.lib().sg_lookup_permute_dev(ffi.dev_ptr(d_inp), ffi.dev_ptr(d_tab), C.c_size_t(rows), ffi.dev_ptr(outs[0]), ffi.dev_ptr(outs[1]),
                                         ffi.current_stream_ptr())
    assert rc == SG_ERR_WITNESS
    with pytest.raises(ValueError):
        A.lookup_permute(d_inp, d_tab, rows)
    _run_blocking(("wide", rows, 17, 200 + rows) if rows == 4090 else ("wide", 7, 3, 107))


def test_preconditions(gpu):
    import torch
    from circuits_halo2_amd import ffi
    L = ffi.lib()
    t = torch.zeros(64, dtype=torch.uint8, device="cuda")
    p, null, stream = ffi.dev_ptr(t), C.c_void_p(0), ffi.current_stream_ptr()
    assert L.sg_lookup_permute_dev(null, null, C.c_size_t(0), null, null, stream) == 0
    assert L.sg_lookup_permute_async_dev(null, null, C.c_size_t(0), null, null, p, stream) == 0
    for args in ((null, p, p, p), (p, null, p, p), (p, p, null, p), (p, p, p, null)):
        assert L.sg_lookup_permute_dev(args[0], args[1], C.c_size_t(2), args[2], args[3], stream) == -1      # SG_ERR_INVALID
        assert L.sg_lookup_permute_async_dev(args[0], args[1], C.c_size_t(2), args[2], args[3], p, stream) == -1
    assert L.sg_lookup_permute_async_dev(p, p, C.c_size_t(2), p, p, null, stream) == -1
    assert L.sg_lookup_permute_dev(p, p, C.c_size_t(1 << 31), p, p, stream) == -1
    assert L.sg_lookup_permute_async_dev(p, p, C.c_size_t(1 << 31), p, p, p, stream) == -1


# ---- the wait-free form: ten calls back to back, rows that shrink and grow, two rejected calls each followed by a valid one
def _plan(seed):
    rows = (lc.USABLE_17, 7, 4090, lc.USABLE_17, 4090, 4090, 8186, lc.USABLE_17, 7, 7)
    plan = []
    for i, n in enumerate(rows):
        if i in (4, 8):
            plan.append(("missing", n, lc.MISSING[(i + seed) % 5], seed + i))
        elif i % 2 == 0:
            plan.append(("wide", n, min(n, 1 << 16) if i % 4 == 0 else 17, seed + i))
        else:
            plan.append(("one_word", n, (i + seed) % 8, seed + i))
    return plan


def _prepare(plan):
    """inputs and outputs of every call on the device (outputs 0xA5 throughout, status words -1) -> calls, status"""
    import torch
    status = torch.full((len(plan),), -1, dtype=torch.int32, device="cuda")
    calls = []
    for spec in plan:
        inp, table, want = lc.case(*spec)
        outs = [torch.full((32 * len(inp),), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(2)]
        calls.append((spec, want, _to_dev_mont(inp), _to_dev_mont(table), outs))
    return calls, status


def _issue(calls, status, i, stream):
    from circuits_halo2_amd import ffi
    spec, _, d_inp, d_tab, outs = calls[i]
    ffi.check(ffi.lib().sg_lookup_permute_async_dev(ffi.dev_ptr(d_inp), ffi.dev_ptr(d_tab), C.c_size_t(spec[1]), ffi.dev_ptr(outs[0]),
                                                    ffi.dev_ptr(outs[1]), C.c_void_p(status.data_ptr() + 4 * i), C.c_void_p(stream.cuda_stream)))


def _check(calls, status):
    st = status.cpu().numpy()
    for i, (spec, want, _, _, outs) in enumerate(calls):
        assert st[i] == (1 if want is None else 0), (i, lc.describe(spec), st[i])
        if want is not None:
            _same(outs[0], want[0], f"call {i} {lc.describe(spec)} A'")
            _same(outs[1], want[1], f"call {i} {lc.describe(spec)} S'")
        else:
            assert (outs[0].cpu().numpy() == 0xA5).all() and (outs[1].cpu().numpy() == 0xA5).all(), i   # not written under status 1


def test_async_form_back_to_back_on_one_stream(gpu):
    import torch
    stream = torch.cuda.Stream()
    calls, status = _prepare(_plan(700))
    torch.cuda.synchronize()                             # inputs in place; from here on no wait until the end
    for i in range(len(calls)):
        _issue(calls, status, i, stream)
    torch.cuda.synchronize()
    _check(calls, status)


def test_async_form_on_two_streams(gpu):
    import torch
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    prepared = [_prepare(_plan(700)), _prepare(_plan(751))]
    torch.cuda.synchronize()
    for i in range(10):
        for (calls, status), stream in zip(prepared, streams):
            _issue(calls, status, i, stream)
    torch.cuda.synchronize()
    for calls, status in prepared:
        _check(calls, status)


def test_async_missing_value_leaves_status_1_and_the_next_call_is_right(gpu):
    import torch
    stream = torch.cuda.Stream()
    calls, status = _prepare([("missing", 4090, "top_word", 800), ("wide", 4090, 17, 200 + 4090)])
    torch.cuda.synchronize()
    for i in range(2):
        _issue(calls, status, i, stream)
    torch.cuda.synchronize()
    assert status.cpu().numpy().tolist() == [1, 0]
    _check(calls, status)
