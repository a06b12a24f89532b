"""GPU tests of round 5's entry points against the oracle, at the shapes the product runs: the one-pass quotient numerator
(numerator_fused_kernel, and the separate kernels behind the same entry point), the coset transform with the shift folded
into the first NTT pass, the rotation sets' linear combinations in one launch, the wait-free lookup permutation and the
asynchronous Kate division batch; and the forward NTT at 2^22 on every output.

Every expected value comes from the CPU oracle (oracle/) or from the host reference the suite already trusts
(prover.permute_expression_pair); nothing here compares one HIP path with another.

The numerator's coset-major layout maps onto the oracle's extended domain as the header of sg_coeff_to_cosets_batch_dev
says: coset block b, row j <-> extended row b + 8 j (ext_k = k + 3, c_b = zeta omega_ext^b).  A rotation moves by a stride
of 8 in the extended domain and wraps inside its residue class, so the five classes b < 5 are the five coset blocks and
the three others (random fill) never mix with them."""
import ctypes as C
import threading

import numpy as np
import pytest

from conftest import fr_np

pytestmark = pytest.mark.gpu

# documented defaults of the parameters set here, restored by value (sg_get_param reports 0 for a per-lane one never set)
DEFAULTS = {"quotient.fused_numerator": 1, "ntt.radix4": 0, "ntt.coset_scale_pass": 0}
D = 5                        # quotient cosets of the reference circuit (degree 6: 2^(k + 3) extended rows, 5 blocks needed)
LAST_ROT = 6                 # blinding factors + 1
CHUNK = 4


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
    oracle.set_quotient_threads(_threads(oracle))
    yield oracle
    oracle.set_quotient_threads(1)


def _threads(O):
    return min(16, O.ncpu())


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


def _R():
    from oracle import pyref
    return pyref.R


def _max_word(n):
    """n copies of the word r - 1: the largest canonical Montgomery word"""
    return np.tile(np.frombuffer((_R() - 1).to_bytes(32, "little"), dtype=np.uint8), n)


def _minus_one(n):
    return np.tile(fr_np([_R() - 1]), n)


def _assert_rows(got, want, what=""):
    """bit for bit; on a mismatch say how many rows differ and where the first one is"""
    g = got.cpu().numpy() if hasattr(got, "cpu") else got
    assert g.size == want.size, what
    bad = (g.reshape(-1, 32) != want.reshape(-1, 32)).any(axis=1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} rows differ, first at row {int(np.argmax(bad))}"


# ============================================================================= 1. one-pass numerator against the oracle
def _gather(ext, k):
    """extended vector (2^(k + 3) rows) -> coset-major (5 blocks of 2^k rows): block b, row j = extended row b + 8 j"""
    n = 1 << k
    return np.ascontiguousarray(ext.reshape(n, 8, 32)[:, :D].transpose(1, 0, 2)).reshape(-1)


class _Inputs:
    """every input column of the numerator drawn on the extended domain (the oracle's layout); the device gets the coset-major
    gather of the same words"""
    NAMES = ["fixed", "advice", "inst", "zs", "sigmas", "sel", "look"]

    def __init__(self, O, k, seed):
        from circuits_halo2_amd import mst_inclusion as M
        self.k = k
        counts = [M.NUM_FIXED, M.NUM_ADVICE, 1, 2, 6, 3, 3]
        s = seed
        for name, cnt in zip(self.NAMES, counts):
            cols = []
            for _ in range(cnt):
                cols.append(O.random_fr(s, 8 << k))
                s += 1
            setattr(self, name, cols)

    def perm_cols(self):
        """the reference circuit's permutation columns (mst_inclusion.PERMUTATION_COLUMNS)"""
        return [self.fixed[2], self.advice[0], self.advice[1], self.fixed[3], self.advice[2], self.inst[0]]

    def device(self):
        d = _Inputs.__new__(_Inputs)
        d.k = self.k
        for name in self.NAMES:
            setattr(d, name, [_dev(_gather(c, self.k)) for c in getattr(self, name)])
        return d


_INPUTS = {}


def _inputs(O, k):
    """the extended inputs of size k, built once and shared across N_CURRENCIES (one size kept at a time)"""
    if k not in _INPUTS:
        _INPUTS.clear()
        host = _Inputs(O, k, 50000 + 1000 * k)
        _INPUTS[k] = (host, host.device())
    return _INPUTS[k]


def _oracle_numerator(O, h, nc, chal, beta, gamma, theta, y):
    """halo2's evaluate_h on the extended domain: gates (previous value zero), permutation, lookup; gathered to coset-major"""
    from circuits_halo2_amd import mst_inclusion as M
    k, ek = h.k, h.k + 3
    zeros = np.zeros(32 << ek, dtype=np.uint8)
    none = np.zeros(0, dtype=np.uint8)
    l0, l_last, l_active = h.sel
    v = O.quotient_gates(zeros, M.gate_graph(nc).as_dict(), h.fixed, h.advice, h.inst, chal, beta, gamma, theta, y, k, ek)
    v = O.quotient_permutation(v, h.zs, h.perm_cols(), h.sigmas, CHUNK, l0, l_last, l_active, beta, gamma, y, k, ek, LAST_ROT)
    a = O.quotient_gates(zeros, M.lookup_input_graph().as_dict(), h.fixed, h.advice, h.inst, none, beta, gamma, theta, y, k, ek)
    lz, pin, ptab = h.look
    v = O.quotient_lookup(v, lz, pin, ptab, a, h.fixed[4], l0, l_last, l_active, beta, gamma, y, k, ek)
    return _gather(v, k)


def _garbage(k, seed=4242):
    from oracle import oracle as O
    return _dev(O.random_fr(seed, D << k))


def _device_numerator(d, nc, chal, beta, gamma, theta, y, values=None):
    """sg_quotient_numerator_cosets_dev over `values` full of garbage (the entry point promises it needs no clearing)"""
    from circuits_halo2_amd import arithmetic as A, mst_inclusion as M
    k = d.k
    values = _garbage(k) if values is None else values
    l0, l_last, l_active = d.sel
    lz, pin, ptab = d.look
    A.quotient_numerator_cosets(values, M.gate_graph(nc), M.lookup_input_graph(), d.fixed, d.advice, d.inst, chal, d.zs, d.perm_cols(),
                                d.sigmas, CHUNK, l0, l_last, l_active, lz, pin, ptab, d.fixed[4], beta, gamma, theta, y, k, k + 3, D,
                                LAST_ROT)
    return values


def _challenges(nc, seed, real):
    """(challenges, beta, gamma, theta, y): the gate program's own challenges (powers of y) or random words of the same count"""
    from circuits_halo2_amd import mst_inclusion as M
    from oracle import oracle as O
    beta, gamma, theta = (O.random_fr(seed + i, 1) for i in range(3))
    y_int = int.from_bytes(O.random_fr(seed + 3, 1).tobytes(), "little") % _R()
    y = fr_np([y_int])
    n_chal = len(M.gate_challenge_exponents(nc))
    chal = np.ascontiguousarray(M.gate_challenges(y_int, nc)) if real else O.random_fr(seed + 4, n_chal)
    assert chal.size == 32 * n_chal
    return chal, beta, gamma, theta, y


_SHAPES = [(k, nc, real) for k in (5, 6, 8, 11) for nc in (1, 2, 3, 4) for real in (True, False)] + [(17, nc, True) for nc in (1, 2, 3, 4)]


@pytest.mark.parametrize("k,nc,real", _SHAPES)
def test_fused_numerator_against_the_oracle(gpu, O, k, nc, real):
    """every row of the one-pass numerator = the oracle's gates, permutation and lookup blocks on the extended domain.
    k = 5, 6: a workgroup spans several cosets (k = 6: the last workgroup is partial, 320 rows); k = 8: one coset per
    workgroup; k = 11: the reference's configuration; k = 17: the product's shape (2560 workgroups, a shift and omega-power
    per workgroup); real = the gate program's own challenges (powers of y), otherwise random words"""
    import torch
    host, d = _inputs(O, k)
    chal, beta, gamma, theta, y = _challenges(nc, 700 + 10 * nc + k, real)
    got = _device_numerator(d, nc, chal, beta, gamma, theta, y)
    torch.cuda.synchronize()
    _assert_rows(got, _oracle_numerator(O, host, nc, chal, beta, gamma, theta, y), f"k={k} nc={nc}")


def test_fused_numerator_refreshes_cached_constants(gpu, O):
    """the fused path caches the lowered programs and refreshes their constant tables per call: the same program with other
    beta, gamma, theta, y and challenges, and another program (nc = 4) between two calls of nc = 2, all issued before one
    wait -- each result equals its own oracle value"""
    import torch
    k = 8
    host, d = _inputs(O, k)
    calls = [(2, _challenges(2, 900, True)), (2, _challenges(2, 910, False)), (4, _challenges(4, 920, True)),
             (2, _challenges(2, 930, True))]
    outs = [_garbage(k, 4300 + i) for i in range(len(calls))]
    torch.cuda.synchronize()
    for (nc, args), values in zip(calls, outs):
        _device_numerator(d, nc, *args, values=values)
    torch.cuda.synchronize()
    for i, ((nc, args), got) in enumerate(zip(calls, outs)):
        _assert_rows(got, _oracle_numerator(O, host, nc, *args), f"call {i} nc={nc}")


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("nc", [2, 4])
def test_numerator_edge_rows_on_both_paths(gpu, O, nc, fused):
    """k = 11 with z, sigma, the selectors and some gate / lookup columns all zero, all the word r - 1 (the largest canonical
    word) or all -1: the lazy-reduction bounds random data rarely reaches; the one-pass kernel and the separate kernels
    (quotient.fused_numerator = 0) both equal the oracle"""
    import torch
    k = 11
    ne = 8 << k
    host = _Inputs(O, k, 61000 + nc)
    zero = np.zeros(32 * ne, dtype=np.uint8)
    top, m1 = _max_word(ne), _minus_one(ne)
    host.zs = [zero, top]
    host.sigmas = [zero, top, m1, host.sigmas[3], top, zero]
    host.sel = [top, m1, top]                               # l0, l_last, l_active
    host.look = [top, zero, top]                            # lookup z, permuted input, permuted table
    for j, c in {0: top, 4: m1, 5: top, 6: top, 7: zero, 8: top, 9: m1, 10: top}.items():
        host.fixed[j] = c
    host.advice = [top, host.advice[1], m1]
    d = host.device()
    chal, beta, gamma, theta, y = _challenges(nc, 950 + nc, True)
    try:
        _set("quotient.fused_numerator", fused)
        got = _device_numerator(d, nc, chal, beta, gamma, theta, y)
        torch.cuda.synchronize()
    finally:
        _restore_defaults()
    _assert_rows(got, _oracle_numerator(O, host, nc, chal, beta, gamma, theta, y), f"edges nc={nc} fused={fused}")


def test_separate_numerator_path_against_the_oracle(gpu, O):
    """quotient.fused_numerator = 0: the separate kernels behind the same entry point, random k = 11 case, = the oracle"""
    import torch
    k, nc = 11, 2
    host, d = _inputs(O, k)
    chal, beta, gamma, theta, y = _challenges(nc, 970, True)
    try:
        _set("quotient.fused_numerator", 0)
        got = _device_numerator(d, nc, chal, beta, gamma, theta, y)
        torch.cuda.synchronize()
    finally:
        _restore_defaults()
    _assert_rows(got, _oracle_numerator(O, host, nc, chal, beta, gamma, theta, y), "separate kernels")


# ============================================================================= 2. the same validation on both paths
_BAD_CALLS = ["last_rotation_2^k", "n_cosets_0", "n_cosets_9", "ext_k_equals_k", "null_advice_column", "null_permutation_column",
              "null_sigma", "null_z", "too_few_sets", "too_many_sets", "chunk_len_12"]


@pytest.mark.parametrize("case", _BAD_CALLS)
def test_numerator_refuses_the_same_calls_on_both_paths(gpu, O, case):
    """a bad call through sg_quotient_numerator_cosets_dev (the C ABI, not the Python wrapper's own checks) is refused with the
    same status under quotient.fused_numerator 1 and 0, and nothing is written; the valid call next to it still works"""
    import torch
    from circuits_halo2_amd import ffi, mst_inclusion as M
    k = 6
    host, d = _inputs(O, k)
    nc = 2
    chal, beta, gamma, theta, y = _challenges(nc, 990, True)
    g, keep = M.gate_graph(nc)._struct()
    gi, keep_i = M.lookup_input_graph()._struct()
    perm, sig, zs = d.perm_cols(), list(d.sigmas), list(d.zs)
    shape = dict(nsets=2, ncols=6, chunk_len=CHUNK, ext_k=k + 3, n_cosets=D, last_rot=LAST_ROT)
    advice = list(d.advice)
    if case == "last_rotation_2^k":
        shape["last_rot"] = 1 << k
    elif case == "n_cosets_0":
        shape["n_cosets"] = 0
    elif case == "n_cosets_9":
        shape["n_cosets"] = 9
    elif case == "ext_k_equals_k":
        shape["ext_k"] = k
    elif case == "null_advice_column":
        advice[1] = None
    elif case == "null_permutation_column":
        perm[4] = None
    elif case == "null_sigma":
        sig[5] = None
    elif case == "null_z":
        zs[1] = None
    elif case == "too_few_sets":
        shape["nsets"] = 1
    elif case == "too_many_sets":
        shape["nsets"] = 3
        zs.append(zs[0])
    elif case == "chunk_len_12":                            # one set of 12 columns: above what the permutation kernels take
        shape.update(nsets=1, ncols=12, chunk_len=12)
        perm, sig = perm * 2, sig * 2
    arr = lambda ts: (C.c_void_p * max(1, len(ts)))(*[t.data_ptr() if t is not None else None for t in ts])
    l0, l_last, l_active = d.sel
    lz, pin, ptab = d.look

    def call(values):
        return ffi.lib().sg_quotient_numerator_cosets_dev(
            ffi.dev_ptr(values), C.byref(g), C.byref(gi), arr(d.fixed), C.c_uint32(len(d.fixed)), arr(advice), C.c_uint32(len(advice)),
            arr(d.inst), C.c_uint32(1), ffi.ptr(chal), C.c_uint32(chal.size // 32), arr(zs), C.c_uint32(shape["nsets"]), arr(perm),
            arr(sig), C.c_uint32(shape["ncols"]), C.c_uint32(shape["chunk_len"]), ffi.dev_ptr(l0), ffi.dev_ptr(l_last),
            ffi.dev_ptr(l_active), ffi.dev_ptr(lz), ffi.dev_ptr(pin), ffi.dev_ptr(ptab), ffi.dev_ptr(d.fixed[4]), None,
            ffi.ptr(beta), ffi.ptr(gamma), ffi.ptr(theta), ffi.ptr(y), C.c_uint32(k), C.c_uint32(shape["ext_k"]),
            C.c_uint32(shape["n_cosets"]), C.c_uint32(shape["last_rot"]), ffi.current_stream_ptr())

    garbage = O.random_fr(4400, D << k)
    codes = {}
    try:
        for fused in (1, 0):
            _set("quotient.fused_numerator", fused)
            values = _dev(garbage)
            codes[fused] = call(values)
            torch.cuda.synchronize()
            assert (values.cpu().numpy() == garbage).all(), f"fused={fused}: a refused call wrote its output"
    finally:
        _restore_defaults()
    assert codes[1] == codes[0] != ffi.SG_OK, f"{case}: status {codes[1]} under the one-pass path, {codes[0]} under the separate kernels"
    got = _device_numerator(d, nc, chal, beta, gamma, theta, y)
    torch.cuda.synchronize()
    _assert_rows(got, _oracle_numerator(O, host, nc, chal, beta, gamma, theta, y), "valid call after a refused one")


# ============================================================================= 3. coset transform at the product's size
_COSET_WANT = {}


@pytest.mark.parametrize("radix4", [0, 1])
@pytest.mark.parametrize("k,count", [(17, 7), (17, 1), (11, 17)])
def test_coset_transform_against_the_oracle(gpu, O, k, count, radix4):
    """sg_coeff_to_cosets_batch_dev (shift folded into the first NTT pass) = the oracle's coeff_to_extended, de-interleaved to
    coset-major; 7 columns x 5 cosets = 35 blocks: more than one batched launch; ntt.radix4 = 1 as well; inputs unchanged"""
    import torch
    from circuits_halo2_amd.domain import EvaluationDomain
    n = 1 << k
    host = [O.random_fr(5200 + 37 * k + j, n) for j in range(count)]
    key = (k, count)
    if key not in _COSET_WANT:
        _COSET_WANT.clear()
        _COSET_WANT[key] = [_gather(O.coeff_to_extended(c, k, k + 3, _threads(O)), k) for c in host]
    dom = EvaluationDomain(6, k)
    assert dom.extended_k == k + 3 and dom.quotient_poly_degree == D
    cols = [_dev(c) for c in host]
    try:
        _set("ntt.radix4", radix4)
        outs = dom.coeff_to_cosets_batch(cols)
        torch.cuda.synchronize()
    finally:
        _restore_defaults()
    assert len(outs) == count
    for j, (got, want) in enumerate(zip(outs, _COSET_WANT[key])):
        _assert_rows(got, want, f"column {j}")
    for c, c0 in zip(cols, host):
        assert (c.cpu().numpy() == c0).all()                  # the inputs are read only


# ============================================================================= 4. rotation sets' combinations in one launch
def _lincomb_case(O, n, sizes, lows, seed, special=False):
    """-> sets for fr_lincomb_sets (device), and the oracle's outputs"""
    rng = np.random.default_rng(seed)
    pool = [O.random_fr(seed + 100 + j, n) for j in range(max(1, (sum(sizes) + 1) // 2))]
    sets, want = [], []
    for s, (m, nl) in enumerate(zip(sizes, lows)):
        idx = [int(rng.integers(len(pool))) for _ in range(m)]
        if m >= 3:
            idx[2] = idx[0]                                    # the same polynomial twice inside one set
        polys = [pool[i] for i in idx]
        coeffs = O.random_fr(seed + 10 * s, m) if m else np.zeros(0, dtype=np.uint8)
        if special and m >= 4:
            coeffs[0:32] = 0                                  # coefficient 0
            coeffs[32:64] = fr_np([_R() - 1])                 # -1
            coeffs[64:96] = _max_word(1)                      # the largest canonical word
        low = O.random_fr(seed + 10 * s + 5, nl) if nl else None
        out = O.fr_lincomb(polys, coeffs) if m else np.zeros(32 * n, dtype=np.uint8)
        for i in range(nl):
            out[32 * i:32 * i + 32] = O.fr_add(out[32 * i:32 * i + 32].copy(), low[32 * i:32 * i + 32].copy())
        sets.append(([_dev(p) for p in polys], coeffs, low))
        want.append(out)
    return sets, want


@pytest.mark.parametrize("name,n,sizes,lows", [
    ("prover", 1 << 17, [5, 25, 3, 2, 4], [2, 3, 4, 2, 3]),
    ("limits", 5000, [32, 0, 3, 3, 3, 3, 2, 2], [1, 4, 0, 2, 3, 4, 1, 0]),
    ("n=1", 1, [3, 1, 0], [1, 0, 1]),
    ("n=3", 3, [2, 5, 0], [3, 1, 2]),
    ("n=2^17+1", (1 << 17) + 1, [32, 1, 0, 4], [4, 0, 3, 2]),
])
def test_lincomb_sets_against_the_oracle(gpu, O, name, n, sizes, lows):
    """sg_fr_lincomb_sets_dev: each set = O.fr_lincomb plus its low coefficients (O.fr_add) on rows < n_low; the prover's five
    sets at 2^17 (one of 25 terms), 8 sets and 48 polynomials, a set of 32, an empty set (the low polynomial, zeros above it),
    odd lengths, coefficients 0, -1 and the word r - 1, a polynomial repeated inside a set"""
    import torch
    from circuits_halo2_amd import arithmetic as A
    sets, want = _lincomb_case(O, n, sizes, lows, 7000 + len(sizes) * 13 + n % 1000, special=True)
    outs = [torch.from_numpy(O.random_fr(7777 + i, n)).cuda() for i in range(len(sets))]    # garbage in the outputs
    A.fr_lincomb_sets(sets, n, outs)
    torch.cuda.synchronize()
    for s, (got, w) in enumerate(zip(outs, want)):
        _assert_rows(got, w, f"{name} set {s}")


# ============================================================================= 5. wait-free lookup permutation at k = 17
_USABLE_17 = (1 << 17) - 6


def _permute_case(rows, seed, kind="ok"):
    """(input, table) as (rows, 4) uint64 canonical limbs; the table holds every 16-bit value with repeats"""
    rng = np.random.default_rng(seed)
    table = np.zeros((rows, 4), dtype=np.uint64)
    table[:, 0] = (np.arange(rows, dtype=np.uint64) * 7919 + seed) % 65536
    inp = table[rng.integers(0, rows, rows)].copy()
    if rows > 100:
        inp[rng.integers(0, rows, rows // 3)] = table[rows // 2]           # long runs of one value
    if kind == "missing":                                                  # status 1: a 16-bit input value not in the table
        inp[rows // 3, 0] = np.setdiff1d(np.arange(65536, dtype=np.uint64), table[:, 0])[0]
    if kind == "wide":                                                     # status 2: a table value >= 2^16
        table[rows - 1, 0] = 70000
    return inp, table


def _to_dev_mont(limbs):
    import torch
    from circuits_halo2_amd import arithmetic as A
    return A.fr_to_montgomery(torch.from_numpy(limbs.view(np.uint8).reshape(-1).copy()).cuda())


def _prepare_permutations(plan):
    """inputs and outputs of every call of `plan` on the device (outputs full of garbage, status words -1); -> calls, status"""
    import torch
    status = torch.full((len(plan),), -1, dtype=torch.int32, device="cuda")
    calls = []
    for rows, seed, kind in plan:
        inp, table = _permute_case(rows, seed, kind)
        outs = [_dev(np.full(32 * rows, 0xA5, dtype=np.uint8)) for _ in range(2)]
        calls.append((kind, rows, inp, table, _to_dev_mont(inp), _to_dev_mont(table), outs))
    return calls, status


def _issue_permutation(calls, status, i, stream):
    """call i of a prepared plan on `stream`, no wait"""
    from circuits_halo2_amd import ffi
    kind, rows, inp, table, d_inp, d_tab, outs = calls[i]
    ffi.check(ffi.lib().sg_lookup_permute_small_async_dev(ffi.dev_ptr(d_inp), ffi.dev_ptr(d_tab), C.c_size_t(rows), ffi.dev_ptr(outs[0]),
                                                          ffi.dev_ptr(outs[1]), C.c_void_p(status.data_ptr() + 4 * i),
                                                          C.c_void_p(stream.cuda_stream)))


def _check_permutations(calls, status):
    from circuits_halo2_amd import arithmetic as A
    from circuits_halo2_amd.prover import permute_expression_pair
    st = status.cpu().numpy()
    canon = lambda t: A.fr_from_montgomery(t).cpu().numpy().view(np.uint64).reshape(-1, 4)
    for i, (kind, rows, inp, table, _, _, outs) in enumerate(calls):
        if kind == "missing":
            assert st[i] == 1, (i, kind, st[i])
        elif kind == "wide":
            assert st[i] == 2, (i, kind, st[i])
        else:
            assert st[i] == 0, (i, rows, st[i])
            want_a, want_s = permute_expression_pair(inp, table)
            assert (canon(outs[0]) == want_a).all(), (i, rows)
            assert (canon(outs[1]) == want_s).all(), (i, rows)


_PERMUTE_PLAN = [(_USABLE_17, 1, "ok"), (7, 2, "ok"), (4090, 3, "ok"), (_USABLE_17, 4, "ok"), (4090, 5, "missing"), (4090, 6, "ok"),
                 (_USABLE_17, 7, "wide"), (_USABLE_17, 8, "ok"), (7, 9, "missing"), (7, 10, "ok")]


def test_async_lookup_permutation_back_to_back(gpu):
    """sg_lookup_permute_small_async_dev, k = 17's usable rows and smaller, ten calls on one stream and then one wait: row counts
    that shrink and grow (the two work spaces alternate, each call cleans the other), calls rejected with status 1 and 2 each
    followed by a valid one; every output = prover.permute_expression_pair, every status word as expected"""
    import torch
    stream = torch.cuda.Stream()
    calls, status = _prepare_permutations(_PERMUTE_PLAN)
    torch.cuda.synchronize()                                  # inputs in place; from here on no wait until the end
    for i in range(len(calls)):
        _issue_permutation(calls, status, i, stream)
    torch.cuda.synchronize()
    _check_permutations(calls, status)


def test_async_lookup_permutation_on_two_streams(gpu):
    """the same kind of sequence on two streams, call by call interleaved (work spaces are per stream)"""
    import torch
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    plans = [_PERMUTE_PLAN, [(rows, seed + 50, kind) for rows, seed, kind in _PERMUTE_PLAN]]
    prepared = [_prepare_permutations(p) for p in plans]
    torch.cuda.synchronize()
    for i in range(len(_PERMUTE_PLAN)):
        for (calls, status), stream in zip(prepared, streams):
            _issue_permutation(calls, status, i, stream)
    torch.cuda.synchronize()
    for calls, status in prepared:
        _check_permutations(calls, status)


# ============================================================================= 6. Kate division batch under its ring
def _kate_sequence(O, seed, stream, n=1 << 17, m=11, calls=10):
    """`calls` > KATE_RING (4) batches issued back to back on `stream` with no host wait in between, each with its own
    polynomials and points; the host `points` buffer is overwritten as soon as a call returns (the header: read before
    return).  Inputs and outputs are in place before the first call.  -> [(polys, points, outs)]"""
    import torch
    from circuits_halo2_amd import ffi
    L = ffi.lib()
    prepared = []
    for c in range(calls):
        distinct = [O.random_fr(seed + 100 * c + j, n) for j in range(3)]
        polys = [distinct[j % 3] for j in range(m)]               # a polynomial divided by several points, as the multi-open does
        d_polys = [_dev(p) for p in distinct]
        outs = [_dev(np.full(32 * n, 0x5A, dtype=np.uint8)) for _ in range(m)]
        prepared.append((polys, O.random_fr(seed + 100 * c + 50, m), outs, d_polys))
    torch.cuda.synchronize()
    points = np.zeros(32 * m, dtype=np.uint8)
    for c, (_, pts, outs, d_polys) in enumerate(prepared):
        points[:] = pts
        pa = (C.c_void_p * m)(*[d_polys[j % 3].data_ptr() for j in range(m)])
        pq = (C.c_void_p * m)(*[o.data_ptr() for o in outs])
        ffi.check(L.sg_fr_kate_division_batch_dev(pa, C.c_size_t(n), ffi.ptr(points), C.c_uint32(m), pq, C.c_void_p(stream.cuda_stream)))
        points[:] = 0xEE                                          # the call has returned: its points may go
    return prepared


def _check_kate(O, issued, n=1 << 17):
    for c, (polys, pts, outs, _) in enumerate(issued):
        for j, (p, q) in enumerate(zip(polys, outs)):
            want_q, _ = O.fr_kate_division(p, pts[32 * j:32 * j + 32].copy())
            got = q.cpu().numpy()
            assert not got[32 * (n - 1):].any(), (c, j)
            _assert_rows(got[:32 * (n - 1)], want_q, f"call {c} division {j}")


def test_kate_division_batch_through_its_ring(gpu, O):
    """ten calls of sg_fr_kate_division_batch_dev (n = 2^17, m = 11: the prover's shape) back to back with no host wait in
    between -- the 4-slot page-locked ring of power tables is reused through its events -- then one wait: every quotient =
    O.fr_kate_division"""
    import torch
    stream = torch.cuda.Stream()
    issued = _kate_sequence(O, 8000, stream)
    torch.cuda.synchronize()
    _check_kate(O, issued)


def test_kate_division_batch_from_two_threads(gpu, O):
    """the same sequence from two host threads on two streams at once"""
    import torch
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    results, errors = [None, None], []

    def run(t):
        try:
            from circuits_halo2_amd import ffi
            ffi.check(ffi.lib().sg_init(0))
            results[t] = _kate_sequence(O, 8500 + 1000 * t, streams[t])
        except Exception as e:                                   # noqa: BLE001 -- reported below
            errors.append(e)

    threads = [threading.Thread(target=run, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    torch.cuda.synchronize()
    assert not errors, errors
    for issued in results:
        _check_kate(O, issued)


# ============================================================================= 7. NTT at 2^22, every output
_NTT22 = {}


@pytest.mark.parametrize("radix4", [0, 2])
def test_ntt_2_22_forward_against_the_oracle(gpu, O, radix4):
    """sg_ntt_fr_dev forward at 2^22 (a three-pass plan) = O.best_fft on every output, with two DIT stages per sweep (the
    default at this size) and without"""
    import torch
    k = 22
    a = O.random_fr(5300, 1 << k)
    if not _NTT22:
        _NTT22["want"] = O.best_fft(a, O.omega(k), k, _threads(O))
    d = _dev(a)
    try:
        _set("ntt.radix4", radix4)
        gpu.best_fft(d, O.omega(k), k)
        torch.cuda.synchronize()
    finally:
        _restore_defaults()
    _assert_rows(d, _NTT22["want"], f"radix4={radix4}")
