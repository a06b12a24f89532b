"""CPU checks of tests/poly_cases.py, the geometry, generators and case list behind tests/test_gpu_poly_edges.py: the restated
constants and rules are the ones csrc/poly_plan.h compiles to, the case list reaches every class of launch (each width of the Kate scan
exactly full and just entered, both instantiations of the batched evaluation, the first, last and refused block counts, every
zero pattern of the batch inversion), the generators and closed forms agree with the oracle at small sizes, and the oracle leaves
the inverse of a zero denominator at zero, as ff::BatchInvert does -- the GPU tests rely on that."""
import os
import subprocess

import numpy as np
import pytest

import poly_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "circuits_halo2_amd", "csrc")


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def test_restated_rules_are_the_compiled_ones(tmp_path):
    """tests/cpp/poly_plan_check.cpp runs the host geometry the launch functions and the C ABI use (csrc/poly_plan.h, no HIP);
    the restatement in poly_cases.py must print the same: every constant, and every rule at every size of the case lists, at
    the refused sizes, at n and n +- 1 for n = 2048 b, and around 2^24 and 2^26 for the evaluations.  The C++ rules are the
    reference: a difference is fixed in poly_cases.py."""
    from oracle import pyref
    exe = str(tmp_path / "poly_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "poly_plan_check.cpp"),
                           "-o", exe])
    sizes = {(n, 1) for n in pc.PREFIX_SIZES + pc.KATE_SIZES + pc.EVAL_SIZES + pc.EVAL_BATCH_TILED + pc.KATE_SMALL_SIZES + pc.KATE_BATCH_SMALL_SIZES}
    sizes |= {(n, 1) for n in (pc.PREFIX_REFUSED, pc.KATE_REFUSED, pc.EVAL_BATCH_REFUSED) + pc.PLAN_EVAL_EDGES}
    sizes |= set(pc.EVAL_BATCH_SHAPES) | {(pc.KD_BLOCK * b + d, m) for b in pc.PLAN_EDGE_BLOCKS for d in (-1, 0, 1) for m in (1, 3, pc.KATE_BATCH_MAX)}
    sizes |= {(1 << 26, 41), (4097, 80), (4097, 81)}
    sizes = sorted(sizes)
    prefixes = sorted({(n, c) for n, _ in sizes for c in (0, n, n + 1, n + 2)} | {((1 << 21) + 1, 0)})
    terms = list(range(0, 2 * pc.LINCOMB_MAX + 1))
    text = "".join(f"size {n} {m}\n" for n, m in sizes) + "".join(f"prefix {n} {c}\n" for n, c in prefixes) + "".join(f"lincomb {m}\n" for m in terms)
    got = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split("\n")[:-1]
    want = [pc.plan_constants()] + [pc.plan_line(n, m) for n, m in sizes]
    want += [f"prefix n={n} count_out={c} blocks={'none' if pc.prefix_blocks(n, c) is None else pc.prefix_blocks(n, c)}" for n, c in prefixes]
    want += [f"lincomb m={m} mid={','.join(map(str, pc.lincomb_mid_reductions(m))) or '-'}" for m in terms]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w
    # requests as arguments give the same answers
    by_args = subprocess.run([exe, "size 2049 16", "lincomb 32"], capture_output=True, text=True, check=True).stdout.split("\n")[:-1]
    assert by_args == [pc.plan_constants(), pc.plan_line(2049, 16), "lincomb m=32 mid=31"]
    assert pc.PP_BLOCK == pc.KD_BLOCK == 2048 and (pc.R, pc.MONT) == (pyref.R, pyref.MONT)
    # the kernels take the same rules: the scans are one workgroup of at most POLY_SCAN_MAX threads
    scan = open(os.path.join(CSRC, "poly_scan.cuh")).read()
    assert "__launch_bounds__(1024) prefix_product_scan_blocks_batch" in scan and "__launch_bounds__(1024) kate_scan_blocks" in scan


def test_geometry_at_the_edges():
    assert [pc.prefix_blocks(n, n + 1) for n in (0, 2047, 2048, (1 << 21) - 1, 1 << 21)] == [1, 1, 2, 1024, None]
    assert pc.prefix_blocks(1 << 21, 1 << 21) == 1024 and pc.prefix_blocks_before_the_fix(1 << 21, 1 << 21) is None
    assert pc.prefix_blocks((1 << 21) + 1, 0) is None and pc.grand_blocks(1 << 21) == 1024 and pc.grand_blocks((1 << 21) + 1) is None
    assert [pc.kate_scan_threads(b) for b in (2, 64, 65, 128, 129, 512, 513, 1024)] == [64, 64, 128, 128, 256, 512, 1024, 1024]
    assert pc.eval_levels(8192) == [8192] and pc.eval_levels(8193) == [8193, 2] and pc.eval_levels((1 << 21) + 1) == [(1 << 21) + 1, 257]
    assert pc.eval_levels((1 << 26) + 1) == [(1 << 26) + 1, 8193, 2]
    assert pc.eval_batch_plan(1 << 24, 2) == (16, 4096, [2]) and pc.eval_batch_plan((1 << 24) + 1, 2) == (32, 2049, [2])
    assert pc.eval_batch_plan(1 << 26, 41) == (32, 8192, [40, 1]) and pc.eval_batch_plan((1 << 26) + 1, 1) is None
    assert [pc.lincomb_mid_reductions(m) for m in (30, 31, 32)] == [[], [31], [31]]


def test_case_list_reaches_every_class():
    seen = pc.reached()
    assert pc.WANTED <= seen, sorted(pc.WANTED - seen)
    # what the issue names, literally
    assert set(pc.PREFIX_SIZES) == {0, 1, 7, 8, 9, 2047, 2048, 2049, 4096, (1 << 17) + 1, (1 << 21) - 1}
    assert set(pc.INVERT_SIZES) == {1, 7, 8, 9, 2047, 2048, 2049, (1 << 17) + 3}
    assert len(pc.KATE_SIZES) == 20 and all(pc.kate_blocks(n) in pc.KATE_BLOCK_COUNTS for n in pc.KATE_SIZES)
    assert set(pc.VECTOR_CLASSES) == {"random", "zero", "one", "max", "ramp", "first", "last"} and set(pc.SCALARS) == {"random", 0, 1, pc.R - 1}
    assert set(pc.PREFIX_CLASSES) == {"random", "one", "max", "first"} and set(pc.KATE_CLASSES) == {"random", "zero", "max", "last"}
    assert set(pc.EVAL_CLASSES) == {"random", "max", "last"} and set(pc.INVERT_VALUES) == {"random", "one", "max"}
    assert set(pc.LINCOMB_M) == {0, 1, 2, 3, 30, 31, 32} and set(pc.LINCOMB_N) == {1, 255, 256, 257}
    assert (21, (1,), 0) in [c[:3] for c in pc.GRAND_CASES] and (18, (2, 1), 1) in [c[:3] for c in pc.GRAND_CASES]
    assert (20, (1,), 1) in [c[:3] for c in pc.GRAND_CASES]


@pytest.mark.parametrize("n", [1, 7, 8, 9, 64, 2049])
def test_zero_patterns(n):
    for pat in pc.ZERO_PATTERNS:
        rows = pc.zero_rows(pat, n)
        assert rows == sorted(set(rows)) and all(0 <= r < n for r in rows), (pat, n)
    assert pc.zero_rows("all", n) == list(range(n)) and pc.zero_rows("tail", n) == [n - 1]
    if n >= 64:
        assert [r % 8 for r in pc.zero_rows("each position", n)] == list(range(8))


def test_fast_words_are_canonical():
    for seed in (1, 2, 3):
        w = pc.fast_words(seed, 1 << 14).reshape(-1, 32)
        top = w[:, ::-1].copy().view(">u8")[:, 0]            # the highest 64 bits of every word
        assert int(top.max()) < 1 << 61 and int(top.max()) >= 1 << 60      # below 2^253, and the bound is used
        assert max(int.from_bytes(bytes(x), "little") for x in w[:256]) < pc.R
    assert (pc.fast_words(7, 100) == pc.fast_words(7, 100)).all() and (pc.fast_words(7, 100) != pc.fast_words(8, 100)).any()


def test_generators(O):
    from conftest import fr_np
    n = 40
    assert (pc.mont([0, 1, 5, pc.R - 1]) == fr_np([0, 1, 5, pc.R - 1])).all()
    assert (pc.vector(O, "one", n, 0) == np.tile(fr_np([1]), n)).all() and not pc.vector(O, "zero", n, 0).any()
    mx = pc.vector(O, "max", n, 0)
    assert all(int.from_bytes(bytes(mx[32 * i:32 * i + 32]), "little") == pc.R - 1 for i in range(n))
    ramp = pc.vector(O, "ramp", n, 0)
    assert [int.from_bytes(bytes(ramp[32 * i:32 * i + 32]), "little") for i in range(n)] == [pc.R - 1 - i for i in range(n)]
    for name, at in (("first", 0), ("last", n - 1)):
        v = pc.vector(O, name, n, 3).reshape(n, 32)
        assert [i for i in range(n) if v[i].any()] == [at] and pc.value_of(v[at]) == pc.single_value(3)
    assert (pc.vector(O, "random", n, 9) == O.random_fr(9, n)).all()
    assert (pc.vector(O, "random", pc.FAST_ABOVE + 1, 9) == pc.fast_words(9, pc.FAST_ABOVE + 1)).all()
    assert [pc.value_of(pc.scalar(O, s, 0)) for s in (0, 1, pc.R - 1)] == [0, 1, pc.R - 1]
    nc = pc.noncanonical_words(5, 10)
    ints = [int.from_bytes(bytes(nc[32 * i:32 * i + 32]), "little") for i in range(10)]
    assert ints[:3] == [pc.R, pc.R + 1, (1 << 256) - 1] and ints[-1] == (1 << 256) - 1 and sum(v >= pc.R for v in ints) >= 5
    red = pc.reduced(nc)
    assert [int.from_bytes(bytes(red[32 * i:32 * i + 32]), "little") for i in range(10)] == [v % pc.R for v in ints]


@pytest.mark.parametrize("x", pc.SCALARS)
@pytest.mark.parametrize("n", [1, 2, 9, 300])
def test_closed_forms_agree_with_the_oracle(O, n, x):
    pt = pc.scalar(O, x, 77)
    xv = pc.value_of(pt)
    v = pc.vector(O, "last", n, n)
    c = pc.single_value(n)
    assert (O.fr_eval_poly(v, pt) == pc.mont([pc.eval_of_last(c, xv, n)])).all()
    q, rem = O.fr_kate_division(v, pt)
    assert (q == pc.mont([pc.kate_of_last(c, xv, n, i) for i in range(n - 1)])).all() if n > 1 else q.size == 0
    assert (rem == pc.mont([pc.kate_of_last(c, xv, n, -1)])).all()
    # a tiled polynomial: period L, n coefficients
    L = 7
    period = O.random_fr(500 + n, L)
    tiled = np.tile(period, n // L + 1)[:32 * n]
    if pow(xv, L, pc.R) != 1:
        full, tail = pc.value_of(O.fr_eval_poly(period, pt)), pc.value_of(O.fr_eval_poly(period[:32 * (n % L)].copy(), pt)) if n % L else 0
        assert (O.fr_eval_poly(tiled, pt) == pc.mont([pc.eval_of_tiled(full, tail, xv, L, n)])).all()


def _values(words):
    return [pc.value_of(words[i:i + 32]) for i in range(0, len(words), 32)]


@pytest.mark.parametrize("n", [1, 8, 9, 64])
def test_oracle_leaves_the_inverse_of_zero_at_zero(O, n):
    """fr_batch_invert, permutation_product and lookup_product against Python integers, with zero denominators among the rows"""
    from oracle import pyref
    inv = lambda v: pow(v, -1, pc.R) if v else 0
    for pat in pc.ZERO_PATTERNS:
        a = O.random_fr(900 + n, n)
        for r in pc.zero_rows(pat, n):
            a[32 * r:32 * r + 32] = 0
        assert _values(O.fr_batch_invert(a)) == [inv(v) for v in _values(a)], pat
    if n & (n - 1) or n < 2:
        return
    k = n.bit_length() - 1
    beta, gamma = O.random_fr(31, 1), O.random_fr(32, 1)
    bv, gv = pc.value_of(beta), pc.value_of(gamma)
    vals, sig = O.random_fr(33, n), O.random_fr(34, n)
    rows = pc.vanishing_rows(n)
    for r in rows:                       # v = -(beta sigma + gamma): the denominator of row r vanishes
        vals[32 * r:32 * r + 32] = pc.mont([-(bv * pc.value_of(sig[32 * r:32 * r + 32]) + gv)])
    v_, s_, w = _values(vals), _values(sig), pyref.omega_for(k)
    z, want = 1, []
    for i in range(n):
        want.append(z)
        z = z * (pow(w, i, pc.R) * bv + gv + v_[i]) * inv((bv * s_[i] + gv + v_[i]) % pc.R) % pc.R
    assert not all(want) and _values(O.permutation_product([vals], [sig], beta, gamma, pc.mont([1]), k)) == want
    a, s, ap, sp = (O.random_fr(40 + i, n) for i in range(4))
    for r in rows:                       # a' = -beta
        ap[32 * r:32 * r + 32] = pc.mont([-bv])
    av, sv, apv, spv = map(_values, (a, s, ap, sp))
    z, want = 1, []
    for i in range(n):
        want.append(z)
        z = z * (av[i] + bv) * (sv[i] + gv) * inv((apv[i] + bv) * (spv[i] + gv) % pc.R) % pc.R
    assert not all(want) and _values(O.lookup_product(a, s, ap, sp, beta, gamma)) == want
