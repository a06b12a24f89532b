"""CPU checks of tests/g1_cases.py, the geometry, generators and case lists behind tests/test_gpu_g1_ops.py: the restated constants
are the ones csrc/g1_ops.hip holds, the oracle is a fit reference for every class of input the GPU tests use (it agrees with
oracle/pyref.py's affine group law, dft_naive and msm_naive on identities, repeated and opposite points at small sizes), and the
case lists reach what they are meant to reach: every shape of the scan's level list, and -- derived from the scalars alone --
the doubling, cancelling and identity operand pairs of the FFT at the stages claimed and of the scan in the kernels claimed."""
import os
import re

import numpy as np
import pytest

import g1_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "circuits_halo2_amd", "csrc")
R = gc.R


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def P():
    from oracle import pyref
    return pyref


def _pt(P, xy):
    return np.frombuffer(P.g1_to_bytes(xy), dtype=np.uint8)


G = (1, 2)


# ----------------------------------------------------------------------------- constants and geometry
def test_restated_constants_are_the_ones_in_the_source(P):
    src = open(os.path.join(CSRC, "g1_ops.hip")).read()
    assert f"static constexpr uint32_t PFX_CHUNK = {gc.PFX_CHUNK};" in src
    bounds = {name: int(v) for v, name in re.findall(r"__launch_bounds__\((\d+)\)\s+(\w+)\(", src)}
    assert bounds["g1_fixed_base_mul"] == bounds["g1_on_curve_kernel"] == gc.BLOCK_256
    for name in ("g1fft_stage", "g1fft_store", "g1_prefix_chunks", "g1_prefix_apply", "g1_prefix_store", "msm_table_step"):
        assert bounds[name] == gc.BLOCK_128, name
    assert "(n + 255) / 256), 256, 0, stream>>>(d_scalars" in src and "(n + 255) / 256), 256, 0, stream>>>(d_points" in src
    assert (gc.R, gc.Q, gc.MONT, gc.ROOT_OF_UNITY) == (P.R, P.Q, P.MONT, P.ROOT_OF_UNITY)
    assert all(gc.omega(k) == P.omega_for(k) for k in range(0, 17))
    plan = open(os.path.join(CSRC, "msm_plan.h")).read()
    assert "W1 = wp.W = (255 + c - 1) / c" in plan and "std::min<uint32_t>(16, std::max<uint32_t>(4, lg))" in plan
    assert [gc.default_window_bits(1 << k) for k in (1, 5, 11, 16, 20)] == [4, 5, 11, 16, 16]


def test_prefix_levels_cover_every_shape():
    for k, levels in gc.PREFIX_KS.items():
        assert gc.prefix_levels(1 << k) == levels
    counts = [len(v) for v in gc.PREFIX_KS.values()]
    assert sorted(set(counts)) == [1, 2, 3, 4]
    assert gc.PREFIX_KS[4] == [16] and gc.PREFIX_KS[5] == [gc.PFX_CHUNK]              # less than a chunk, exactly one
    assert gc.PREFIX_KS[10][1] == gc.PFX_CHUNK                                        # the totals fill one chunk exactly
    assert gc.prefix_levels(33) == [33, 2] and gc.prefix_levels(1025) == [1025, 33, 2]
    assert gc.prefix_probe_rows(16) == [0, 15] and gc.prefix_probe_rows(64) == [0, 31, 32, 33, 63]
    assert gc.prefix_probe_rows(2048) == [0, 31, 32, 33, 1023, 1024, 1025, 2047]


# ----------------------------------------------------------------------------- 1: fixed-base products
def test_fixed_base_vectors_hold_every_edge_at_a_block_end():
    edges = gc.fixed_base_edges()
    values = [v for _, v in edges]
    assert len(edges) == 7 + 254 + 7 and len(set(values)) == len(values) - 2          # 2^0 = 1 and 2^1 = 2 appear twice
    assert {1 << b for b in range(254)} <= set(values) and max(values) < R and (1 << 253) < R < (1 << 254)
    assert gc.FIXED_BASE_SIZES == (1, gc.BLOCK_256 - 1, gc.BLOCK_256, gc.BLOCK_256 + 1, 2 * gc.BLOCK_256 + 1)
    for n in gc.FIXED_BASE_SIZES:
        vecs = gc.fixed_base_vectors(n)
        assert all(len(v) == n and v[-1] in values for v in vecs)
        assert (set(values) if n > 1 else set(gc.FIXED_BASE_EDGES_ALONE)) <= {x for v in vecs for x in v}
    assert set(gc.FIXED_BASE_EDGES_ALONE) <= set(values) and set(values[:7]) <= set(gc.FIXED_BASE_EDGES_ALONE)
    u = gc.fixed_base_unreduced_values()
    assert len(u) == 257 and {0, 1, R - 1, 1 << 253} <= set(u)
    words = gc.unreduced(u).reshape(-1, 32)
    for v, w in zip(u, words):
        w = int.from_bytes(bytes(w), "little")
        assert R <= w < gc.MONT and w % R == v * gc.MONT % R


def test_oracle_fixed_base_mul_on_the_edges(O, P):
    """0, r - 1, every 2^b and the other edge scalars against pyref's double-and-add; 0 gives 64 zero bytes, r - 1 gives -G"""
    values = [v for _, v in gc.fixed_base_edges()]
    got = O.fixed_base_mul(gc.mont(values), 2).reshape(-1, 64)
    for v, g in zip(values, got):
        assert (g == _pt(P, P.g1_mul(G, v))).all(), v
    assert not got[0].any() and (got[3] == _pt(P, (1, gc.Q - 2))).all()
    assert (got[5] != got[6]).any() and not O.g1_add(got[5], got[6]).any()           # (r-1)/2 + (r+1)/2 = r
    assert (O.g1_add(got[5], got[5]) == got[3]).all()                                # 2 * (r-1)/2 = r - 1
    assert (gc.mont(values) == np.frombuffer(P.frs_to_bytes(values), dtype=np.uint8)).all()


# ----------------------------------------------------------------------------- 2: FFT over G1
def test_oracle_best_fft_at_the_smallest_sizes_and_the_trace(O, P):
    """O.best_fft at log_n = 0 and 1 and on every small case against dft_naive; fft_trace -- the butterflies in g1fft_stage's
    order -- gives the same transform, so its operand classes are those of the kernel"""
    for log_n in (0, 1, 2, 3, 5):
        for root in gc.FFT_ROOTS:
            w = gc.fft_root(root, log_n)
            for pattern in gc.FFT_PATTERNS:
                s = gc.fft_scalars(pattern, log_n, root)
                want = P.dft_naive(s, w)
                assert P.frs_from_bytes(O.best_fft(gc.mont(s), gc.mont([w]), log_n).tobytes()) == want, (log_n, root, pattern)
                assert gc.fft_trace(s, w, log_n)[0] == want
    s = gc.fft_scalars("random", 0)
    assert P.frs_from_bytes(O.best_fft(gc.mont(s), gc.mont([1]), 0).tobytes()) == s
    s = gc.fft_scalars("random", 1)
    assert P.frs_from_bytes(O.best_fft(gc.mont(s), gc.mont([R - 1]), 1).tobytes()) == [(s[0] + s[1]) % R, (s[0] - s[1]) % R]
    for log_n in (8,):
        for root in gc.FFT_ROOTS:
            w = gc.fft_root(root, log_n)
            s = gc.fft_scalars("late_equal", log_n, root)
            assert P.frs_from_bytes(O.best_fft(gc.mont(s), gc.mont([w]), log_n).tobytes()) == gc.fft_trace(s, w, log_n)[0]


def test_fft_cases_reach_the_claimed_operand_pairs():
    cases = gc.fft_cases()
    assert len(cases) == len(set(cases)) == len(gc.FFT_LOGS) * 2 * (4 * 2 + 2 * (len(gc.FFT_PATTERNS) - 2))
    for log_n in gc.FFT_LOGS:
        here = [c[1:] for c in cases if c[0] == log_n]
        assert {(r, p) for r, _, p in here} == {(r, p) for r in gc.FFT_ROOTS for p in gc.FFT_PATTERNS}
        assert {(r, sc) for r, sc, p in here if p == "random"} == {(r, sc) for r in gc.FFT_ROOTS for sc in gc.FFT_SCALES}
        assert all(("omega_inv", "n_inv", p) in here and ("omega", "none", p) in here for p in gc.FFT_PATTERNS)
    assert gc.FFT_LOGS == (0, 1, 2, 3, 5, 8) and (1 << 8) // 2 == 2 * 64 and (1 << 8) // 2 > gc.BLOCK_128 - 1
    assert {c[2] for c in cases} == {"none", "n_inv", "one", "zero"} and gc.fft_scale("none", 3) is None
    for log_n in gc.FFT_LOGS:
        assert gc.fft_root("omega", log_n) * gc.fft_root("omega_inv", log_n) % R == 1
        assert gc.fft_scale("n_inv", log_n) * (1 << log_n) % R == 1
        for root in gc.FFT_ROOTS:
            w = gc.fft_root(root, log_n)
            for pattern in gc.FFT_PATTERNS:
                _, seen = gc.fft_trace(gc.fft_scalars(pattern, log_n, root), w, log_n)
                for claim in gc.fft_claims(pattern, log_n):
                    assert claim in seen, (log_n, root, pattern, claim)
            _, seen = gc.fft_trace(gc.fft_scalars("random", log_n, root), w, log_n)
            assert {kind for _, kind, _ in seen} <= {"generic"}                       # uniform inputs never get there
    # between them the patterns meet every class at stage 0 and at a later, twiddled stage
    claims = {c for p in gc.FFT_PATTERNS for c in gc.fft_claims(p, 8)}
    assert {(0, "double", False), (0, "cancel", False), (0, "b_identity", False), (1, "double", True), (7, "cancel", False),
            (7, "a_identity", True), (1, "b_identity", True)} <= claims


def test_oracle_group_law_on_identities_repeats_and_opposites(O, P):
    """O.g1_add / O.g1_mul / O.best_multiexp against pyref's affine law and msm_naive over bases that hold identities, the same
    point twice and P beside -P -- including scalars that make the whole sum cancel"""
    a, b = gc.randoms(21, 2)
    pa, pb = P.g1_mul(G, a), P.g1_mul(G, b)
    for x, y in [(pa, pb), (pa, pa), (pa, P.g1_neg(pa)), (None, pa), (pa, None), (None, None)]:
        assert (O.g1_add(_pt(P, x), _pt(P, y)) == _pt(P, P.g1_add(x, y))).all()
    for k in (0, 1, 2, R - 1, a):
        assert (O.g1_mul(_pt(P, pa), gc.mont([k])) == _pt(P, P.g1_mul(pa, k))).all()
        assert (O.g1_mul(_pt(P, None), gc.mont([k])) == 0).all()
    for n in (1, 2, 7, 33):
        t = gc.randoms(22 + n, n)
        for i in range(n):
            t[i] = 0 if i % 5 == 2 else t[0] if i % 5 == 4 else R - t[0] if i % 5 == 3 else t[i]
        pts = [P.g1_mul(G, v) for v in t]
        bases = np.concatenate([_pt(P, p) for p in pts])
        assert (bases == O.fixed_base_mul(gc.mont(t))).all()
        for sc in (gc.randoms(23 + n, n, nonzero=False), [1] * n, [R - 1] * n, [0] * n, [1 if i % 5 in (0, 3) and i < 5 else 0 for i in range(n)]):
            want = P.msm_naive(sc, pts)
            assert (O.best_multiexp(gc.mont(sc), bases) == _pt(P, want)).all(), (n, sc[:3])
            dot = sum(x * y for x, y in zip(sc, t)) % R
            assert (O.fixed_base_mul(O.fr_dot(gc.mont(sc), gc.mont(t))) == _pt(P, want)).all()
            assert P.fr_from_bytes(O.fr_dot(gc.mont(sc), gc.mont(t)).tobytes()) == dot
    assert P.frs_from_bytes(O.fr_mul_n(gc.mont([a, 0, R - 1]), gc.mont([b, b, R - 1])).tobytes()) == [a * b % R, 0, 1]


# ----------------------------------------------------------------------------- 3: prefix sums and window tables
def test_prefix_cases_reach_the_claimed_branches(O, P):
    assert gc.PREFIX_PATTERNS == ("random", "equal", "alternating", "zeros", "cancel32")
    for k in gc.PREFIX_KS:
        for pattern in gc.PREFIX_PATTERNS:
            s = gc.prefix_scalars(pattern, k)
            q, seen = gc.prefix_trace(s)
            assert q == gc.running_sums(s), (k, pattern)                             # the blocked scan is a scan
            for claim in gc.prefix_claims(pattern, k):
                assert claim in seen, (k, pattern, claim)
            if pattern == "random":
                assert {kind for _, kind in seen} <= {"generic", "a_identity"}         # (every chunk starts from the identity)
            if pattern == "cancel32" and k >= 6:
                assert q[32] == 0 and q[31] and q[33]
            if pattern == "alternating":
                assert not any(q[1::2]) and all(q[0::2])
    claims = {c for p in gc.PREFIX_PATTERNS for c in gc.prefix_claims(p, 16)}
    assert {("chunks0", "double"), ("chunks1", "double"), ("apply", "double"), ("store", "double"), ("chunks0", "cancel"),
            ("store", "cancel"), ("chunks0", "b_identity"), ("chunks1", "b_identity")} <= claims
    # the step column's difference-form commitment is Q_j: sum_i (c_i - c_(i+1)) Q_i with c_n = 0
    n, s = 16, gc.prefix_scalars("random", 4)
    q = gc.running_sums(s)
    for j in gc.prefix_probe_rows(n):
        col = P.frs_from_bytes(gc.step_column(j, n).tobytes())
        assert col == [1] * (j + 1) + [0] * (n - j - 1)
        assert sum((col[i] - (col[i + 1] if i + 1 < n else 0)) * q[i] for i in range(n)) % R == q[j]
        assert sum(c * v for c, v in zip(col, s)) % R == q[j]
    pw = gc.piecewise_values(2048)
    assert len(pw) == 2048 and len(set(pw)) < 2048 // 8 and 0 in pw


def test_window_table_cases_read_every_row():
    assert gc.TABLE_KS == (5, 11) and gc.TABLE_WINDOW_BITS == (4, 7, 13, 16, 0)
    for c in range(4, 17):
        width = gc.window_widths(c)
        assert len(width) == (255 + c - 1) // c and sum(width) == 254 and min(width) >= c - 2
        rows = {gc.table_row_of_bit(c, b) for b in gc.TABLE_BITS}
        assert rows == set(range(len(width)))                                       # the single-bit columns read every row of the table
    assert gc.window_widths(4)[-3:] == [4, 3, 3] and len(gc.window_widths(4)) == 64 and len(gc.window_widths(16)) == 16
    for k in gc.TABLE_KS:
        n = 1 << k
        t = gc.table_basis_scalars(k, 0)
        assert t.count(0) >= n // 6 and t.count(t[1]) >= n // 6 and (R - t[1]) in t
        assert len(set(gc.table_basis_scalars(k, 1))) == n
        rows = [gc.table_bit_row(b, n) for b in gc.TABLE_BITS]
        assert any(t[r] == 0 for r in rows) and any(t[r] == t[1] for r in rows) and len(set(rows)) >= min(n, 254) // 2


# ----------------------------------------------------------------------------- 4: on-curve check
def test_curve_cases(O, P):
    """every spoiled point is off the curve by pyref -- or, for the unreduced twins, ON the curve as a residue and not below q as
    a word, which is what halo2curves' from_raw_bytes refuses; the good bases hold identities and P beside -P"""
    cases = gc.curve_cases()
    assert {k for _, k, _ in cases} == set(gc.CURVE_KS) == {1, 8, 9} and (1 << 8) == gc.BLOCK_256
    assert max(len(sp) for _, _, sp in cases) == 300
    for k in gc.CURVE_KS:
        n = 1 << k
        assert {(b, i) for _, kk, sp in cases if kk == k and len(sp) == 1 for b, i, _ in sp} == {(b, i) for b in (0, 1) for i in {0, min(255, n - 1), n - 1}}
        assert {h for _, kk, sp in cases if kk == k for _, _, h in sp} == set(gc.SPOILS)
    s = gc.curve_scalars(8)[0]
    assert s.count(0) >= 28 and (s[6] + s[7]) % R == 0
    pts = O.fixed_base_mul(gc.mont(s), 2).reshape(-1, 64)
    assert all(O.g1_is_on_curve(p) for p in pts)
    assert (pts[6][:32] == pts[7][:32]).all() and (pts[6][32:] != pts[7][32:]).any()
    for idx in (0, 6, 7, 255):
        good = P.g1_from_bytes(bytes(pts[idx]))
        assert good is not None and P.g1_is_on_curve(good)
        for how in gc.SPOILS:
            bad = gc.spoil(pts[idx], how)
            x, y = gc.fq_words(bad[:32]), gc.fq_words(bad[32:])
            residue = P.g1_from_bytes(bytes(gc.raw_words([x % gc.Q, y % gc.Q])))
            if how in ("x+q", "y+q"):
                assert residue == good and max(x, y) >= gc.Q and max(x, y) < gc.MONT
            else:
                assert max(x, y) < gc.Q and not P.g1_is_on_curve(residue) and not O.g1_is_on_curve(bad)


# ----------------------------------------------------------------------------- 5: KZG set-up
def test_setup_cases(O, P):
    """lagrange_at is the Lagrange basis (it interpolates every monomial) and has L_j(omega^j) = 1; every k holds a tau inside the
    domain, where the closed form with 1 / 0 = 0 differs from it in exactly that row"""
    assert gc.SETUP_KS == (0, 1, 5, 8)
    for k in gc.SETUP_KS:
        n, w = 1 << k, gc.omega(k)
        taus = dict(gc.setup_taus(k))
        assert {"random", "0", "1", "r-1"} <= set(taus) and (("omega^3" in taus) == (k >= 2))
        for name, tau in taus.items():
            L = gc.lagrange_at(tau, k)
            for m in sorted({0, 1, n // 2, n - 1} & set(range(n))):
                assert sum(L[i] * pow(w, i * m, R) for i in range(n)) % R == pow(tau, m, R), (k, name, m)
            old = gc.lagrange_as_the_kernel_had_it(tau, k)
            inside = pow(tau, n, R) == 1
            assert inside == (name in ("1", "omega^3") or (name == "r-1" and k >= 1))
            if inside:
                j = L.index(1)
                assert pow(w, j, R) == tau and sum(L) == 1 and not any(old) and j == {"1": 0, "r-1": n // 2, "omega^3": 3}[name]
            else:
                assert old == L
            assert P.frs_from_bytes(O.fr_powers(gc.mont([tau]), n).tobytes()) == [pow(tau, i, R) for i in range(n)]
        assert gc.lagrange_at(0, k) == [pow(n, -1, R)] * n
