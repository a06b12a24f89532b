"""The quotient's coset pipeline restated from outside the library: the quotient numerator is evaluated on the first n_cosets
cosets c_b H (c_b = zeta omega_ext^b, H the 2^k domain) of halo2's extended domain of 2^(k + ext) rows, and the quotient's
pieces h_0 .. h_{n_cosets - 1} of n = 2^k coefficients each follow from those values alone.  This module holds the grid of
(k, ext, n_cosets) shapes that tests/test_gpu_cosets.py runs, the coset-major layout, and two references built from the oracle
(oracle/oracle.py, oracle/pyref.py) and Python integers only: the numerator's coset values of known pieces, and the pieces of
arbitrary coset values.  tests/test_coset_cases_cpu.py ties both to halo2's extended_to_coeff(divide_by_vanishing_poly(..))
without a GPU.  How many cosets there are is the caller's choice: 1 .. 8, at most 2^ext."""
import numpy as np

import ntt_cases
from oracle import oracle as O
from oracle import pyref as PR

R = PR.R
MAX_COSETS = 8
KS = (3, 5, 7, 8, 9)           # 8 rows (less than a wave), 32, 128 (two blocks per workgroup), 256 (one workgroup), 512
PAIRS = ((1, 1), (1, 2), (2, 3), (2, 4), (3, 5), (3, 6), (3, 7), (3, 8), (4, 8))     # (ext, n_cosets)
LONG = (ntt_cases.BATCHED_MAX_LOG + 1, 1, 2)     # above the batched plans the 2^k transforms of the blocks run one by one


def domain_args(ext, n_cosets):
    """(j, n_cosets argument) with which the Python layer reaches a shape: EvaluationDomain(j, k) has j - 1 cosets of an
    extended domain of 2^(k + ceil(log2(j - 1))) rows; None: the domain's own count"""
    if (1 << ext) >= n_cosets > 1 and (1 << (ext - 1)) < n_cosets:
        return n_cosets + 1, None                       # j = 3 .. 9: 2 .. 8 cosets with their natural ext
    if n_cosets == 1:
        assert ext == 1
        return 3, 1                                     # (j = 2 would be ext_k = k: no coset outside the domain)
    assert (ext, n_cosets) == (4, 8)
    return 10, 8


def shapes():
    """[((k, ext, n_cosets), (j, n_cosets argument))]: every pair of PAIRS at every k of KS, and the long case"""
    grid = [(k, ext, nc) for k in KS for ext, nc in PAIRS] + [LONG]
    return [(s, domain_args(s[1], s[2])) for s in grid]


def threads():
    return min(16, O.ncpu())


def _fr(values):
    return np.frombuffer(PR.frs_to_bytes(values), dtype=np.uint8).copy()


def gather(ext_vec, k, ext, n_cosets):
    """extended vector (2^(k + ext) rows) -> coset-major (n_cosets blocks of 2^k rows): block b, row a = extended row a 2^ext + b"""
    n = 1 << k
    assert ext_vec.size == 32 << (k + ext) and 1 <= n_cosets <= 1 << ext
    return np.ascontiguousarray(ext_vec.reshape(n, 1 << ext, 32)[:, :n_cosets].transpose(1, 0, 2)).reshape(-1)


def shifts(k, ext, n_blocks):
    """c_b = zeta omega_ext^b, b < n_blocks (Python integers)"""
    w_ext = PR.omega_for(k + ext)
    return [PR.ZETA * pow(w_ext, b, R) % R for b in range(n_blocks)]


def gammas(k, ext, n_blocks):
    """g_b = c_b^n: what X^n is on the coset c_b H"""
    return [pow(c, 1 << k, R) for c in shifts(k, ext, n_blocks)]


def numerator_from_pieces(pieces, k, ext, n_cosets, n_blocks=None):
    """coset-major values of h(X) (X^n - 1), h = sum_t X^(n t) h_t, on the first n_blocks (default: n_cosets) cosets.  On c_b H
    the polynomial X^n is the constant g_b, so block b = (g_b - 1) sum_t g_b^t (h_t on c_b H)"""
    n_blocks = n_cosets if n_blocks is None else n_blocks
    assert len(pieces) == n_cosets
    n = 1 << k
    cos = [gather(O.coeff_to_extended(p, k, k + ext, threads()), k, ext, n_blocks) for p in pieces]
    out = []
    for b, g in enumerate(gammas(k, ext, n_blocks)):
        coeffs = _fr([(g - 1) * pow(g, t, R) % R for t in range(n_cosets)])
        out.append(O.fr_lincomb([c[32 * n * b:32 * n * (b + 1)] for c in cos], coeffs))
    return np.concatenate(out)


def _invert(m):
    """inverse of a square matrix mod r (Gauss-Jordan, Python integers)"""
    d = len(m)
    a = [list(row) + [int(i == j) for j in range(d)] for i, row in enumerate(m)]
    for col in range(d):
        piv = next(r for r in range(col, d) if a[r][col])
        a[col], a[piv] = a[piv], a[col]
        inv = pow(a[col][col], -1, R)
        a[col] = [v * inv % R for v in a[col]]
        for r in range(d):
            if r != col and a[r][col]:
                f = a[r][col]
                a[r] = [(v - f * w) % R for v, w in zip(a[r], a[col])]
    return [row[d:] for row in a]


def solve_matrix(k, ext, n_cosets):
    """M = V^-1 diag(1 / (g_b - 1)), V[b][t] = g_b^t: pieces[t] = sum_b M[t][b] P_b, P_b the coefficients of the numerator
    restricted to c_b H"""
    g = gammas(k, ext, n_cosets)
    v_inv = _invert([[pow(gb, t, R) for t in range(n_cosets)] for gb in g])
    return [[v_inv[t][b] * pow(g[b] - 1, -1, R) % R for b in range(n_cosets)] for t in range(n_cosets)]


def ref_cosets_to_pieces(values, k, ext, n_cosets):
    """the pieces of ARBITRARY coset-major values (they need not be the image of any pieces): per block the inverse transform
    of size n (coefficients of P_b(c_b X)), times c_b^-i, then the Vandermonde solve per coefficient index"""
    n = 1 << k
    assert values.size == 32 * n * n_cosets
    w_inv, n_inv = O.omega_inv(k), O.n_inv(k)
    rows = []
    for b, c in enumerate(shifts(k, ext, n_cosets)):
        blk = O.ifft(values[32 * n * b:32 * n * (b + 1)], w_inv, n_inv, k, threads())
        rows.append(O.fr_mul_n(blk, O.fr_powers(_fr([pow(c, -1, R)]), n)))
    return [O.fr_lincomb(rows, _fr(m_t)) for m_t in solve_matrix(k, ext, n_cosets)]


def max_word(rows):
    """the word r - 1: the largest canonical word (the value (r - 1) / 2^256 in Montgomery form)"""
    return np.tile(np.frombuffer((R - 1).to_bytes(32, "little"), dtype=np.uint8), rows)


def minus_one(rows):
    return np.tile(_fr([R - 1]), rows)


def _one_hot(rows, seed):
    v = np.zeros(32 * rows, dtype=np.uint8)
    v[-32:] = O.random_fr(seed, 1)
    assert v[-32:].any()
    return v


def value_fills():
    """[(name, fill(rows, seed) -> a whole vector)]"""
    return [("random", lambda rows, seed: O.random_fr(seed, rows)),
            ("zero", lambda rows, seed: np.zeros(32 * rows, dtype=np.uint8)),
            ("max_word", lambda rows, seed: max_word(rows)),
            ("minus_one", lambda rows, seed: minus_one(rows)),
            ("one_hot_last_row", _one_hot)]
