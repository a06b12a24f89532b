"""CPU checks of tests/coset_cases.py, the references behind tests/test_gpu_cosets.py: the numerator built coset by coset from
known pieces is halo2's (extended_to_coeff(divide_by_vanishing_poly(..)) of it over the WHOLE extended domain returns the
pieces), the reference for arbitrary coset values inverts it and is linear, the layout is the one the library documents, and
the grid reaches every coset count, every ext_k - k and the row counts it names -- without a GPU."""
import numpy as np
import pytest

import coset_cases as cc
from oracle import oracle as O

SMALL = [s for s, _ in cc.shapes() if s[0] <= 9]
_ids = lambda s: "k%d-ext%d-nc%d" % s


def _pieces(k, nc, seed):
    return [O.random_fr(seed + t, 1 << k) for t in range(nc)]


def _rows_equal(got, want):
    return got.size == want.size and bool((got == want).all())


def test_gather_is_the_documented_layout():
    """block b, row a = extended row a 2^ext + b, on a vector whose rows carry their own index"""
    for k, ext, nc in [(3, 1, 1), (3, 1, 2), (5, 2, 3), (4, 3, 8), (3, 4, 8)]:
        n, rows = 1 << k, 1 << (k + ext)
        v = np.zeros((rows, 32), dtype=np.uint8)
        v[:, 0] = np.arange(rows) % 256
        v[:, 1] = np.arange(rows) // 256
        g = cc.gather(v.reshape(-1), k, ext, nc).reshape(nc, n, 32)
        for b in range(nc):
            for a in range(n):
                assert int(g[b, a, 0]) + 256 * int(g[b, a, 1]) == a * (1 << ext) + b, (k, ext, nc, b, a)


@pytest.mark.parametrize("shape", SMALL, ids=_ids)
def test_the_numerator_of_known_pieces_is_halo2s(shape):
    """the numerator h (X^n - 1) built block by block over all 2^ext cosets, put back into the extended order, divided by the
    vanishing polynomial and taken to coefficients by the oracle's halo2 functions: the pieces, then zeros; the first
    n_cosets blocks of it are numerator_from_pieces"""
    k, ext, nc = shape
    n, full = 1 << k, 1 << ext
    g = cc.gammas(k, ext, full)
    assert len(set(g)) == full and 1 not in g
    pieces = _pieces(k, nc, 100 * k + 10 * ext + nc)
    cm = cc.numerator_from_pieces(pieces, k, ext, nc, n_blocks=full)
    ext_vec = np.ascontiguousarray(cm.reshape(full, n, 32).transpose(1, 0, 2)).reshape(-1)      # row a 2^ext + b <- block b, row a
    assert _rows_equal(cc.gather(ext_vec, k, ext, full), cm)
    coeffs = O.extended_to_coeff(O.divide_by_vanishing_poly(ext_vec, k, k + ext), k, k + ext)
    assert _rows_equal(coeffs[:32 * n * nc], np.concatenate(pieces))
    assert not coeffs[32 * n * nc:].any()
    assert _rows_equal(cc.numerator_from_pieces(pieces, k, ext, nc), cm[:32 * n * nc])


@pytest.mark.parametrize("shape", SMALL, ids=_ids)
def test_the_reference_for_arbitrary_values_inverts_the_numerator_and_is_linear(shape):
    k, ext, nc = shape
    n = 1 << k
    pieces = _pieces(k, nc, 7000 + 100 * k + 10 * ext + nc)
    back = cc.ref_cosets_to_pieces(cc.numerator_from_pieces(pieces, k, ext, nc), k, ext, nc)
    assert len(back) == nc
    for t in range(nc):
        assert _rows_equal(back[t], pieces[t]), t
    a, b = O.random_fr(8100 + k, nc * n), O.random_fr(8200 + k, nc * n)
    lam = O.random_fr(8300 + k, 2)
    both = cc.ref_cosets_to_pieces(O.fr_lincomb([a, b], lam), k, ext, nc)
    pa, pb = cc.ref_cosets_to_pieces(a, k, ext, nc), cc.ref_cosets_to_pieces(b, k, ext, nc)
    for t in range(nc):
        assert _rows_equal(both[t], O.fr_lincomb([pa[t], pb[t]], lam)), t


def test_the_solve_matrix_inverts_the_vandermonde_matrix():
    """M diag(g_b - 1) V = 1 with Python integers, at every pair of the grid"""
    for ext, nc in cc.PAIRS:
        g, m = cc.gammas(5, ext, nc), cc.solve_matrix(5, ext, nc)
        for t in range(nc):
            for u in range(nc):
                assert sum(m[t][b] * (g[b] - 1) * pow(g[b], u, cc.R) for b in range(nc)) % cc.R == int(t == u), (ext, nc, t, u)


def test_the_librarys_coset_arithmetic_is_the_restated_one(tmp_path):
    """csrc/coset_plan.h (what coset_tables_for uploads), through tests/cpp/coset_plan_check.cpp and plain g++: at every shape of
    the grid the shifts, their inverses and the solve matrix are coset_cases.shifts, their modular inverses and
    coset_cases.solve_matrix, word for word (the 32 bytes in memory); equal gammas are refused as a singular matrix, a coset
    inside the domain as such"""
    import os
    import subprocess
    from oracle import pyref as PR
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "coset_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(root, "circuits_halo2_amd", "csrc"),
                           os.path.join(root, "tests", "cpp", "coset_plan_check.cpp"), "-o", exe])
    word = lambda x: PR.fr_to_bytes(x % cc.R).hex()
    shapes = [s for s, _ in cc.shapes()]
    lines = [f"{k} {ext} {nc} {word(PR.ZETA)} {word(PR.omega_for(k + ext))}" for k, ext, nc in shapes]
    lines += [f"5 1 2 {word(PR.ZETA)} {word(1)}", f"5 1 2 {word(1)} {word(PR.omega_for(6))}"]
    got = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")[:-1]
    assert len(got) == len(lines)
    for (k, ext, nc), line in zip(shapes, got):
        c = cc.shifts(k, ext, nc)
        m = cc.solve_matrix(k, ext, nc)
        want = ("ok shift=" + ",".join(word(x) for x in c) + " inv_shift=" + ",".join(word(pow(x, -1, cc.R)) for x in c)
                + " m=" + ",".join(word(m[t][b]) for t in range(nc) for b in range(nc)))
        assert line == want, (k, ext, nc)
    assert got[len(shapes):] == ["singular", "inside_domain"]


def test_the_fills_are_what_they_say():
    fills = dict(cc.value_fills())
    assert list(fills) == ["random", "zero", "max_word", "minus_one", "one_hot_last_row"]
    rows = 24
    word = lambda v, i: int.from_bytes(v[32 * i:32 * i + 32].tobytes(), "little")
    for name, fill in fills.items():
        v = fill(rows, 5)
        assert v.dtype == np.uint8 and v.size == 32 * rows, name
        assert all(word(v, i) < cc.R for i in range(rows)), name           # canonical words
    assert len({word(fills["random"](rows, 5), i) for i in range(rows)}) == rows
    assert not fills["zero"](rows, 5).any()
    assert all(word(fills["max_word"](rows, 5), i) == cc.R - 1 for i in range(rows))
    assert all(word(fills["minus_one"](rows, 5), i) * pow(1 << 256, -1, cc.R) % cc.R == cc.R - 1 for i in range(rows))
    hot = fills["one_hot_last_row"](rows, 5)
    assert not hot[:-32].any() and hot[-32:].any()


def test_the_grid_reaches_what_it_claims():
    grid = cc.shapes()
    shapes = [s for s, _ in grid]
    assert len(set(shapes)) == len(shapes) == len(cc.KS) * len(cc.PAIRS) + 1
    assert {nc for _, _, nc in shapes} == set(range(1, cc.MAX_COSETS + 1))
    assert {ext for _, ext, _ in shapes} == {1, 2, 3, 4}
    assert all(1 <= nc <= 1 << ext for _, ext, nc in shapes)
    assert any(nc == 1 << ext for _, ext, nc in shapes) and any(nc < 1 << ext for _, ext, nc in shapes)
    ks = {k for k, _, _ in shapes}
    assert min(ks) < 8 and 8 in ks and max(ks) > 18
    assert {(1 << k) for k in ks} >= {8, 32, 128, 256, 512}
    assert [s for s in shapes if s[0] > 9] == [(19, 1, 2)]
    for k in cc.KS:                                            # every pair at every k
        assert {(e, c) for kk, e, c in shapes if kk == k} == set(cc.PAIRS)
    # the Python layer's way to each shape: halo2's EvaluationDomain::new(j, k) has j - 1 cosets, ext = ceil(log2(j - 1))
    for (k, ext, nc), (j, arg) in grid:
        degree = j - 1
        assert (degree - 1).bit_length() == ext, (k, ext, nc)
        assert (degree if arg is None else arg) == nc
        assert arg is None or arg < degree
    assert {j for _, (j, arg) in grid if arg is None} == set(range(3, 10))
