"""tests/prover_definition.py shown right, and shown to have teeth, without a device: the Lagrange weights against a naive MSM over
the Lagrange-basis points, the grand products closing on the example assignment under arbitrary challenges, the nine draws' row
counts, and -- the point of it all -- that each blinding mistake the GPU test exists to catch moves the expected commitment."""
import pytest

import lookup_permute_cases as lc
import mst_assignment as MA
import prover_definition as D
from oracle import pyref as PR

R = PR.R
K = 9
TAU = 0x1D0C0FFEE1234567890ABCDEF
KEY = bytes(range(32))
CHALLENGES = {"beta": 0x1234567890ABCDEF1234567890ABCDEF % R, "gamma": (R - 5) // 3}


@pytest.fixture(scope="module")
def asg():
    return MA.build(K)


@pytest.fixture(scope="module")
def columns(asg):
    return D.expected_columns(asg, K, KEY, CHALLENGES)


@pytest.mark.parametrize("k", [3, 4])
def test_lagrange_weights_against_a_naive_msm(k):
    n = 1 << k
    weights = D.lagrange_at(TAU, k)
    assert sum(weights) % R == 1
    # L_i is the polynomial that is 1 on omega^i and 0 on the other rows: at tau = omega^j (outside the formula's reach) by
    # interpolation, so check the defining property through a polynomial: sum_i omega^(i t) L_i(tau) = tau^t for t < n
    omega = PR.omega_for(k)
    for t in (1, 2, n - 1):
        assert sum(pow(omega, i * t, R) * w for i, w in enumerate(weights)) % R == pow(TAU, t, R)
    points = [PR.g1_mul(PR.G1_GEN, w) for w in weights]
    for column in ([1] + [0] * (n - 1), [0] * (n - 1) + [R - 1], [pow(3, 1000 + 17 * i, R) for i in range(n)], [5] * n):
        assert D.commit_at_tau(column, TAU, k) == PR.msm_naive(column, points)
        assert D.commit_coefficients_at_tau(column, TAU) == PR.msm_naive(column, [PR.g1_mul(PR.G1_GEN, pow(TAU, i, R)) for i in range(n)])
    # the two bases are two commitments of one polynomial: X^t is the column omega^(i t)
    assert D.commit_at_tau([pow(omega, 3 * i, R) for i in range(n)], TAU, k) == D.commit_coefficients_at_tau([0, 0, 0, 1], TAU)
    assert D.commit_at_tau([0] * n, TAU, k) is None
    assert D.commit_at_tau([5] * n, TAU, k) == PR.g1_mul(PR.G1_GEN, 5)          # a constant column commits to the constant


def test_products_close_and_the_permuted_pair_is_halo2s(asg, columns):
    n, u = 1 << K, D.usable_rows(K)
    assert u == asg["usable_rows"] == 506
    assert columns["z0"][0] == 1 and columns["z1"][0] == columns["z0"][u] and columns["z1"][u] == 1
    assert columns["z0"][u] != 1                     # the copy constraints cross the chunks: the first chunk alone does not close
    assert columns["lz"][0] == 1 and columns["lz"][u] == 1
    inp, tab = D.lookup_rows(asg, K)
    assert tab == asg["fixed"][4][:u] and any(inp)
    a, s = columns["pin"][:u], columns["ptab"][:u]
    assert (a, s) == lc.expected(inp, tab)
    assert a == sorted(inp) and sorted(s) == sorted(tab)
    assert all(a[i] == s[i] or (i and a[i] == a[i - 1]) for i in range(u))
    # usable rows of the advice columns are the assignment's
    for j in range(3):
        assert columns[f"a{j}"][:u] == asg["advice"][j][:u]
    assert all(len(columns[name]) == n and max(columns[name]) < R for name in D.NAMES)
    # other challenges: other products, closing all the same
    other = D.expected_columns(asg, K, KEY, {"beta": 7, "gamma": R - 1000})    # (no table value + gamma is zero)
    assert other["z1"][u] == 1 and other["lz"][u] == 1 and other["z0"][:u + 1] != columns["z0"][:u + 1]


def test_draw_counts_and_disjoint_streams(columns):
    n, u = 1 << K, D.usable_rows(K)
    assert sorted(D.DRAWS.values()) == list(range(1, 10)) and [D.DRAWS[name] for name in D.NAMES] == list(range(1, 10))
    want = {"a0": (u, 6), "a1": (u, 6), "a2": (u, 6), "pin": (u, 6), "ptab": (u, 6), "z0": (u + 1, 5), "z1": (u + 1, 5), "lz": (u + 1, 5),
            "random": (0, n)}
    words = {}
    for name in D.NAMES:
        assert D.blinding_rows(name, K) == want[name]
        first, count = want[name]
        assert first + count == n
        words[name] = D.raw_words(KEY, D.DRAWS[name], count)
        assert len(words[name]) == count == len(set(words[name]))
        # the column's tail is the draw, read as the Montgomery word it is stored as
        assert columns[name][first:] == [w * pow(1 << 256, -1, R) % R for w in words[name]]
        assert [v * (1 << 256) % R for v in columns[name][first:]] == list(words[name])
    for a in D.NAMES:
        for b in D.NAMES:
            if a < b:
                assert not set(words[a]) & set(words[b]), (a, b)


def _zero_one_row(col):
    u = D.usable_rows(K)
    return col[:u + 2] + [0] + col[u + 3:]


def _shift_up(col):
    """the blinding of a grand product written one row early: rows [u, n - 1), the last row as the product left it (zero here)"""
    u = D.usable_rows(K)
    return col[:u] + col[u + 1:] + [0]


MUTATIONS = {
    "a0 and a1 draw ids swapped": ("a0", lambda asg, cols: D.expected_columns(asg, K, KEY, CHALLENGES, draws={"a0": 2, "a1": 1})["a0"]),
    "one blinding row of a2 zeroed": ("a2", lambda asg, cols: _zero_one_row(cols["a2"])),
    "z0 blinding shifted to [u, n-1)": ("z0", lambda asg, cols: _shift_up(cols["z0"])),
    "lz blinded with draw 7 instead of 8": ("lz", lambda asg, cols: D.expected_columns(asg, K, KEY, CHALLENGES, draws={"lz": 7})["lz"]),
    "random truncated to n-1 values": ("random", lambda asg, cols: cols["random"][:-1] + [0]),
    "raw word read as a canonical value": ("a1", lambda asg, cols: D.expected_columns(asg, K, KEY, CHALLENGES, reading="montgomery")["a1"]),
}


@pytest.mark.parametrize("what", list(MUTATIONS))
def test_teeth_each_blinding_mistake_moves_the_expected_point(asg, columns, what):
    name, mutate = MUTATIONS[what]
    wrong = mutate(asg, columns)
    n, u = 1 << K, D.usable_rows(K)
    assert len(wrong) == n and wrong != columns[name]
    first = D.blinding_rows(name, K)[0]
    assert wrong[:min(first, u)] == columns[name][:min(first, u)]            # the rows the constraints are checked on are untouched
    assert D.commit_named(name, wrong, TAU, K) != D.commit_named(name, columns[name], TAU, K)
    if what == "a0 and a1 draw ids swapped":                                   # ... and the swapped column is the other's blinding
        assert wrong[u:] == columns["a1"][u:]
    if what == "raw word read as a canonical value":
        assert wrong[u:] == list(D.raw_words(KEY, D.DRAWS["a1"], n - u))


def test_the_random_polynomial_is_coefficients_not_a_lagrange_column(columns):
    """halo2 draws the vanishing argument's random polynomial in coefficient form and commits it in the monomial basis: read as a
    Lagrange column the same n values commit to another point"""
    assert D.commit_named("random", columns["random"], TAU, K) == D.commit_coefficients_at_tau(columns["random"], TAU)
    assert D.commit_coefficients_at_tau(columns["random"], TAU) != D.commit_at_tau(columns["random"], TAU, K)


def test_points_of_a_proof_are_named_in_the_verifiers_order():
    """proof_points on a synthetic 2144-byte proof: 16 names in the proof's order, the words big-endian"""
    proof = b"".join(i.to_bytes(32, "big") for i in range(1, 68))
    pts = D.proof_points(proof)
    assert [name for name, _ in pts] == list(D.NAMES) + ["h0", "h1", "h2", "h3", "h4", "W", "W'"]
    assert pts[0][1] == (1, 2) and pts[8][1] == (17, 18) and pts[13][1] == (27, 28) and pts[14][1] == (64, 65) and pts[15][1] == (66, 67)
