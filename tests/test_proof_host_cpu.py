"""The HIP-free half of the compiled prover (include/summa_fr.hpp, summa_transcript.hpp, summa_proof_host.hpp) against
Python integers, without a GPU: tests/cpp/proof_host_check.cpp is built with a host compiler alone (no ROCm include path,
no HIP define -- compiling is the proof that the headers are HIP-free), under -Werror and address / undefined sanitizers,
and prints what the functions return for inputs this test makes up at k = 4 (n = 16, where ROT_LAST = -6 is a point of
its own).

Per seed: every polynomial of the rotation sets is a seeded random polynomial of degree < 16, h is five such pieces, and
every evaluation is computed here.  Checked: the definitions (r_i by this file's own Lagrange interpolation, c_j, the
weights nu^i c_j, h(x), the points, the products outside each set), and the identity that ties them together: with
f_i = q_i - r_i divided exactly by Z_{S_i} (long division, remainder zero) and f = sum_i nu^i f_i / Z_{S_i}, the
linearisation L built from the printed scales, the printed coefficient of f and the printed low coefficients vanishes at mu."""
import hashlib
import os
import random
import subprocess

import pytest

from conftest import ROOT

from circuits_halo2_amd import mst_inclusion as M
from circuits_halo2_amd import prover as P
from circuits_halo2_amd.merkle_sum_tree import keccak256

R, Q = P.R, P.Q
K, N = 4, 16
OMEGA = pow(P.ROOT_OF_UNITY, 1 << (28 - K), R)
PIECES = 5
GATE_CASES = [[[0, 1, 5], [2], [], [7, 7, 300]],        # every exponent below 2^16: the power table
              [[1, 1 << 16], [(1 << 16) + 3, 2]],        # an exponent at / above 2^16: one exponentiation per term
              []]                                        # no challenges: one zero, so that the kernel has a pointer


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("proof_host") / "proof_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "proof_host_check.cpp"), "-o", out])
    return out


def hx(v):
    return "%064x" % v


def run(exe, scalars, evals, piece_evals, fq_inputs):
    words = [str(K)] + [hx(v) for v in scalars + evals + piece_evals] + [str(len(GATE_CASES))]
    for case in GATE_CASES:
        words.append(str(len(case)))
        for group in case:
            words += [str(len(group))] + [str(e) for e in group]
    words += [str(len(fq_inputs))] + [b.hex() for b in fq_inputs]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], input=" ".join(words), capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    out = {}
    for ln in r.stdout.splitlines():
        name, _, rest = ln.partition(" ")
        out.setdefault(name, []).append(rest.split())
    return out


def ints(words):
    return [int(w, 16) for w in words]


# ---- polynomials over Python integers, coefficients low to high
def ev(c, x):
    acc = 0
    for a in reversed(c):
        acc = (acc * x + a) % R
    return acc


def mul_linear(c, p):                       # c(X) (X - p)
    out = [0] * (len(c) + 1)
    for i, a in enumerate(c):
        out[i + 1] = (out[i + 1] + a) % R
        out[i] = (out[i] - p * a) % R
    return out


def add_scaled(acc, c, s):
    acc = acc + [0] * (len(c) - len(acc))
    for i, a in enumerate(c):
        acc[i] = (acc[i] + s * a) % R
    return acc


def divmod_poly(a, b):                      # long division by a monic b
    a = list(a)
    quo = [0] * max(len(a) - len(b) + 1, 0)
    for i in range(len(a) - len(b), -1, -1):
        quo[i] = a[i + len(b) - 1]
        for j, bj in enumerate(b):
            a[i + j] = (a[i + j] - quo[i] * bj) % R
    return quo, a


def interpolate(pts, vals):
    out = [0] * len(pts)
    for i, pi in enumerate(pts):
        basis, den = [1], 1
        for j, pj in enumerate(pts):
            if j != i:
                basis = mul_linear(basis, pj)
                den = den * (pi - pj) % R
        out = add_scaled(out, basis, vals[i] * pow(den, -1, R))
    return out


def vanishing(pts):
    z = [1]
    for p in pts:
        z = mul_linear(z, p)
    return z


def point(x, rot):
    return x * pow(OMEGA, rot % N, R) % R


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_multiopen_scalars_against_python_integers(exe, seed):
    rng = random.Random(seed)
    fe = lambda: rng.randrange(1, R)
    x, y, zeta, nu, mu = (fe() for _ in range(5))
    polys = {}
    for _, keys in P.ROTATION_SETS:
        for key in keys:
            polys[key] = [fe() for _ in range(N)]
    pieces = [[fe() for _ in range(N)] for _ in range(PIECES)]
    polys[("h", None)] = [c for piece in pieces for c in piece]          # h(X) = sum_i X^(n i) h_i(X)
    evals = [ev(polys[(name, idx)], point(x, rot)) for name, idx, rot in P.EVAL_ORDER]
    piece_evals = [ev(piece, x) for piece in pieces]
    fq_values = [0, 1, Q - 1, rng.randrange(Q)]
    out = run(exe, [OMEGA, x, y, zeta, nu, mu], evals, piece_evals,
              [((v << 256) % Q).to_bytes(32, "little") for v in fq_values])       # Montgomery words, as the C ABI returns them

    # the shape tables are those of the Python driver
    assert [(w[0], int(w[1]), int(w[2])) for w in out["eval_order"]] == P.EVAL_ORDER
    got_sets = []
    for w in out["rotation_set"]:
        bar = w.index("|")
        keys = [(t.split(":")[0], None if t.startswith("h:") else int(t.split(":")[1])) for t in w[bar + 1:]]
        got_sets.append((tuple(int(r) for r in w[:bar]), keys))
    assert got_sets == [(tuple(rots), list(keys)) for rots, keys in P.ROTATION_SETS]
    assert [(int(w[0]), int(w[1])) for w in out["perm"]] == M.PERMUTATION_COLUMNS
    assert P.ROT_LAST == -6 and len({point(x, r) for r in (-6, -1, 0, 1)}) == 4

    # definitions
    x_n = pow(x, N, R)
    assert ints(out["xn_pow"][0]) == [pow(x_n, i, R) for i in range(PIECES)]
    h_eval = sum(pow(x_n, i, R) * piece_evals[i] for i in range(PIECES)) % R
    assert ints(out["h_eval"][0]) == [h_eval] == [ev(polys[("h", None)], x)]
    assert {int(w[0]): int(w[1], 16) for w in out["point"]} == {r: point(x, r) for r in (-6, -1, 0, 1)}
    claimed = {(name, idx, rot): v for (name, idx, rot), v in zip(P.EVAL_ORDER, evals)}
    value = lambda key, rot: h_eval if key[0] == "h" else claimed[(key[0], key[1], rot)]
    rs, cs = [], []
    for si, (rots, keys) in enumerate(P.ROTATION_SETS):
        pts = [point(x, r) for r in rots]
        c = []
        for j, pj in enumerate(pts):
            den = 1
            for t, pt in enumerate(pts):
                if t != j:
                    den = den * (pj - pt) % R
            c.append(pow(den, -1, R))
        assert ints(out["denom_inv"][si]) == c
        vals = [sum(pow(zeta, j, R) * value(key, r) for j, key in enumerate(keys)) % R for r in rots]
        r_i = interpolate(pts, vals)
        assert ints(out["r"][si]) == r_i
        rs.append(r_i)
        cs.append(c)
    assert ints(out["div_points"][0]) == [point(x, r) for rots, _ in P.ROTATION_SETS for r in rots] and len(out["div_points"][0]) == 11
    assert ints(out["div_weights"][0]) == [pow(nu, si, R) * c % R for si in range(len(cs)) for c in cs[si]]
    mu_minus = {r: (mu - point(x, r)) % R for r in (-6, -1, 0, 1)}
    assert {int(w[0]): int(w[1], 16) for w in out["mu_minus"]} == mu_minus
    outside = []
    for rots, _ in P.ROTATION_SETS:
        d = 1
        for r, v in mu_minus.items():
            if r not in rots:
                d = d * v % R
        outside.append(d)
    assert ints(out["outside"][0]) == outside
    z_s0 = 1
    for r in P.ROTATION_SETS[0][0]:
        z_s0 = z_s0 * mu_minus[r] % R
    assert ints(out["z_s0"][0]) == [z_s0]
    assert out["five_points_refused"] == [["1"]]

    # the identity: L(mu) == 0 with the scales, the coefficient of f and the low coefficients the C++ printed
    lin_coeffs, lin_low = ints(out["lin_coeffs"][0]), ints(out["lin_low"][0])
    assert len(lin_coeffs) == len(P.ROTATION_SETS) + 1 and len(lin_low) == 4
    assert lin_coeffs[-1] == (-z_s0) % R
    assert lin_coeffs[:-1] == [pow(nu, i, R) * outside[i] * pow(outside[0], -1, R) % R for i in range(len(outside))]
    f, l_at_mu = [], 0
    for si, (rots, keys) in enumerate(P.ROTATION_SETS):
        q_i = []
        for j, key in enumerate(keys):
            q_i = add_scaled(q_i, polys[key], pow(zeta, j, R))
        f_i = add_scaled(q_i, rs[si], R - 1)
        quo, rem = divmod_poly(f_i, vanishing([point(x, r) for r in rots]))
        assert not any(rem)
        f = add_scaled(f, quo, pow(nu, si, R))
        l_at_mu += lin_coeffs[si] * ev(f_i, mu)
    l_at_mu += lin_coeffs[-1] * ev(f, mu) + ev(lin_low, mu)
    assert l_at_mu % R == 0

    # gate challenges: sums of powers of y, both branches and the empty list
    want = [[sum(pow(y, e, R) for e in group) % R for group in case] or [0] for case in GATE_CASES]
    assert [ints(w) for w in out["gate_challenges"]] == want

    # the Fq byte conversion and both transcripts
    assert out["fq_constants"] == [["1"]]
    assert [int(w[0], 16) for w in out["fq_be"]] == fq_values
    be = lambda v: v.to_bytes(32, "big")
    h1 = keccak256(be(x) + be(y))
    h2 = keccak256(h1 + b"\x01")
    assert ints(out["evm_squeeze"][0]) == [int.from_bytes(h1, "big") % R, int.from_bytes(h2, "big") % R]
    assert out["evm_proof"] == [[be(x).hex()]]
    le = lambda v: v.to_bytes(32, "little")
    st = hashlib.blake2b(digest_size=64, person=b"Halo2-Transcript")
    st.update(b"\x02" + le(x) + b"\x02" + le(y))
    squeezed = []
    for _ in range(2):
        st.update(b"\x00")
        squeezed.append(int.from_bytes(st.copy().digest(), "little") % R)
    assert ints(out["blake2b_squeeze"][0]) == squeezed
    assert out["blake2b_proof"] == [[le(x).hex()]]
