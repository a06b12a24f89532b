"""What the first nine commitments of a proof MUST be, from the protocol's definition and Python integers: helpers shared by
test_prover_definition_cpu.py and test_gpu_prover_definition.py, no tests of their own.  No HIP, no torch; uses oracle/.

A restatement of phases 1-3 of halo2's `create_proof` for the constraint system of circuits_halo2_amd.mst_inclusion: the three
advice columns, the lookup's permuted pair a' / s', the two permutation grand products and the lookup grand product as Lagrange
columns of n = 2^k canonical integers, and the random polynomial as its n COEFFICIENTS -- blinding rows included, because the
blinding values are a ChaCha20 stream of a known key (oracle.pyref.chacha_field_elements) and the SRS of the tests has a known
tau, so each commitment is one scalar times the generator: (sum_i v_i L_i(tau)) G for a Lagrange column, (sum_i c_i tau^i) G for
the random polynomial (halo2's vanishing::Argument::commit fills `domain.empty_coeff()` and commits in the monomial basis;
SURVEY.md section 3.1 step 7).  The verifier cannot see the blinding rows; this can.

Phases 4-6 (quotient, evaluations, multi-open) are NOT restated: once the nine commitments are the definition's, the five quotient
pieces' sum, every evaluation, W and W' are fixed up to the soundness of the protocol, and oracle.summa_verifier.verify accepting
the proof carries them.  check_proof asserts that acceptance and, of the points it cannot pin, only that they are points.

THE EASIEST THING TO GET WRONG: a drawn value is 32 raw bytes stored into a column of MONTGOMERY words (halo2curves keeps field
elements as a * 2^256 mod r; both drivers write the stream's words into the column as they come, which is as uniform as any other
reading).  The field element a drawn word w stands for is therefore  w * 2^-256 mod r,  not w.  chacha_field_elements returns the
raw words; drawn() below converts.

The row ranges and the draw numbers are constants of THIS file, from halo2, not imported from the drivers under test.
"""
import functools

import lookup_permute_cases as lc
from oracle import pyref as PR
from oracle import summa_verifier as SV

R = PR.R
G = PR.G1_GEN
MONT_INV = pow(PR.MONT, -1, R)

# halo2 `ConstraintSystem::blinding_factors()` + 1: the last rows of every column are not usable.  Advice (and the permuted lookup
# columns) are blinded from `unusable_rows_start = n - (blinding_factors + 1)` on (plonk/prover.rs: `for cell in &mut advice[unusable_rows_start..]`,
# lookup/prover.rs: `permuted_input_expression[unusable_rows_start..]`): rows [u, n).
# A grand product has n - blinding_factors = u + 1 computed rows -- z[u] is the closing value the verifier's l_last term and the
# rotation -(blinding_factors + 1) of the next chunk read (oracle/summa_verifier.py: ROT_LAST, l_last) -- and is blinded after it
# (permutation/prover.rs, lookup/prover.rs: `for z in &mut z[params.n() - blinding_factors..]`): rows [u + 1, n).
BLINDING_FACTORS = SV.BLINDING_FACTORS


def usable_rows(k):
    return (1 << k) - (BLINDING_FACTORS + 1)


# the order in which upstream's create_proof draws: one draw per advice column as it is blinded, then per lookup the permuted input
# and the permuted table, then per permutation chunk its product, then per lookup its product, then the random polynomial
# (vanishing argument).  Draw d is ChaCha20 stream id d of the proof's key.
NAMES = ("a0", "a1", "a2", "pin", "ptab", "z0", "z1", "lz", "random")
DRAWS = {"a0": 1, "a1": 2, "a2": 3, "pin": 4, "ptab": 5, "z0": 6, "z1": 7, "lz": 8, "random": 9}
# name -> the key of oracle.summa_verifier.COMMIT_ORDER
PROOF_KEY = {"a0": ("a", 0), "a1": ("a", 1), "a2": ("a", 2), "pin": ("pin", 0), "ptab": ("ptab", 0), "z0": ("z", 0), "z1": ("z", 1),
             "lz": ("lz", 0), "random": ("random", 0)}
assert [PROOF_KEY[name] for name in NAMES] == SV.COMMIT_ORDER[:9]


def blinding_rows(name, k):
    """(first row, count) of the rows of column `name` that hold its draw"""
    n, u = 1 << k, usable_rows(k)
    if name == "random":
        return 0, n
    if name in ("z0", "z1", "lz"):
        return u + 1, n - u - 1
    return u, n - u


@functools.lru_cache(maxsize=None)
def raw_words(key, draw, count):
    """the stream's words as the device writes them (32-byte little-endian integers below r)"""
    return tuple(PR.chacha_field_elements(key, draw, count))


def drawn(key, draw, count, reading="raw"):
    """the field elements that draw number `draw` puts into `count` rows.  reading "raw" (the definition): the word is stored as it
    is into a Montgomery column, so it stands for word * 2^-256; "montgomery" (a mistake, for the teeth test): the word is taken as
    the canonical value and converted on the way in"""
    words = raw_words(key, draw, count)
    if reading == "raw":
        return [w * MONT_INV % R for w in words]
    assert reading == "montgomery"
    return list(words)


def _inv(a):
    return pow(a, -1, R)


def _columns_of(asg, k):
    n = 1 << k
    inst = list(asg["instances"]) + [0] * (n - len(asg["instances"]))      # the instance column: the public inputs, then zeros
    return {"f": asg["fixed"], "a": asg["advice"], "i": [inst]}


def permutation_columns():
    """M.PERMUTATION_COLUMNS as ("f" | "a" | "i", index) pairs and the chunk size"""
    from circuits_halo2_amd import arithmetic as A
    from circuits_halo2_amd import mst_inclusion as M
    kind = {A.FIXED: "f", A.ADVICE: "a", A.INSTANCE: "i"}
    return [(kind[c[0]], c[1]) for c in M.PERMUTATION_COLUMNS], M.PERMUTATION_CHUNK


def lookup_rows(asg, k):
    """-> (input, table) on the usable rows, row by row: the lookup's input expression (oracle.summa_verifier.lookup_input_table) and
    the table column fixed[4]"""
    n, u = 1 << k, usable_rows(k)
    # the expression reads a0 at rotation +1: on the last usable row that is a blinding row, whose selector must be off
    assert asg["fixed"][5][u - 1] == 0
    inp, tab = [], []
    for row in range(u):
        q = lambda kind, c, rot: (asg["fixed"] if kind == "f" else asg["advice"])[c][(row + rot) % n]
        i, t = SV.lookup_input_table(q)
        assert t == asg["fixed"][4][row]
        inp.append(i)
        tab.append(t)
    return inp, tab


def witness_columns(asg, k):
    """the five columns that depend on no challenge, with their blinding rows ZERO (what a prover that forgot to blind commits
    to): a0 a1 a2 on rows [0, u), a' s' = the lookup's input and table on rows [0, u) permuted by halo2's rule as
    lookup_permute_cases.expected states it"""
    n, u = 1 << k, usable_rows(k)
    pad = [0] * (n - u)
    out = {f"a{j}": [v % R for v in asg["advice"][j][:u]] + pad for j in range(3)}
    inp, tab = lookup_rows(asg, k)
    pin, ptab = lc.expected(inp, tab)
    out["pin"], out["ptab"] = pin + pad, ptab + pad
    return out


def permutation_products(asg, k, beta, gamma):
    """-> [z of chunk 0, z of chunk 1], each the u + 1 computed rows z[0 .. u]:
    z[0] = 1 (first chunk) or the previous chunk's z[u];  z[i + 1] = z[i] * prod_j (v_j[i] + beta delta^j omega^i + gamma) /
    prod_j (v_j[i] + beta sigma_j[i] + gamma), column j of the whole list carrying delta^j.  The values are the assignment's own
    (unblinded: only rows below u are read)."""
    u = usable_rows(k)
    cols, chunk = permutation_columns()
    values = _columns_of(asg, k)
    omega = PR.omega_for(k)
    out, start = [], 1
    for c0 in range(0, len(cols), chunk):
        z, w = [start], 1
        for i in range(u):
            num = den = 1
            for j in range(c0, min(c0 + chunk, len(cols))):
                kind, c = cols[j]
                v = values[kind][c][i]
                num = num * ((v + beta * pow(PR.DELTA, j, R) % R * w + gamma) % R) % R
                den = den * ((v + beta * asg["sigma"][j][i] + gamma) % R) % R
            z.append(z[-1] * num % R * _inv(den) % R)
            w = w * omega % R
        out.append(z)
        start = z[u]
    return out


def lookup_product(asg, k, pin, ptab, beta, gamma):
    """the u + 1 computed rows: z[0] = 1, z[i + 1] = z[i] (input_i + beta)(table_i + gamma) / ((a'_i + beta)(s'_i + gamma))"""
    inp, tab = lookup_rows(asg, k)
    z = [1]
    for i in range(usable_rows(k)):
        z.append(z[-1] * ((inp[i] + beta) % R) % R * ((tab[i] + gamma) % R) % R * _inv((pin[i] + beta) * (ptab[i] + gamma) % R) % R)
    return z


def expected_columns(asg, k, key, challenges, draws=None, reading="raw"):
    """-> {name: n canonical integers} for the nine NAMES: the vectors whose commitments a proof under the ChaCha20 key `key` and
    the transcript's `challenges` (beta, gamma) must carry -- eight Lagrange columns, and for "random" the n coefficients.
    `draws` (default DRAWS) and `reading` exist for the teeth test."""
    n = 1 << k
    draws = dict(DRAWS, **(draws or {}))
    beta, gamma = challenges["beta"], challenges["gamma"]
    cols = witness_columns(asg, k)
    z0, z1 = permutation_products(asg, k, beta, gamma)
    lz = lookup_product(asg, k, cols["pin"], cols["ptab"], beta, gamma)
    cols.update({"z0": z0, "z1": z1, "lz": lz, "random": []})
    out = {}
    for name in NAMES:
        first, count = blinding_rows(name, k)
        col = cols[name][:first] + drawn(key, draws[name], count, reading)
        assert len(col) == n, name
        out[name] = col
    return out


@functools.lru_cache(maxsize=None)
def lagrange_at(tau, k):
    """L_i(tau) = omega^i (tau^n - 1) / (n (tau - omega^i)) for the n rows"""
    n = 1 << k
    omega = PR.omega_for(k)
    common = (pow(tau, n, R) - 1) * _inv(n) % R
    out, w = [], 1
    for _ in range(n):
        out.append(w * common % R * _inv((tau - w) % R) % R)
        w = w * omega % R
    return tuple(out)


def commit_at_tau(column, tau, k):
    """the commitment of a Lagrange column under the SRS of a KNOWN tau, as an affine point (None: the identity): one scalar
    product and one multiplication of the generator"""
    weights = lagrange_at(tau % R, k)
    assert len(column) == len(weights)
    return PR.g1_mul(G, sum(v * l for v, l in zip(column, weights)) % R)


def commit_coefficients_at_tau(coeffs, tau):
    """the commitment of a polynomial given by its coefficients (monomial basis): (sum_i c_i tau^i) G"""
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * tau + c) % R
    return PR.g1_mul(G, acc)


def commit_named(name, vector, tau, k):
    """the commitment of expected_columns()[name]: the random polynomial is coefficients, everything else a Lagrange column"""
    return commit_coefficients_at_tau(vector, tau) if name == "random" else commit_at_tau(vector, tau, k)


def proof_points(proof, flavour="evm"):
    """-> the 16 points of a proof in order, as (name, point): the 14 commitments, W, W'"""
    comms, _, w, w2 = SV.parse_proof(proof) if flavour == "evm" else SV.parse_proof_blake2b(proof)
    names = list(NAMES) + [f"h{j}" for j in range(5)]
    return [(name, comms[key]) for name, key in zip(names, SV.COMMIT_ORDER)] + [("W", w), ("W'", w2)]


def replay_challenges(proof, instances, vk, flavour="evm"):
    """-> (accepted, trace): the verifier's verdict and every challenge it squeezed (the transcript is the verifier's own)"""
    trace = {}
    ok = SV.verify(proof, instances, vk, trace=trace, flavour=flavour)
    return ok, trace


def expected_points(asg, k, tau, key, challenges):
    cols = expected_columns(asg, k, key, challenges)
    return {name: commit_named(name, cols[name], tau, k) for name in NAMES}


def check_proof(proof, asg, k, tau, key, vk, flavour="evm"):
    """the verifier accepts; the first nine points are the definition's under `key` and the proof's own challenges, bit for bit;
    the five quotient pieces, W and W' are points of the curve other than the identity.  -> {name: point} of all 16"""
    ok, trace = replay_challenges(proof, asg["instances"], vk, flavour)
    assert ok, "the verifier rejects the proof"
    got = dict(proof_points(proof, flavour))
    want = expected_points(asg, k, tau, key, trace)
    for name in NAMES:
        assert got[name] == want[name], f"commitment {name}: the proof's point is not the definition's"
    for name in [f"h{j}" for j in range(5)] + ["W", "W'"]:
        p = got[name]
        assert p is not None and p != (0, 0) and SV.on_curve(p), name
    return got
