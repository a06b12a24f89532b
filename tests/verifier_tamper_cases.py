"""A catalogue of single-change tampers of one inclusion proof, its public inputs and its verifying key, built from the proof's
layout (oracle.summa_verifier.COMMIT_ORDER / EVAL_ORDER: 14 commitments, 35 evaluations, W, W'); shared by
test_verifier_binding_cpu.py and test_gpu_verifier_binding.py.  A plain helper module like verify_batch_cases.py: no tests here.

    EVM flavour      64-byte points (x || y big-endian), evaluations from 0x380, W at 0x7e0, W' at 0x820: 2144 bytes
    Blake2b flavour  32-byte fields (compressed points, little-endian scalars): 1632 bytes

A case is Case(id, family, proof, instances, key_change, parses, field):
    key_change  None, or a function from a key (the dict of `reference_key_dict`) to a changed key
    parses      every field is still the canonical encoding of a curve point / a field element, so that a verifier can refuse the
                case at the pairing only (key cases change trusted input that has no encoding: always True)
    field       the one field the case changes (("point", i), ("scalar", j), ("instance", i), ("key", name)), or None for a
                change of the shape (lengths, counts)
Every generator asserts its own intent: the case differs from the original in exactly the named field, a parses=True point is
on the curve and is another point, an alias is congruent to the original mod q / mod r and is not canonical.

A single-field change before the last challenge (mu) is refused by Fiat-Shamir alone for a verifier that absorbs what it reads;
the cases with teeth are the aliases (a reader that reduces before it absorbs accepts them), W' (read after mu: only the
pairing binds it) and the key / params family (never absorbed: bound by their coefficients in the final check alone)."""
import json
import os
from collections import namedtuple

from oracle import pyref as PR
from oracle import summa_verifier as SV

Q, R = PR.Q, PR.R
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
H = lambda s: int(s, 16)
FAMILIES = ("point", "scalar", "instance", "length", "key")
POINT_NAMES = ["%s%d" % key for key in SV.COMMIT_ORDER] + ["W", "W2"]          # W2 = W', the one field after the last challenge
SCALAR_NAMES = ["%s%d@%d" % key for key in SV.EVAL_ORDER]
N_POINTS, N_SCALARS = len(POINT_NAMES), len(SCALAR_NAMES)
KEY_COMMITMENTS = [("fixed_comms", j) for j in range(SV.NUM_FIXED)] + [("permutation_comms", j) for j in range(len(SV.PERMUTATION_COLUMNS))]

Case = namedtuple("Case", "id family proof instances key_change parses field")


# ------------------------------------------------------------------ layout
def point_size(flavour):
    return 64 if flavour == "evm" else 32


def point_offset(i, flavour):
    """byte offset of proof point i (0..13 the commitments, 14 = W, 15 = W')"""
    size = point_size(flavour)
    return size * i if i < len(SV.COMMIT_ORDER) else size * len(SV.COMMIT_ORDER) + 32 * N_SCALARS + size * (i - len(SV.COMMIT_ORDER))


def scalar_offset(j, flavour):
    return point_size(flavour) * len(SV.COMMIT_ORDER) + 32 * j


def proof_length(flavour):
    return point_size(flavour) * N_POINTS + 32 * N_SCALARS


assert proof_length("evm") == 2144 and scalar_offset(0, "evm") == 0x380 and point_offset(14, "evm") == 0x7e0 and point_offset(15, "evm") == 0x820
assert proof_length("blake2b") == 1632


def field_boundaries(flavour):
    """the offsets at which a field ends and the next begins (neither 0 nor the whole length)"""
    ends = [point_offset(i, flavour) for i in range(1, N_POINTS)] + [scalar_offset(j, flavour) for j in range(N_SCALARS)]
    return sorted(set(ends) - {0})


def compress(p):
    """(x, y) -> 32 bytes: x little-endian, bit 6 of the last byte = the parity of y (bit 7 = infinity, never set here)"""
    enc = bytearray(p[0].to_bytes(32, "little"))
    assert enc[31] < 0x40
    enc[31] |= (p[1] & 1) << 6
    return bytes(enc)


def read_point(proof, i, flavour):
    off = point_offset(i, flavour)
    if flavour == "evm":
        return (int.from_bytes(proof[off:off + 32], "big"), int.from_bytes(proof[off + 32:off + 64], "big"))
    return SV.decompress_g1(proof[off:off + 32])


def encode_point(p, flavour):
    return p[0].to_bytes(32, "big") + p[1].to_bytes(32, "big") if flavour == "evm" else compress(p)


def read_scalar(proof, j, flavour):
    off = scalar_offset(j, flavour)
    return int.from_bytes(proof[off:off + 32], "big" if flavour == "evm" else "little")


def _splice(proof, off, new):
    """the proof with the field at `off` replaced: nothing else changes, and the field does"""
    out = proof[:off] + new + proof[off + len(new):]
    assert len(out) == len(proof) and out[:off] == proof[:off] and out[off + len(new):] == proof[off + len(new):]
    assert out[off:off + len(new)] != proof[off:off + len(new)]
    return out


# ------------------------------------------------------------------ families: proof points
def x_plus_q_points(proof):
    """the Blake2b proof's points whose x + q still fits the 254 bits of a compressed point: only those have an x alias"""
    return [i for i in range(N_POINTS) if read_point(proof, i, "blake2b")[0] + Q < 1 << 254]


def point_cases(proof, instances, flavour):
    out = []
    for i, name in enumerate(POINT_NAMES):
        off, size = point_offset(i, flavour), point_size(flavour)
        x, y = p = read_point(proof, i, flavour)
        assert PR.g1_is_on_curve(p) and x < Q and y < Q and encode_point(p, flavour) == proof[off:off + size]

        def add(kind, raw, parses):
            assert len(raw) == size
            out.append(Case("%s-point-%s-%s" % (flavour, name, kind), "point", _splice(proof, off, raw), list(instances), None, parses,
                            ("point", i)))
        # well-formed other points: the pairing has to refuse them
        others = [("gen", (1, 2)), ("next", read_point(proof, (i + 1) % N_POINTS, flavour))]
        if flavour == "evm":
            others.insert(0, ("neg", (x, Q - y)))
        for kind, other in others:
            assert PR.g1_is_on_curve(other) and other != p and other[0] < Q and other[1] < Q
            add(kind, encode_point(other, flavour), True)
        if flavour == "evm":
            word = lambda a, b: a.to_bytes(32, "big") + b.to_bytes(32, "big")
            m = ((1 << 256) - 1 - x) // Q
            assert m >= 2 and x + m * Q < 1 << 256 <= x + (m + 1) * Q and y + Q < 1 << 256
            for kind, (ax, ay) in (("x+q", (x + Q, y)), ("y+q", (x, y + Q)), ("x+mq", (x + m * Q, y))):
                assert (ax - x) % Q == 0 and (ay - y) % Q == 0 and (ax >= Q or ay >= Q)          # an alias of the same point
                add(kind, word(ax, ay), False)
            add("zero", word(0, 0), False)
            add("y=0", word(x, 0), False)
            add("x=q", word(Q, y), False)
        else:
            raw = proof[off:off + 32]
            # the sign bit flipped is the negated point: a flag-bit change that still parses
            flipped = raw[:31] + bytes([raw[31] ^ 0x40])
            assert flipped == compress((x, Q - y)) and SV.decompress_g1(flipped) == (x, Q - y)
            add("neg-signbit", flipped, True)
            add("infinity-bit", raw[:31] + bytes([raw[31] | 0x80]), False)
            add("identity", bytes(31) + b"\x80", False)
            if x + Q < 1 << 254:
                alias = bytearray((x + Q).to_bytes(32, "little"))
                assert alias[31] < 0x40
                alias[31] |= raw[31] & 0x40
                assert int.from_bytes(bytes(alias[:31]) + bytes([alias[31] & 0x3F]), "little") % Q == x
                add("x+q", bytes(alias), False)
    return out


# ------------------------------------------------------------------ families: evaluations
def scalar_cases(proof, instances, flavour):
    out = []
    order = "big" if flavour == "evm" else "little"
    for j, name in enumerate(SCALAR_NAMES):
        off = scalar_offset(j, flavour)
        v = read_scalar(proof, j, flavour)
        assert v < R

        def add(kind, value, parses):
            assert value != v and (value < R) == parses and value < 1 << 256
            out.append(Case("%s-scalar-%s-%s" % (flavour, name, kind), "scalar", _splice(proof, off, value.to_bytes(32, order)),
                            list(instances), None, parses, ("scalar", j)))
        assert v != 0 and R - v != v, "the fixture's evaluations are non-zero: r - v is another canonical value"
        add("+1", (v + 1) % R, True)
        add("r-v", R - v, True)
        add("zero", 0 if v else 1, True)
        m = ((1 << 256) - 1 - v) // R
        assert m >= 2 and v + m * R < 1 << 256 <= v + (m + 1) * R
        for kind, alias in (("v+r", v + R), ("v+mr", v + m * R)):
            assert alias % R == v and alias >= R                       # an alias of the same value
            add(kind, alias, False)
        add("r", R, False)
        add("ones", (1 << 256) - 1, False)
    return out


# ------------------------------------------------------------------ families: public inputs
def instance_cases(proof, instances, flavour):
    out = []
    inst = [int(v) for v in instances]
    n = len(inst)
    assert n == 4 and all(0 <= v < R for v in inst)

    def add(kind, changed, parses, field):
        assert changed != inst
        out.append(Case("%s-instance-%s" % (flavour, kind), "instance", proof, changed, None, parses, field))
    for i, v in enumerate(inst):
        plus = list(inst)
        plus[i] = (v + 1) % R
        add("%d+1" % i, plus, True, ("instance", i))
        alias = list(inst)
        alias[i] = v + R
        assert alias[i] % R == v
        add("%d+r" % i, alias, False, ("instance", i))
    pairs = [(i, j) for i in range(n) for j in range(i + 1, n) if inst[i] != inst[j]]       # (equal values swapped change nothing)
    assert pairs and {i for pair in pairs for i in pair} == set(range(n)), "every public input is swapped with another at least once"
    for i, j in pairs:
        swapped = list(inst)
        swapped[i], swapped[j] = inst[j], inst[i]
        add("swap%d%d" % (i, j), swapped, True, None)
    add("fifth-zero", inst + [0], True, None)
    add("last-dropped", inst[:-1], True, None)
    return out


# ------------------------------------------------------------------ families: lengths
def length_cases(proof, instances, flavour):
    out = []
    assert len(proof) == proof_length(flavour)

    def add(kind, changed):
        assert len(changed) != len(proof)
        assert changed == proof[:len(changed)] or changed[:len(proof)] == proof
        out.append(Case("%s-length-%s" % (flavour, kind), "length", changed, list(instances), None, False, None))
    for cut in field_boundaries(flavour):
        add("cut%d" % cut, proof[:cut])
    add("byte-appended", proof + b"\x00")
    add("word-appended", proof + bytes(32))
    add("empty", b"")
    return out


# ------------------------------------------------------------------ families: the verifying key and the verifier params
def reference_key_dict():
    """the key of the reference's verifier contract (tests/golden/k6_verifier_trace.json) as the catalogue's plain dict: integers
    and integer tuples only -- {k, n_currencies, vk_digest, fixed_comms [11], permutation_comms [6], g2, s_g2}"""
    v = json.load(open(os.path.join(GOLD, "k6_verifier_trace.json")))["vk"]
    comm = [(H(a), H(b)) for a, b in v["commitments"]]
    neg_s_g2 = ((H(v["neg_s_g2_x_2"]), H(v["neg_s_g2_x_1"])), (H(v["neg_s_g2_y_2"]), H(v["neg_s_g2_y_1"])))
    return {"k": 11, "n_currencies": 2, "vk_digest": H(v["vk_digest"]), "fixed_comms": comm[:11], "permutation_comms": comm[11:],
            "g2": ((H(v["g2_x_2"]), H(v["g2_x_1"])), (H(v["g2_y_2"]), H(v["g2_y_1"]))), "s_g2": g2_neg(neg_s_g2)}


def g2_neg(p):
    return (p[0], ((-p[1][0]) % Q, (-p[1][1]) % Q))


def oracle_key(key):
    """the catalogue's key as oracle.summa_verifier.verify takes it"""
    return {"k": key["k"], "n_currencies": key["n_currencies"], "vk_digest": key["vk_digest"], "fixed_comms": list(key["fixed_comms"]),
            "permutation_comms": list(key["permutation_comms"]), "g2": key["g2"], "neg_s_g2": g2_neg(key["s_g2"])}


def project_key(key):
    """the catalogue's key as circuits_halo2_amd.verifier takes it: (verifier params: g2 / s_g2 as 128 Montgomery bytes, api.VerifyingKey)"""
    from types import SimpleNamespace
    from circuits_halo2_amd import api
    params = SimpleNamespace(g2=PR.g2_to_bytes(key["g2"]), s_g2=PR.g2_to_bytes(key["s_g2"]))
    vk = api.VerifyingKey(key["k"], key["n_currencies"], [tuple(c) for c in key["fixed_comms"]],
                          [tuple(c) for c in key["permutation_comms"]], key["vk_digest"])
    return params, vk


def _with(key, **changes):
    out = dict(key)
    out.update(changes)
    assert sorted(out) == sorted(key) and sorted(n for n in key if out[n] != key[n]) == sorted(changes), "exactly the named entries change"
    return out


def key_cases(proof, instances, key, flavour):
    out = []
    all_comms = [tuple(key[part][j]) for part, j in KEY_COMMITMENTS]
    assert all(PR.g1_is_on_curve(c) for c in all_comms)

    def add(kind, change, field):
        changed = change(key)
        assert changed != key and sorted(changed) == sorted(key)
        out.append(Case("%s-key-%s" % (flavour, kind), "key", proof, list(instances), change, True, field))

    def replace(part, j, point):
        def change(k_):
            comms = [tuple(c) for c in k_[part]]
            assert comms[j] != point and PR.g1_is_on_curve(point)
            comms[j] = point
            return _with(k_, **{part: comms})                         # the digest stays: nothing tells the transcript
        return change
    for at, (part, j) in enumerate(KEY_COMMITMENTS):
        c = all_comms[at]
        neighbour = next(all_comms[(at + d) % len(all_comms)] for d in range(1, len(all_comms)) if all_comms[(at + d) % len(all_comms)] != c)
        name = ("f%d" if part == "fixed_comms" else "sigma%d") % j
        for kind, point in (("neg", (c[0], Q - c[1])), ("gen", (1, 2)), ("neighbour", neighbour)):
            add("%s-%s" % (name, kind), replace(part, j, point), ("key", name))
    add("g2-s_g2-swapped", lambda k_: _with(k_, g2=k_["s_g2"], s_g2=k_["g2"]), ("key", "g2"))
    add("s_g2-negated", lambda k_: _with(k_, s_g2=g2_neg(k_["s_g2"])), ("key", "s_g2"))
    add("g2-is-s_g2", lambda k_: _with(k_, g2=k_["s_g2"]), ("key", "g2"))
    for other in (key["k"] - 1, key["k"] + 1):
        add("k%d" % other, (lambda o: lambda k_: _with(k_, k=o))(other), ("key", "k"))
    for other in (1, 3):
        assert other != key["n_currencies"]
        add("currencies%d" % other, (lambda o: lambda k_: _with(k_, n_currencies=o))(other), ("key", "n_currencies"))
    add("digest+1", lambda k_: _with(k_, vk_digest=(k_["vk_digest"] + 1) % R), ("key", "vk_digest"))
    return out


# ------------------------------------------------------------------ the catalogue
_GENERATORS = {"point": point_cases, "scalar": scalar_cases, "instance": instance_cases, "length": length_cases}


def catalogue(proof, instances, key, flavour, families=FAMILIES):
    """every case of the named families for one accepted proof; the ids are unique"""
    assert flavour in ("evm", "blake2b")
    proof = bytes(proof)
    out = []
    for family in families:
        out += key_cases(proof, instances, key, flavour) if family == "key" else _GENERATORS[family](proof, instances, flavour)
    assert len({c.id for c in out}) == len(out)
    return out


def golden_evm():
    """(proof, public inputs, key) of the reference's own shipped proof (k6_inclusion_proof_solidity_calldata.json)"""
    cd = json.load(open(os.path.join(GOLD, "k6_inclusion_proof_solidity_calldata.json")))
    return bytes.fromhex(cd["proof"][2:]), [H(x) for x in cd["public_inputs"]], reference_key_dict()


def groups(cases, size):
    """the cases in runs of `size` consecutive ones: what one parametrised test carries"""
    return [cases[i:i + size] for i in range(0, len(cases), size)]


def judge(case, key, flavour):
    """the oracle's verdict on a case -> (accepted, trace): the trace is filled iff the oracle got as far as the pairing"""
    trace = {}
    changed = case.key_change(key) if case.key_change else key
    ok = SV.verify(case.proof, case.instances, oracle_key(changed), trace, flavour=flavour)
    return ok, trace
