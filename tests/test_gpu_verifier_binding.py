"""The project's three verifiers -- verifier.verify_proof(driver="python"), driver="native" (sp_verify_proof) and verifier.verify_batch
(sv_verify_batch) -- over the catalogue of verifier_tamper_cases.py: every single change of a proof field, a public input, a length,
a key commitment, g2 / s_g2, k, the currency count or the digest is a rejection (False, never an exception), in both transcript
flavours: the golden k = 11 EVM proof under the reference's key, and one k = 9 Blake2b proof made here.  The expected verdict is the
catalogue's (all reject), judged by oracle/summa_verifier.py (test_verifier_binding_cpu.py for the EVM catalogue, here for Blake2b).

A single-field change before the last challenge is refused by Fiat-Shamir alone for a verifier that absorbs what it reads.  The
teeth of this file are the aliases (x + q, y + q, v + r, flag bits, instance words + r at the C ABI: a reader that reduces before it
absorbs would accept a second byte string), W' (read after the last challenge: only the pairing binds it) and the key / params
family (never absorbed: bound by a coefficient of the final ~37-point MSM alone).  What makes the per-field sweep meaningful is
`test_rejected_for_the_right_reason`: for every case that still parses, the twin's terms summed by the device MSM are the
oracle's pairing input for the same tampered bytes, point for point -- the twin draws the oracle's challenges from every field and
rejects at the pairing, not by accident at the parser.  `test_a_mutant_*` shows the catalogue catches a verifier that is wrong."""
import ctypes as C

import numpy as np
import pytest

import verifier_tamper_cases as TC
import verify_batch_cases as VC

pytestmark = pytest.mark.gpu
FLAVOURS = ("evm", "blake2b")
# the Blake2b proof's blinding seed (test_gpu_prover.seeded_rng), and how many of its 16 points have an x + q that fits the 254
# bits of a compressed point (about a third do; at least 3 are required, only those carry the "x+q" case)
BLAKE2B_SEED, BLAKE2B_X_ALIASES = 1, 7
A_GROUPS = {"point": 6, "scalar": 12, "instance": 2, "length": 1, "key": 8}       # tests per family: a few seconds each
D_GROUPS = {"point": 6, "scalar": 12, "instance": 2}
BATCH_CASES = 96                                                                   # + a good proof after every third: 128 proofs a call


class Context:
    """one accepted proof, its key in both forms, its catalogue, and the oracle's verdicts (each case judged once)"""

    def __init__(self, flavour, proof, instances, key, params, vk, goldens):
        self.flavour, self.proof, self.instances, self.key, self.params, self.vk, self.goldens = flavour, proof, instances, key, params, vk, goldens
        self.cases = TC.catalogue(proof, instances, key, flavour)
        self.judged = {}

    def judge(self, case):
        if case.id not in self.judged:
            self.judged[case.id] = TC.judge(case, self.key, self.flavour)
        return self.judged[case.id]

    def keyed(self, case):
        """(params, vk) the case is verified under"""
        return TC.project_key(case.key_change(self.key)) if case.key_change else (self.params, self.vk)

    def group(self, family, g, of, only_parsing=False):
        cases = [c for c in self.cases if c.family == family and (c.parses or not only_parsing)]
        return cases[len(cases) * g // of:len(cases) * (g + 1) // of]


def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from circuits_halo2_amd import ffi
    ffi.check(ffi.lib().sg_init(0))


def _evm_context():
    params, vk = VC.reference_key()
    proof, instances, key = TC.golden_evm()
    twin_params, twin_vk = TC.project_key(key)          # the catalogue's key is the reference's, in both forms
    assert bytes(params.g2) == twin_params.g2 and bytes(params.s_g2) == twin_params.s_g2
    assert (vk.k, vk.n_currencies, vk.transcript_repr) == (twin_vk.k, twin_vk.n_currencies, twin_vk.transcript_repr)
    assert [tuple(c) for c in vk.fixed_comms + vk.permutation_comms] == twin_vk.fixed_comms + twin_vk.permutation_comms
    assert VC.golden_proofs()[0] == (proof, instances)
    return Context("evm", proof, instances, key, params, vk, VC.golden_proofs()), params


def _blake2b_context():
    import test_gpu_prover as TP
    from circuits_halo2_amd import api, prover as P
    s = TP.make_setup(9)
    advice = [s["dev"](c) for c in s["asg"]["advice"]]
    instances = [int(v) for v in s["asg"]["instances"]]
    proof = P.create_proof(s["params"], s["pk"], advice, instances, TP.seeded_rng(BLAKE2B_SEED), transcript=P.Blake2bWrite())
    pk = s["pk"]
    key = {"k": 9, "n_currencies": 2, "vk_digest": int(pk.vk_digest), "fixed_comms": [tuple(c) for c in pk.fixed_comms],
           "permutation_comms": [tuple(c) for c in pk.permutation_comms], "g2": s["vk"]["g2"], "s_g2": TC.g2_neg(s["vk"]["neg_s_g2"])}
    vk = api.VerifyingKey(9, 2, key["fixed_comms"], key["permutation_comms"], key["vk_digest"])
    twin_params, _ = TC.project_key(key)
    assert bytes(s["params"].g2) == twin_params.g2 and bytes(s["params"].s_g2) == twin_params.s_g2
    return Context("blake2b", proof, instances, key, s["params"], vk, [(proof, instances)]), s["params"]


@pytest.fixture(scope="module")
def contexts():
    """flavour -> Context, each built when first asked for"""
    _gpu()
    built, to_free = {}, []

    def get(flavour):
        if flavour not in built:
            built[flavour], params = (_evm_context if flavour == "evm" else _blake2b_context)()
            to_free.append(params)
        return built[flavour]
    yield get
    for params in to_free:
        params.free()


def _single(ctx, case, driver):
    from circuits_halo2_amd import verifier as V
    params, vk = ctx.keyed(case)
    return V.verify_proof(params, vk, case.proof, case.instances, ctx.flavour, driver=driver)


# ------------------------------------------------------------------ the originals
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_the_original_is_accepted_by_the_oracle_and_all_three_verifiers(contexts, flavour):
    from circuits_halo2_amd import verifier as V
    ctx = contexts(flavour)
    assert len(ctx.proof) == TC.proof_length(flavour)
    ok, trace = TC.judge(TC.Case("original", "none", ctx.proof, ctx.instances, None, True, None), ctx.key, flavour)
    assert ok is True and "pairing_lhs_x" in trace
    for driver in ("python", "native"):
        assert V.verify_proof(ctx.params, ctx.vk, ctx.proof, ctx.instances, flavour, driver=driver) is True, driver
    stats = {}
    assert V.verify_batch(ctx.params, ctx.vk, [ctx.proof], [ctx.instances], flavour, stats=stats) == [True] and stats == {"pairings": 1}


def test_the_blake2b_catalogue_keeps_at_least_three_x_aliases(contexts):
    """x + q fits a compressed point's 254 bits for about a third of all points: the fixed seed's proof has the recorded number"""
    ctx = contexts("blake2b")
    fit = TC.x_plus_q_points(ctx.proof)
    print("blake2b points with an x + q alias:", len(fit), [TC.POINT_NAMES[i] for i in fit])
    assert len(fit) >= 3 and len(fit) == BLAKE2B_X_ALIASES
    assert sum(c.id.endswith("-x+q") for c in ctx.cases if c.family == "point") == len(fit)
    import collections
    print("cases:", dict(collections.Counter(c.family for c in ctx.cases)))


# ------------------------------------------------------------------ (a) the single-proof verifiers, (e) judged by the oracle first
@pytest.mark.parametrize("flavour,family,g", [(fl, fam, g) for fl in FLAVOURS for fam in TC.FAMILIES for g in range(A_GROUPS[fam])])
def test_both_single_proof_verifiers_reject_every_case(contexts, flavour, family, g):
    """False from the Python twin and from sp_verify_proof for every case, and no exception.  The Blake2b catalogue is made here, so
    the oracle judges it here first (the EVM one: test_verifier_binding_cpu.py): a case the oracle accepted would be a finding
    about the oracle"""
    ctx = contexts(flavour)
    cases = ctx.group(family, g, A_GROUPS[family])
    assert cases
    for c in cases:
        if flavour == "blake2b":
            accepted, trace = ctx.judge(c)
            assert accepted is False, ("oracle", c.id)
            if c.family in ("point", "scalar", "instance"):
                assert ("pairing_lhs_x" in trace) == c.parses, c.id
        for driver in ("python", "native"):
            assert _single(ctx, c, driver) is False, (driver, c.id)


# ------------------------------------------------------------------ (b) the batch verifier
def _batches(ctx, cases):
    """[(proofs, instances, want)]: runs of at most BATCH_CASES cases, a good proof after every third one"""
    out = []
    for run in TC.groups(cases, BATCH_CASES):
        proofs, insts, want = [], [], []
        for n, c in enumerate(run):
            proofs.append(c.proof), insts.append(list(c.instances)), want.append(False)
            if n % 3 == 2:
                good = ctx.goldens[(n // 3) % len(ctx.goldens)]
                proofs.append(good[0]), insts.append(list(good[1])), want.append(True)
        out.append((proofs, insts, want))
    return out


@pytest.mark.parametrize("flavour,family", [(fl, fam) for fl in FLAVOURS for fam in ("point", "scalar", "instance", "length")])
def test_the_batch_verifier_finds_exactly_the_cases(contexts, flavour, family):
    """all of a family's cases in batches of at most 128 with good proofs between them: good ones true, cases false, and the pairing
    checks within 1 + 2 |bad| ceil(log2 n)"""
    from circuits_halo2_amd import verifier as V
    ctx = contexts(flavour)
    cases = [c for c in ctx.cases if c.family == family]
    seen = 0
    for proofs, insts, want in _batches(ctx, cases):
        n, bad = len(proofs), want.count(False)
        assert n <= 128 and (want.count(True) == bad // 3)
        stats = {}
        got = V.verify_batch(ctx.params, ctx.vk, proofs, insts, flavour, stats=stats)
        assert got == want, [i for i in range(n) if got[i] != want[i]]
        print(flavour, family, "proofs:", n, "bad:", bad, "pairings:", stats["pairings"], "bound:", VC.pairing_bound(n, bad))
        assert stats["pairings"] <= VC.pairing_bound(n, bad)
        seen += bad
    assert seen == len(cases)


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_the_batch_verifier_under_every_changed_key(contexts, flavour):
    """three good proofs under a changed key: all three rejected, for each key case"""
    from circuits_halo2_amd import verifier as V
    ctx = contexts(flavour)
    good = [ctx.goldens[i % len(ctx.goldens)] for i in range(3)]
    proofs, insts = [p for p, _ in good], [list(i) for _, i in good]
    assert V.verify_batch(ctx.params, ctx.vk, proofs, insts, flavour) == [True] * 3
    cases = [c for c in ctx.cases if c.family == "key"]
    assert len(cases) == 59
    for c in cases:
        params, vk = ctx.keyed(c)
        assert V.verify_batch(params, vk, proofs, insts, flavour) == [False] * 3, c.id


# ------------------------------------------------------------------ (c) instance aliases at the C ABI
def test_instance_words_plus_r_are_rejected_at_the_c_abi(contexts):
    """the Montgomery word of a public input plus r (and plus the largest multiple of r that fits) denotes the same field element;
    the Python wrappers cannot produce it.  sp_verify_proof and sv_verify_batch answer rc == 0, accepted == 0"""
    from circuits_halo2_amd import ffi, verifier as V
    ctx = contexts("evm")
    L = ffi.verifier_lib()
    digest, fixed, perm, g2, s_g2 = V._native_key(ctx.params, ctx.vk)
    raw = np.frombuffer(ctx.proof, dtype=np.uint8).copy()
    words = [int.from_bytes(V._fr_bytes(v), "little") for v in ctx.instances]
    column = lambda ws: np.frombuffer(b"".join(w.to_bytes(32, "little") for w in ws), dtype=np.uint8).copy()

    def single(ws):
        inst, ok = column(ws), C.c_int(7)
        rc = L.sp_verify_proof(C.c_uint32(ctx.vk.k), C.c_uint32(ctx.vk.n_currencies), ffi.ptr(digest), ffi.ptr(fixed), ffi.ptr(perm), ffi.ptr(g2),
                               ffi.ptr(s_g2), ffi.ptr(raw), C.c_size_t(len(ctx.proof)), ffi.ptr(inst), C.c_uint32(len(ws)), C.c_int(0), C.byref(ok))
        return rc, ok.value

    def batch(columns):
        n = len(columns)
        insts = [column(ws) for ws in columns]
        accepted, pairings = np.full(n, 7, dtype=np.uint8), C.c_uint32(0)
        rc = L.sv_verify_batch(C.c_uint32(ctx.vk.k), C.c_uint32(ctx.vk.n_currencies), ffi.ptr(digest), ffi.ptr(fixed), ffi.ptr(perm), ffi.ptr(g2),
                               ffi.ptr(s_g2), (C.c_void_p * n)(*[raw.ctypes.data] * n), (C.c_size_t * n)(*[len(ctx.proof)] * n),
                               (C.c_void_p * n)(*[a.ctypes.data for a in insts]), (C.c_uint32 * n)(*[len(ws) for ws in columns]), C.c_uint32(n),
                               C.c_int(0), None, ffi.ptr(accepted), C.byref(pairings))
        return rc, accepted.tolist()
    assert single(words) == (0, 1) and batch([words] * 3) == (0, [1, 1, 1])
    aliases = []
    for i, w in enumerate(words):
        m = ((1 << 256) - 1 - w) // TC.R
        assert w < TC.R and m >= 2
        for alias in (w + TC.R, w + m * TC.R):
            assert alias % TC.R == w and alias < 1 << 256
            aliases.append(words[:i] + [alias] + words[i + 1:])
    aliases.append([w + TC.R for w in words])
    for ws in aliases:
        assert single(ws) == (0, 0), ws
        assert batch([words, ws, words]) == (0, [1, 0, 1]), ws
    assert batch(aliases[:8]) == (0, [0] * 8)


# ------------------------------------------------------------------ (d) rejected for the right reason
@pytest.mark.parametrize("flavour,family,g", [(fl, fam, g) for fl in FLAVOURS for fam in sorted(D_GROUPS) for g in range(D_GROUPS[fam])])
def test_rejected_for_the_right_reason(contexts, flavour, family, g):
    """every proof / instance case that still parses: the twin's terms (verifier.proof_terms) through the device MSM the verifier
    itself uses (best_multiexp: the tiny-MSM path) are the oracle's left pairing input on the same tampered input, and the twin's W'
    is the oracle's right one.  So the twin drew the oracle's challenges from every field, and its rejection is the pairing's"""
    from conftest import fr_np, point_np
    from circuits_halo2_amd import verifier as V
    from circuits_halo2_amd.arithmetic import best_multiexp
    ctx = contexts(flavour)
    cases = ctx.group(family, g, D_GROUPS[family], only_parsing=True)
    assert cases
    for c in cases:
        accepted, trace = ctx.judge(c)
        assert accepted is False and "pairing_lhs_x" in trace, c.id
        terms = V.proof_terms(ctx.vk, c.proof, c.instances, flavour)
        assert terms is not None, c.id
        points, scalars, w2 = terms
        assert len(points) == len(scalars) <= 64
        got = best_multiexp(fr_np(scalars), np.concatenate([point_np(p) for p in points]))
        assert (got == point_np((trace["pairing_lhs_x"], trace["pairing_lhs_y"]))).all(), c.id
        assert w2 == (trace["pairing_rhs_x"], trace["pairing_rhs_y"]), c.id


def test_the_right_reason_covers_every_parsing_case(contexts):
    """the groups above are all of the parsing proof / instance cases: 16 x 3 points, 35 x 3 evaluations, the public inputs' 11"""
    ctx = contexts("evm")
    for family, count in (("point", 48), ("scalar", 105), ("instance", 11)):
        got = [c.id for g in range(D_GROUPS[family]) for c in ctx.group(family, g, D_GROUPS[family], only_parsing=True)]
        assert len(got) == len(set(got)) == count
    for family in TC.FAMILIES:
        got = [c.id for g in range(A_GROUPS[family]) for c in ctx.group(family, g, A_GROUPS[family])]
        assert got == [c.id for c in ctx.cases if c.family == family]


# ------------------------------------------------------------------ (f) teeth: mutants of the Python twin
def _accepted_by_twin(ctx, cases):
    return [c.id for c in cases if _single(ctx, c, "python")]


def test_a_mutant_that_reduces_scalars_before_absorbing_is_caught(contexts, monkeypatch):
    """_Reader.read_scalar without the range check, reducing mod r before the absorb: the original still verifies, and so does a
    second byte string -- the v + r alias of an evaluation.  The catalogue's verdict (reject) fails such a reader"""
    from circuits_halo2_amd import verifier as V
    ctx = contexts("evm")

    def read_scalar(self):
        v = int.from_bytes(self._take(32), "big" if self.evm else "little") % V.R
        self.tr.common_scalar(v)
        return v
    aliases = [c for c in ctx.cases if c.family == "scalar" and c.id.endswith(("-v+r", "-v+mr"))][:6]
    assert _accepted_by_twin(ctx, aliases) == []
    monkeypatch.setattr(V._Reader, "read_scalar", read_scalar)
    assert V.verify_proof(ctx.params, ctx.vk, ctx.proof, ctx.instances, "evm", driver="python") is True
    assert _accepted_by_twin(ctx, aliases) == [c.id for c in aliases]


def test_a_mutant_that_reduces_coordinates_before_the_curve_check_is_caught(contexts, monkeypatch):
    """the EVM read_point reducing x and y mod q before the curve check and the absorb accepts the x + q and y + q aliases"""
    from circuits_halo2_amd import verifier as V
    ctx = contexts("evm")
    original = V._Reader.read_point

    def read_point(self):
        if not self.evm:
            return original(self)
        raw = self._take(64)
        p = (int.from_bytes(raw[:32], "big") % V.Q, int.from_bytes(raw[32:], "big") % V.Q)
        if not V._on_curve(p):
            raise ValueError("commitment not on the curve")
        self.tr.common_point(p)
        return p
    aliases = [c for c in ctx.cases if c.family == "point" and c.id.endswith(("-x+q", "-y+q", "-x+mq"))]
    aliases = aliases[:6] + aliases[-3:]                              # the first two points and W'
    assert _accepted_by_twin(ctx, aliases) == []
    monkeypatch.setattr(V._Reader, "read_point", read_point)
    assert V.verify_proof(ctx.params, ctx.vk, ctx.proof, ctx.instances, "evm", driver="python") is True
    assert _accepted_by_twin(ctx, aliases) == [c.id for c in aliases]


def test_a_mutant_that_does_not_bind_a_key_commitment_is_caught(contexts, monkeypatch):
    """a proof_terms whose term for the fixed commitment f7 does not come from the key it is given (it keeps the reference key's f7)
    accepts the original and every key case that changes f7 alone: nothing but that term binds a key commitment.

    (Forcing f7's coefficient to 0 and removing its share c * f7(x) from r_eval is no such mutant: the proof's W and W' open f7 with
    the rest, so that verifier rejects the ORIGINAL -- checked with Python integers on the golden proof.  A verifier that ignores the
    key's f7 has to keep a correct term for it, as this one does.)"""
    from circuits_halo2_amd import api, verifier as V
    ctx = contexts("evm")
    original = V.proof_terms
    f7 = tuple(ctx.vk.fixed_comms[7])

    def proof_terms(vk, proof, instances, flavour):
        fixed = list(vk.fixed_comms)
        fixed[7] = f7
        return original(api.VerifyingKey(vk.k, vk.n_currencies, fixed, vk.permutation_comms, vk.transcript_repr), proof, instances, flavour)
    cases = [c for c in ctx.cases if c.family == "key"]
    mine = [c for c in cases if c.field == ("key", "f7")]
    assert len(mine) == 3 and _accepted_by_twin(ctx, mine) == []
    monkeypatch.setattr(V, "proof_terms", proof_terms)
    assert V.verify_proof(ctx.params, ctx.vk, ctx.proof, ctx.instances, "evm", driver="python") is True
    assert _accepted_by_twin(ctx, mine) == [c.id for c in mine]
    others = [c for c in cases if c.field in (("key", "f6"), ("key", "f8"), ("key", "s_g2"))]
    assert len(others) == 7 and _accepted_by_twin(ctx, others) == []
