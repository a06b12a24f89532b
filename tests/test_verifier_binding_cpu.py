"""The restated verifier (oracle/summa_verifier.py) over the whole EVM catalogue of verifier_tamper_cases.py, on the reference's
own shipped proof (k6_inclusion_proof_solidity_calldata.json) under the key of k6_verifier_trace.json: the original is accepted,
every single-field change of the proof, its public inputs and its key is rejected without an exception, and a change that still
parses is rejected at the pairing (the trace is filled), not at the parser.  This is what lets the oracle be the judge of the
project's three verifiers in test_gpu_verifier_binding.py.  No GPU and no built library."""
import collections

import pytest

from oracle import summa_verifier as SV
import verifier_tamper_cases as TC

PROOF, INSTANCES, KEY = TC.golden_evm()
CASES = TC.catalogue(PROOF, INSTANCES, KEY, "evm")
PER_GROUP = {"point": 4, "scalar": 5, "instance": 4, "length": 60, "key": 3}      # fields (length: cases) per test: a few seconds each


def _groups():
    """[(test id, cases)]: each family cut into runs of whole fields, in catalogue order"""
    out = []
    for family in TC.FAMILIES:
        by_field = collections.OrderedDict()
        for n, c in enumerate(c for c in CASES if c.family == family):
            by_field.setdefault(c.field if c.field is not None else ("shape", n // PER_GROUP[family]), []).append(c)
        fields = list(by_field.values())
        for g, run in enumerate(TC.groups(fields, PER_GROUP[family])):
            out.append(("%s-%d" % (family, g), [c for cases in run for c in cases]))
    return out


GROUPS = _groups()


def test_the_original_is_accepted():
    trace = {}
    assert SV.verify(PROOF, INSTANCES, TC.oracle_key(KEY), trace) and trace["pairing_lhs_x"]


def test_every_case_is_in_one_group():
    assert sorted(c.id for _, cases in GROUPS for c in cases) == sorted(c.id for c in CASES)


@pytest.mark.parametrize("cases", [g[1] for g in GROUPS], ids=[g[0] for g in GROUPS])
def test_the_oracle_rejects_every_case(cases):
    """no exception, a rejection each; a proof or instance case that parses got as far as the pairing"""
    for c in cases:
        accepted, trace = TC.judge(c, KEY, "evm")
        assert accepted is False, c.id
        if c.family in ("point", "scalar", "instance"):
            assert ("pairing_lhs_x" in trace) == c.parses, c.id


def test_catalogue_covers_every_field_both_ways():
    """every one of the 16 points, 35 evaluations and 4 public inputs appears in a case that parses and in one that does not;
    every one of the 17 key commitments is negated, replaced by the generator and by a neighbour (the key is trusted input with
    no encoding of its own: its cases all parse); g2, s_g2, k, the currency count and the digest are each changed"""
    seen = collections.defaultdict(set)
    for c in CASES:
        if c.field is not None:
            seen[c.field].add(c.parses)
    for kind, count in (("point", TC.N_POINTS), ("scalar", TC.N_SCALARS), ("instance", len(INSTANCES))):
        assert (TC.N_POINTS, TC.N_SCALARS, len(INSTANCES)) == (16, 35, 4)
        for i in range(count):
            assert seen[(kind, i)] == {True, False}, (kind, i)
    key_ids = {c.id for c in CASES if c.family == "key"}
    names = ["f%d" % j for j in range(11)] + ["sigma%d" % j for j in range(6)]
    assert len(names) == 17
    for name in names:
        assert {"evm-key-%s-%s" % (name, kind) for kind in ("neg", "gen", "neighbour")} <= key_ids
        assert seen[("key", name)] == {True}
    for name in ("g2", "s_g2", "k", "n_currencies", "vk_digest"):
        assert seen[("key", name)] == {True}


def test_catalogue_ids_are_unique_and_the_counts_are_those_of_the_layout():
    assert len({c.id for c in CASES}) == len(CASES)
    count = collections.Counter(c.family for c in CASES)
    # 16 points x (3 + 6); 35 evaluations x (3 + 4); 4 inputs x 2 + 5 swaps of unequal inputs + 2 counts; 50 cuts + 3; 17 x 3 + 3 + 4 + 1
    assert count == {"point": 144, "scalar": 245, "instance": 15, "length": 53, "key": 59}


def test_every_case_changes_exactly_its_field():
    """restated outside the generators: outside the named field's bytes the proof is the original, inside it is not; instance and
    key cases keep the proof; length cases keep every byte they have"""
    for c in CASES:
        if c.family in ("point", "scalar"):
            kind, i = c.field
            off = TC.point_offset(i, "evm") if kind == "point" else TC.scalar_offset(i, "evm")
            size = 64 if kind == "point" else 32
            assert c.proof[:off] == PROOF[:off] and c.proof[off + size:] == PROOF[off + size:] and c.proof[off:off + size] != PROOF[off:off + size]
            assert c.instances == INSTANCES and c.key_change is None
        elif c.family == "length":
            assert len(c.proof) != len(PROOF) and c.instances == INSTANCES and c.key_change is None
        else:
            assert c.proof == PROOF and (c.instances != INSTANCES) == (c.family == "instance") and (c.key_change is not None) == (c.family == "key")
    cuts = {len(c.proof) for c in CASES if c.family == "length"}
    assert cuts == set(range(64, 0x380, 64)) | set(range(0x380, 0x7e0, 32)) | {0x7e0, 0x820, 0, 2145, 2176}


def test_every_evm_alias_of_the_golden_proof_fits_its_word():
    """nothing is left out for the EVM flavour: x + q, y + q and v + r of every field fit 256 bits and are in the catalogue"""
    ids = {c.id for c in CASES}
    for name in TC.POINT_NAMES:
        assert {"evm-point-%s-%s" % (name, kind) for kind in ("neg", "gen", "next", "x+q", "y+q", "x+mq", "zero", "y=0", "x=q")} <= ids
    for name in TC.SCALAR_NAMES:
        assert {"evm-scalar-%s-%s" % (name, kind) for kind in ("+1", "r-v", "zero", "v+r", "v+mr", "r", "ones")} <= ids
