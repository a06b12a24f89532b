"""tests/stream_cases.py without a GPU: the table covers every entry point of include/summa_gpu.h that takes a stream, and every
row could fail -- by the oracle alone, the result for the real inputs differs from the result for the decoy in every output row,
neither holds a row of the 0x5A the output buffers start with, and the shapes reach the paths the table claims."""
import os

import numpy as np
import pytest

import ntt_cases
import stream_cases as sc
from conftest import ROOT

HEADER = open(os.path.join(ROOT, "include", "summa_gpu.h")).read()
NAMES = [r.name for r in sc.ROWS]


def test_every_entry_point_with_a_stream_is_a_row_or_a_named_exemption():
    """a prototype with a `void* stream` parameter that is neither a row nor exempt, or a row whose function the header lacks,
    fails here: no entry point is added without its ordering being tested"""
    entries = sc.header_stream_entries(HEADER)
    assert len(entries) == len(set(entries)) >= 60
    in_rows = {r.entry for r in sc.ROWS}
    missing = [e for e in entries if e not in in_rows and e not in sc.EXEMPT]
    assert not missing, f"entry points with a stream parameter and no row in tests/stream_cases.py: {missing}"
    unknown = sorted(in_rows - set(entries))
    assert not unknown, f"rows that name no stream-taking prototype of the header: {unknown}"
    for name, reason in sc.EXEMPT.items():
        assert name not in in_rows and reason and f" {name}(" in HEADER, name
    assert len(NAMES) == len(set(NAMES))


def test_the_parser_finds_a_new_prototype():
    text = HEADER.replace("#ifdef __cplusplus\n}", "int sg_new_thing_dev(const void* d_in,\n    void* d_out, void* stream);\n#ifdef __cplusplus\n}", 1)
    assert "sg_new_thing_dev" in sc.header_stream_entries(text) and "sg_new_thing_dev" not in sc.header_stream_entries(HEADER)
    assert "sg_time_ntt_dev" not in sc.header_stream_entries(HEADER) and "sg_stream_wait" in sc.header_stream_entries(HEADER)


def test_only_entries_without_a_result_are_exempt():
    assert set(sc.EXEMPT) == {"sg_stream_wait", "sg_time_ntt_dev"}


# every build the GPU module runs: seeds 0 and 1 of every row (two streams), seeds 2 and 3 of the rows that are interleaved on two
# streams, and the cold builds (seeds 2 and 3) of the rows that cache something
BUILDS = [(r.name, seed, False) for r in sc.ROWS for seed in ((0, 1, 2, 3) if r.per_stream else (0, 1))]
BUILDS += [(r.name, seed, True) for r in sc.ROWS if r.caches for seed in (2, 3)]


@pytest.mark.parametrize("name,seed,cold", BUILDS, ids=[f"{n}-{s}{'-cold' if c else ''}" for n, s, c in BUILDS])
def test_real_and_decoy_cannot_be_mistaken(name, seed, cold):
    case = sc.built(name, seed, cold)
    real, decoy = case.want("real"), case.want("decoy")
    names = set(case.output_names()) | ({"host"} if "host" in real else set())
    assert set(real) == set(decoy) == names and names, (sorted(real), sorted(names))
    pairs = list(case.ins.values()) + list(case.host_ins.values())
    for pair in pairs:
        assert pair[0].shape == pair[1].shape and pair[0].dtype == pair[1].dtype
    assert not pairs or any(not np.array_equal(a, b) for a, b in pairs)      # (offsets of one layout, shared usernames: some pairs agree)
    assert set(case.inout) <= set(case.ins) and not set(case.outs) & set(case.ins) and set(case.fixed) <= names and set(case.aux) <= names
    assert case.ins or case.host_ins or case.outs, "a row with nothing to order"
    for out in sorted(names):
        r, d = sc.rows_of(real[out]), sc.rows_of(decoy[out])
        assert r.shape == d.shape, out
        if out in case.outs:
            assert real[out].size == case.outs[out], out
        elif out in case.inout:
            assert real[out].size == case.ins[out][0].size, out
        for w, what in ((r, "real"), (d, "decoy")):
            if what == "decoy" and name == "fr_flag_noncanonical":
                continue                     # the decoy's flag is the untouched buffer, by the entry's definition
            stale = (w == sc.FILL).all(axis=1)
            assert not stale.any(), f"{out}: the {what} result holds a row of 0x5A at {int(np.argmax(stale))}"
        same = (r == d).all(axis=1)
        if out in case.aux or not (case.ins or case.host_ins):      # (no caller's buffer goes in: one result, checked below)
            continue
        if out in case.blocks:                                       # most cells fixed by a floor plan: every block holds a row that differs
            per_block = same.reshape(case.blocks[out], -1)
            assert not per_block.all(axis=1).any(), f"{out}: real and decoy agree in all of block {int(np.argmax(per_block.all(axis=1)))}"
            continue
        allowed = sorted(case.fixed.get(out, []))
        assert sorted(np.flatnonzero(same).tolist()) == allowed, f"{out}: real and decoy agree at rows {np.flatnonzero(same)[:8]}, allowed {allowed}"
    if not case.ins and not case.host_ins:
        assert np.array_equal(np.concatenate([real[o] for o in sorted(names)]), np.concatenate([decoy[o] for o in sorted(names)]))


def test_different_seeds_give_different_real_inputs():
    """the rows that run on two streams at once take four seeds, 0 and 2 on one stream and 1 and 3 on the other, and the cold
    builds take two: each call's result must be its own"""
    import itertools
    for r in sc.ROWS:
        sets = ([[sc.built(r.name, seed) for seed in range(4)]] if r.per_stream else []) + ([[sc.built(r.name, seed, True) for seed in (2, 3)]] if r.caches else [])
        for cases in sets:
            for a, b in itertools.combinations(cases, 2):
                if not (a.ins or a.host_ins):
                    continue
                for out in a.want():
                    if out not in a.aux:
                        assert not np.array_equal(a.want()[out], b.want()[out]), (r.name, out)


def test_the_shapes_reach_the_paths_the_table_claims():
    # batched launches on the caller's stream up to 2^18, the two batch streams above (csrc/ntt_plan.h through ntt_cases)
    for logs in (sc.BATCH_LOGS, sc.BATCH_COLD):
        assert logs["caller"] <= ntt_cases.BATCHED_MAX_LOG < logs["batch streams"]
    assert sc.BATCH_LOGS["batch streams"] == ntt_cases.BATCHED_MAX_LOG + 1 == ntt_cases.NARROWED_K, "the first size on the batch streams"
    assert sc.BATCH_VECTORS == 3 <= ntt_cases.BATCH_MAX, "three vectors: stream 0's half of the scratch is used twice"
    # multi-pass plans (a scratch vector per transform: on the batch streams the halves of the lane's scratch, used by vectors 0
    # and 2 one after the other) at every batched size, warm and cold; one pass at 2^10
    for log_n in (*sc.BATCH_LOGS.values(), *sc.BATCH_COLD.values()):
        assert ntt_cases.factor(11, 9, log_n)[0] > 1, log_n
    assert ntt_cases.factor(11, 9, sc.K)[0] == 1
    # each of the two batch entries has a row at each of the two sizes
    for entry, out_of_place in (("sg_ntt_fr_batch_dev", False), ("sg_ntt_fr_batch_oop_dev", True)):
        rows = [r for r in sc.ROWS if r.entry == entry]
        sizes = sorted({a[0].size for r in rows for a in sc.built(r.name).ins.values()})
        assert sizes == sorted(32 << log_n for log_n in sc.BATCH_LOGS.values()) and len(rows) == 2, entry
        assert all(len(sc.built(r.name).ins) == sc.BATCH_VECTORS and bool(sc.built(r.name).outs) == out_of_place for r in rows), entry
    # the batch rows as fused jobs, with the library's own limits (csrc/msm_plan.h) under each row's parameters: at least three
    # groups, so both engines run and so does the finish path of a third group and later
    assert (sc.max_fused(sc.N), sc.max_fused(sc.N // 2), sc.max_fused(sc.N, 16), sc.max_fused_fixed(sc.N, sc.N, 16)) == (64, 64, 1, 2)
    want = {"msm_g1_batch": [(0, 2), (2, 1), (3, 1), (4, 1)], "commit_batch": [(0, 2), (2, 2), (4, 1)], "commit_batch_mixed": [(0, 1), (1, 1), (2, 1), (3, 1), (4, 1)]}
    for name in sc.BATCH_ROWS:
        lengths, fixed, groups = sc.row_groups(name)
        assert groups == want[name] and len(groups) >= 3 and len(lengths) == 5 and fixed == (name == "commit_batch"), name
    assert sc.fused_groups([sc.N] * sc.COMMIT_JOBS) == [(0, 5)], "without the parameter five columns of 2^10 are ONE job"
    assert {r.entry for r in sc.ROWS if r.name in sc.BATCH_ROWS} == {"sg_msm_g1_batch_dev", "sg_commit_batch_dev", "sg_commit_batch_mixed_dev"}
    assert sc.N > 64, "above msm.tiny_max"
    assert sorted(set(sc.MIXED_BASES)) == [0, 1], "coefficient and Lagrange columns in one call"
    # the cold sizes are nobody else's
    warm = {sc.K, sc.K + sc.EXT, sc.K + sc.NUM_EXT, 8, *sc.BATCH_LOGS.values()}
    assert not warm & {sc.K_COLD, sc.K_COLD + sc.EXT, *sc.BATCH_COLD.values()}
    for r in sc.ROWS:
        if r.caches and r.entry.startswith(("sg_ntt", "sg_intt", "sg_lagrange", "sg_coeff", "sg_extended", "sg_divide", "sg_cosets", "sg_kzg")):
            cold, warm_case = sc.built(r.name, 2, True), sc.built(r.name)
            sizes = lambda c: sorted(a[0].size for a in c.ins.values()) + sorted(c.outs.values())
            assert sizes(cold) != sizes(warm_case), r.name
    assert sum(1 for r in sc.ROWS if r.per_stream) >= 5 and {"ntt", "fr_lincomb_sets", "fr_kate_division_batch", "lookup_permute_async"} <= {r.name for r in sc.ROWS if r.per_stream}


def test_the_group_rule_is_commit_plans():
    """consecutive equal lengths fuse, up to the limit: the cases tests/test_commit_plan_cpu.py pins on csrc/commit_plan.h"""
    assert sc.fused_groups([4, 4, 4, 2, 4], lambda n: 64) == [(0, 3), (3, 1), (4, 1)]
    assert sc.fused_groups([4, 4, 4, 4, 4], lambda n: 2) == [(0, 2), (2, 2), (4, 1)]
    assert sc.fused_groups([]) == []
    assert len(sc.fused_groups([1 << 10] * 130)) == 3, "the library's limit of 64 to a job is the default"
