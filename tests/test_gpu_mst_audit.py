"""The range audit on the device (csrc/mst_audit.cuh through ss_mst_range_audit_dev, DeviceMerkleSumTree.range_audit /
explain_unprovable and prove_batch(audit=...)) against the integer model of mst_audit_cases.py: flags, masks, the ordered list
and all four summary words, compared exactly.  The synthetic cases upload level-major sums mod r in Montgomery form -- the audit
reads balances only, so no hash is needed -- at the depths of mst_audit_cases.DEPTHS (block edges), at depth 11 (several tiles of
the list's scan) and at GROUPS_DEPTH = 15: 2^15 leaves are 512 tiles of 64, more than the 256 tile counts one workgroup of the
groups step scans, so the second group's places depend on the first group's total.  Sparse trees at depths 16, 20 and 21, against
the numpy model over their non-zero nodes, have 4, 64 and 128 such groups: the scatter's wave sums 64 group totals a trip of its
loop, so every lane and shuffle step carries data at 64 and the second trip runs at 128.  And 5, 33, 63 and 64 currencies put a
node's bits of the flags kernel's bit string across a word's edge, or exactly on it."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN

import mst_audit_cases as cases
import witness_cases as wc

pytestmark = pytest.mark.gpu

OVERFLOW, PLAIN = os.path.join(GOLDEN, "entry_16_overflow.csv"), os.path.join(GOLDEN, "entry_16.csv")
OVERFLOW_MASKS = [0b00001, 0b00010] + [0b00100] * 2 + [0b01000] * 4 + [0b10000] * 8
UNWRITTEN = 0x7FFFFFFF


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    from circuits_halo2_amd import ffi
    ffi.check(ffi.lib().sg_init(0))
    return ffi


def run_abi(ffi, d_bal, depth, nc, n_bytes, cap, stream=None):
    """ss_mst_range_audit_dev over the device array d_bal -> the shape of cases.model; cap None: room for every leaf, cap 0: a
    null list.  The list's buffer has two spare entries and starts as UNWRITTEN: what lies behind the listed leaves must stay."""
    import torch
    S = ffi.snapshot_lib()
    leaves = 1 << depth
    bad_cap = leaves if cap is None else cap
    size = C.c_uint64(0)
    ffi.check(S.ss_mst_range_audit_scratch(depth, C.byref(size)))
    d_flags = torch.full((2 * leaves - 1,), 0xEE, dtype=torch.uint8, device="cuda")
    d_masks = torch.full((leaves,), UNWRITTEN, dtype=torch.int32, device="cuda")
    d_bad = torch.full((bad_cap + 2,), UNWRITTEN, dtype=torch.int32, device="cuda")
    d_scratch = torch.full((size.value // 4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    summary = (C.c_uint64 * 4)()
    torch.cuda.current_stream().synchronize()                  # the fills above ran on the current stream
    ffi.check(S.ss_mst_range_audit_dev(ffi.dev_ptr(d_bal), depth, nc, n_bytes, ffi.dev_ptr(d_flags), ffi.dev_ptr(d_masks),
                                       ffi.dev_ptr(d_bad) if bad_cap else None, bad_cap, ffi.dev_ptr(d_scratch), summary,
                                       C.c_void_p(stream.cuda_stream) if stream is not None else ffi.current_stream_ptr()))
    bad = d_bad.cpu().tolist()
    listed = int(summary[2])
    assert all(x == UNWRITTEN for x in bad[listed:]), "entries behind the listed leaves were written"
    return {"flags": d_flags.cpu().tolist(), "masks": d_masks.cpu().tolist(), "bad": bad[:listed], "summary": list(summary),
            "tensors": (d_flags, d_masks, d_bad)}


def check(ffi, levels, n_bytes, caps, what):
    import torch
    depth, nc = len(levels) - 1, len(levels[0][0])
    d_bal = torch.from_numpy(cases.mont_bytes(cases.level_major(levels))).cuda()
    for cap in caps:
        want = cases.model(levels, n_bytes, (1 << depth) if cap is None else cap)
        got = run_abi(ffi, d_bal, depth, nc, n_bytes, cap)
        for key in ("summary", "bad", "masks", "flags"):
            assert got[key] == want[key], (what, cap, key)


@pytest.mark.parametrize("nc", cases.CURRENCIES)
@pytest.mark.parametrize("depth", cases.DEPTHS)
def test_synthetic_trees_agree_with_the_model(gpu, depth, nc):
    for n_bytes in cases.N_BYTES:
        for name, plant, caps in cases.plants(depth, nc, n_bytes):
            check(gpu, cases.planted(depth, nc, n_bytes, plant), n_bytes, caps, (name, depth, nc, n_bytes))


@pytest.mark.parametrize("nc,n_bytes", [(2, 8), (3, 5)])
def test_the_tile_counts_span_two_groups_of_the_prefix_step(gpu, nc, n_bytes):
    depth = cases.GROUPS_DEPTH
    assert (1 << depth) // cases.TILE == 2 * cases.GROUP
    for name, plant, caps in cases.plants(depth, nc, n_bytes):
        if name in ("edges", "every leaf", "last leaf"):
            check(gpu, cases.planted(depth, nc, n_bytes, plant), n_bytes, caps[:3], (name, depth, nc, n_bytes))


@pytest.mark.parametrize("nc", cases.MANY_CURRENCIES)
@pytest.mark.parametrize("depth", cases.MANY_DEPTHS)
def test_the_bit_gather_at_many_currencies_agrees_with_the_model(gpu, depth, nc):
    """a node's nc bits out of the workgroup's bit string: fields that straddle a word of it with up to 63 bits on either side
    (nc = 5, 33, 63) and the aligned one that skips the mask (nc = 64), flags up to 64, a partial last block"""
    for n_bytes in cases.MANY_N_BYTES:
        for name, plant, caps in cases.plants(depth, nc, n_bytes) + cases.many_currency_plants(depth, nc, n_bytes):
            check(gpu, cases.planted(depth, nc, n_bytes, plant), n_bytes, caps, (name, depth, nc, n_bytes))


def run_abi_np(ffi, d_bal, depth, nc, n_bytes, cap):
    """run_abi for the depths where lists of Python integers cost too much: the same call over the same pre-filled buffers, the
    outputs as numpy arrays, the list whole -- the listed leaves and the two spare entries behind the cap"""
    import torch
    S = ffi.snapshot_lib()
    leaves = 1 << depth
    bad_cap = leaves if cap is None else cap
    size = C.c_uint64(0)
    ffi.check(S.ss_mst_range_audit_scratch(depth, C.byref(size)))
    d_flags = torch.full((2 * leaves - 1,), 0xEE, dtype=torch.uint8, device="cuda")
    d_masks = torch.full((leaves,), UNWRITTEN, dtype=torch.int32, device="cuda")
    d_bad = torch.full((bad_cap + 2,), UNWRITTEN, dtype=torch.int32, device="cuda")
    d_scratch = torch.full((size.value // 4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    summary = (C.c_uint64 * 4)()
    torch.cuda.current_stream().synchronize()
    ffi.check(S.ss_mst_range_audit_dev(ffi.dev_ptr(d_bal), depth, nc, n_bytes, ffi.dev_ptr(d_flags), ffi.dev_ptr(d_masks),
                                       ffi.dev_ptr(d_bad) if bad_cap else None, bad_cap, ffi.dev_ptr(d_scratch), summary,
                                       ffi.current_stream_ptr()))
    return {"flags": d_flags.cpu().numpy(), "masks": d_masks.cpu().numpy().view(np.uint32), "bad": d_bad.cpu().numpy().view(np.uint32),
            "summary": list(summary)}


@pytest.mark.parametrize("depth", sorted(cases.SPARSE_DEPTHS))
def test_sparse_trees_past_64_groups_agree_with_the_numpy_model(gpu, depth):
    """4, 64 and 128 groups of the list's compaction: at 64 every lane of the scatter's wave holds a group's total and all six
    shuffle steps carry data, at 128 the loop over the totals takes its second trip"""
    import torch
    nc, n_bytes = cases.SPARSE_DEPTHS[depth], cases.SPARSE_N_BYTES
    assert (1 << depth) // cases.GROUP_ROWS == {16: 4, 20: cases.LANES, 21: 2 * cases.LANES}[depth]
    for name, plant, caps in cases.sparse_plants(depth, n_bytes):
        nodes = cases.sparse_nodes(depth, nc, plant)
        d_bal = torch.from_numpy(cases.sparse_bytes(depth, nc, nodes)).cuda()
        full = cases.sparse_model(depth, n_bytes, nodes)
        assert full["summary"][1] == caps[3] and len(caps) == 5 + (depth == 21) and all(1 < c < caps[3] for c in caps[5:])
        for cap in caps:
            want, got = cases.cut(full, cap), run_abi_np(gpu, d_bal, depth, nc, n_bytes, cap)
            what = (name, depth, cap)
            assert got["summary"] == want["summary"], what
            listed = want["summary"][2]
            wrong = np.flatnonzero(got["bad"][:listed] != want["bad"])
            assert wrong.size == 0, (what, "the list", int(wrong[0]), int(got["bad"][wrong[0]]), int(want["bad"][wrong[0]]))
            assert (got["bad"][listed:] == UNWRITTEN).all(), (what, "entries behind the listed leaves were written")
            assert np.array_equal(got["masks"], want["masks"]) and np.array_equal(got["flags"], want["flags"]), what


@pytest.mark.parametrize("kind", wc.TREE_KINDS)
@pytest.mark.parametrize("cfg", wc.witness_configs(), ids=lambda c: f"levels{c.levels}-nc{c.nc}-bytes{c.n_bytes}")
def test_real_trees_agree_with_the_model(gpu, cfg, kind):
    import torch
    from circuits_halo2_amd.merkle_sum_tree import DeviceMerkleSumTree
    tree = wc.witness_tree(cfg.levels, cfg.nc, kind, cfg.n_bytes)
    users, bals = wc.tree_words(tree)
    dev = DeviceMerkleSumTree(torch.from_numpy(np.ascontiguousarray(users)).cuda(), torch.from_numpy(np.ascontiguousarray(bals)).cuda(),
                              cfg.levels, cfg.nc)
    want = cases.model(tree.node_bal, cfg.n_bytes, 1 << cfg.levels)
    a = dev.range_audit(cfg.n_bytes)
    assert [a.n_bad_nodes, a.n_unprovable, len(a.unprovable), 0 if a.root_in_range else a.root_currency + 1] == want["summary"]
    assert a.unprovable.dtype == np.uint32 and a.unprovable.tolist() == want["bad"] and a.n_bytes == cfg.n_bytes
    assert a.d_node_flags.cpu().tolist() == want["flags"] and a.d_leaf_reasons.cpu().tolist() == want["masks"]
    assert a.reasons(range(1 << cfg.levels)).tolist() == want["masks"]
    assert a.ok == (kind == "in_range")
    capped = dev.range_audit(cfg.n_bytes, cap=1)
    assert capped.unprovable.tolist() == want["bad"][:1] and capped.n_unprovable == want["summary"][1]
    top = cases.top_of(cfg.n_bytes)
    for idx in range(1 << cfg.levels):                         # every entry of the explanation is a range check the circuit makes
        told = dev.explain_unprovable(a, idx)
        checked = {v for _, v in wc.range_checked(cfg, tree, idx) if v >= top}
        assert {t[4] for t in told} == checked and (told == []) == (want["masks"][idx] == 0), idx


def test_the_overflow_csv_the_plain_one_and_an_update_between_audits(gpu):
    import torch
    from circuits_halo2_amd.merkle_sum_tree import DeviceMerkleSumTree
    tree = DeviceMerkleSumTree.from_csv(OVERFLOW, 2)
    a = tree.range_audit(8)
    levels = cases.csv_levels(OVERFLOW)
    assert a.d_leaf_reasons.cpu().tolist() == OVERFLOW_MASKS and a.unprovable.tolist() == list(range(16))
    assert (a.n_bad_nodes, a.n_unprovable, a.root_in_range, a.root_currency, a.ok) == (5, 16, False, 0, False)
    assert tree.explain_unprovable(a, 0) == [("leaf", 0, 0, 0, 1 << 112)]
    assert tree.explain_unprovable(a, 1) == [("sibling", 0, 0, 0, 1 << 112)]
    assert tree.explain_unprovable(a, 8) == [("sibling", 3, 0, 0, levels[3][0][0])]
    # on one stream: the update repairs user 0, and the audit behind it is ok
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        tree.update_leaves_at([0], [[11888, levels[0][0][1]]])
        b = tree.range_audit(8)
    assert b.ok and b.n_bad_nodes == 0 and b.unprovable.size == 0 and not b.d_leaf_reasons.any().item()
    assert not a.ok                                            # the earlier audit is a snapshot of the earlier tree
    plain = DeviceMerkleSumTree.from_csv(PLAIN, 2)
    assert plain.range_audit(8).ok
    with torch.cuda.stream(side):
        leaves = [list(b_) for b_ in cases.csv_levels(PLAIN)[0]]
        leaves[5][0] = cases.top_of(8)
        plain.update_leaves_at([5], [leaves[5]])
        c = plain.range_audit(8)
    want = cases.model(cases.levels_of(leaves), 8, 16)
    assert c.d_node_flags.cpu().tolist() == want["flags"] and c.d_leaf_reasons.cpu().tolist() == want["masks"]
    assert c.unprovable.tolist() == want["bad"] == list(range(16)) and [c.n_bad_nodes, c.n_unprovable] == want["summary"][:2]
    assert plain.explain_unprovable(c, 5) == [("leaf", 0, 5, 0, cases.top_of(8))]


def test_the_audit_is_ordered_on_its_stream(gpu):
    """the node balances hold an in-range decoy; on a side stream a delay, the copy of the real out-of-range array, and behind
    it, with no wait in between, the audit: its answer must be the real array's"""
    import torch
    depth, nc, n_bytes = 11, 2, 8
    name, plant, _ = [p for p in cases.plants(depth, nc, n_bytes) if p[0] == "edges"][0]
    real = cases.planted(depth, nc, n_bytes, plant)
    decoy = cases.planted(depth, nc, n_bytes, [])
    want = cases.model(real, n_bytes, 1 << depth)
    assert want["summary"][1] and cases.model(decoy, n_bytes, 1 << depth)["summary"] == [0, 0, 0, 0]
    d_real = torch.from_numpy(cases.mont_bytes(cases.level_major(real))).cuda()
    d_in = torch.from_numpy(cases.mont_bytes(cases.level_major(decoy))).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        torch.cuda._sleep(60_000_000)                          # some 25 ms: the copy has not run when the audit is enqueued
        d_in.copy_(d_real, non_blocking=True)
    got = run_abi(gpu, d_in, depth, nc, n_bytes, None, stream=side)
    for key in ("summary", "bad", "masks", "flags"):
        assert got[key] == want[key], key


def test_two_runs_are_byte_identical(gpu):
    import torch
    depth, nc, n_bytes = 11, 3, 5
    top = cases.top_of(n_bytes)
    rng = np.random.default_rng(5)
    spots = sorted(set(rng.integers(0, 1 << depth, 300).tolist()))
    plant = [(i, i % nc, top + i) for i in spots] + [(i ^ 1, i % nc, cases.R - top - i) for i in spots if i ^ 1 not in spots]
    levels = cases.planted(depth, nc, n_bytes, plant)
    d_bal = torch.from_numpy(cases.mont_bytes(cases.level_major(levels))).cuda()
    one, two = run_abi(gpu, d_bal, depth, nc, n_bytes, None), run_abi(gpu, d_bal, depth, nc, n_bytes, None)
    assert one["summary"] == two["summary"] == cases.model(levels, n_bytes, 1 << depth)["summary"] and one["summary"][1] > 300
    assert all(torch.equal(x, y) for x, y in zip(one["tensors"], two["tensors"]))


def test_prove_batch_reports_every_user_of_the_overflow_tree_from_the_audit(gpu):
    """k = 11, the reference's: all sixteen users go to `errors` with their first failing range check and the launch log of the
    commitments' accumulations stays empty; a user of the plain tree, audited as well, is proved (and the log shows it)"""
    from circuits_halo2_amd import batch as B
    from circuits_halo2_amd.merkle_sum_tree import DeviceMerkleSumTree
    levels, nc, k = 4, 2, 11
    params, pk, vk = B.setup_on_all_ranks(k, os.path.join(GOLDEN, "hermez-raw-11"), levels, nc)
    try:
        tree = DeviceMerkleSumTree.from_csv(OVERFLOW, nc)
        gpu.set_param("msm.acc_log", 1)
        try:
            res = B.prove_batch(tree, list(range(16)), params, pk, levels, audit=tree.range_audit())
            log = gpu.msm_launch_log()
            plain = DeviceMerkleSumTree.from_csv(PLAIN, nc)
            gpu.set_param("msm.acc_log", 1)                    # clears the log
            control = B.prove_batch(plain, [3], params, pk, levels, audit=plain.range_audit())
            control_log = gpu.msm_launch_log()
        finally:
            gpu.set_param("msm.acc_log", 0)
        where = ["leaf"] + [f"sibling at level {l}" for l in (0, 1, 1, 2, 2, 2, 2)] + ["sibling at level 3"] * 8
        assert res.errors == {i: f"range check: {w}, currency 0" for i, w in enumerate(where)} and res.proofs == {}
        assert log == [], "a proof's commitments ran for a user the audit had filed"
        assert not control.errors and sorted(control.proofs) == [3] and control_log
    finally:
        params.free()
