"""A device-resident Merkle sum tree updated in place: sg_mst_update_dev of csrc/abi_mst.hip (the listed forms of mst_leaves_kernel /
mst_level_kernel of csrc/witness.hip, the launch plan of csrc/mst_update_plan.h) through `DeviceMerkleSumTree.update_leaf /
update_leaves / update_leaves_at` and through the C ABI.

Every expected value comes from the oracle: the tree of the MODIFIED entries, built by the C oracle's leaf and level functions
over pyref.mst_entry's field elements (oracle.fr_to_mont brings integers to memory form).  After every update all four arrays
of the tree -- usernames, leaf balances, node hashes, node balances -- are compared byte for byte, so a node the update should
not have touched, or one it forgot, shows."""
import functools
import os
import random

import numpy as np
import pytest

from conftest import GOLDEN

from oracle import pyref as P

pytestmark = pytest.mark.gpu

R = P.R
NINETY_DIGITS = 10 ** 89 + 7
SPECIAL = [0, (1 << 64) - 1, R - 1, R, R + 1, NINETY_DIGITS, 12]       # r and r + 1 reduce mod r; 12 travels as "00012" where a test says so


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    import circuits_halo2_amd as sg
    from circuits_halo2_amd import ffi
    ffi.check(sg.lib().sg_init(0))
    yield sg
    torch.cuda.synchronize()


def mont(values) -> np.ndarray:
    from oracle import oracle as O
    canon = b"".join((v % R).to_bytes(32, "little") for v in values)
    return O.fr_to_mont(np.frombuffer(canon, dtype=np.uint8).copy())


@functools.lru_cache(maxsize=None)
def username_fr(name) -> int:
    return 0 if name is None else P.mst_entry(name, [])[0]


def oracle_tree(entries, nc):
    """[(name or None or field element, [balances])], 2^depth of them -> (usernames, leaf balances, node hashes, node balances)
    as the bytes a device-resident tree of them holds"""
    from oracle import oracle as O
    assert len(entries) & (len(entries) - 1) == 0
    users = mont([u if isinstance(u, int) else username_fr(u) for u, _ in entries])
    bals = mont([b for _, bal in entries for b in bal])
    hs, bs = [O.mst_leaves(users, bals, nc)], [bals]
    while hs[-1].size > 32:
        h, b = O.mst_level(hs[-1], bs[-1], nc)
        hs.append(h)
        bs.append(b)
    return users, bals, np.concatenate(hs), np.concatenate(bs)


def arrays(tree):
    return [t.cpu().numpy().copy() for t in (tree.d_users, tree.d_bals, tree.d_h, tree.d_b)]


def same_tree(got, want, what):
    for name, g, w in zip(("usernames", "leaf balances", "node hashes", "node balances"), got, want):
        g, w = np.asarray(g).reshape(-1), np.asarray(w).reshape(-1)
        assert g.size == w.size, f"{what}: {name}: {g.size} bytes, {w.size} expected"
        bad = (g.reshape(-1, 32) != w.reshape(-1, 32)).any(axis=1)
        assert not bad.any(), f"{what}: {name}: {int(bad.sum())} of {bad.size} rows differ, first at row {int(np.argmax(bad))}"


def start_entries(n, nc):
    return [(f"user{i}", [1000 * i + 10 * c + 1 for c in range(nc)]) for i in range(n)]


def new_balances(idx, nc, shift=0):
    """balances for the leaves `idx` that cycle through SPECIAL and, beyond it, values of their own"""
    rows = []
    for j, i in enumerate(idx):
        rows.append([SPECIAL[(j * nc + c + shift) % len(SPECIAL)] if (j * nc + c) < 2 * len(SPECIAL) else 7 * i + c + 5 + shift for c in range(nc)])
    return rows


def applied(entries, idx, rows):
    out = list(entries)
    for i, bal in zip(idx, rows):
        out[i] = (out[i][0], list(bal))
    return out


# ============================================================================= every shape of the plan
DEPTH5 = [[0], [31], [0, 31], [6, 7], [7, 8], list(range(32))]
CASES = ([(0, 1, [0])] + [(1, 2, idx) for idx in ([0], [1], [0, 1])] + [(5, nc, idx) for nc in (1, 2, 3) for idx in DEPTH5] +
         [(8, 2, sorted(random.Random(8).sample(range(256), 129))), (8, 2, list(range(256))), (9, 1, list(range(0, 258, 2)))])


@pytest.mark.parametrize("depth,nc,idx", CASES, ids=[f"depth{d}-nc{nc}-{len(idx)}from{idx[0]}to{idx[-1]}" for d, nc, idx in CASES])
def test_update_leaves_at_gives_the_tree_of_the_modified_entries(gpu, depth, nc, idx):
    """one leaf at either end, both ends (they meet at the root only), siblings, neighbours under different parents, every leaf;
    129 leaves cross the 128-thread block of the leaf kernel and of the first level's; the 129 even leaves of depth 9 have 129
    distinct parents, the one list of a level kernel that runs one past a block.  The new balances hold 0, 2^64 - 1,
    r - 1, r, r + 1 and a 90-digit number."""
    from circuits_halo2_amd.merkle_sum_tree import DeviceMerkleSumTree
    entries = start_entries(1 << depth, nc)
    tree = DeviceMerkleSumTree.from_entries(entries, nc)
    assert tree.depth == depth
    same_tree(arrays(tree), oracle_tree(entries, nc), "as built")
    rows = new_balances(idx, nc)
    root = tree.update_leaves_at(idx, rows)
    entries = applied(entries, idx, rows)
    want = oracle_tree(entries, nc)
    same_tree(arrays(tree), want, "after the update")
    assert bytes(root[0]) == want[2][-32:].tobytes() and bytes(root[1]) == want[3][-32 * nc:].tobytes()
    assert tree.entries == entries


def test_balance_fields_through_the_abi(gpu):
    """the decimal fields as the ABI takes them: zero, the 64-bit boundary, r - 1, r and r + 1 (reduced mod r), 90 digits, leading
    zeros; all four leaves of a tree of depth 2"""
    from circuits_halo2_amd import ffi
    from circuits_halo2_amd.merkle_sum_tree import DeviceMerkleSumTree
    entries = start_entries(4, 2)
    tree = DeviceMerkleSumTree.from_entries(entries, 2)
    values = SPECIAL + [NINETY_DIGITS + 1]
    fields = [str(v).encode() for v in values]
    fields[6] = b"00012"
    assert len(fields[5]) == 90 and len(fields) == 8
    idx = np.arange(4, dtype=np.uint32)
    off = np.zeros(9, dtype=np.uint64)
    off[1:] = np.cumsum([len(f) for f in fields])
    data = np.frombuffer(b"".join(fields), dtype=np.uint8).copy()
    ffi.check(ffi.lib().sg_mst_update_dev(ffi.ptr(idx), ffi.ptr(data), ffi.ptr(off), 4, 2, 2, ffi.dev_ptr(tree.d_users), ffi.dev_ptr(tree.d_bals),
                                          ffi.dev_ptr(tree.d_h), ffi.dev_ptr(tree.d_b), ffi.current_stream_ptr()))
    import torch
    torch.cuda.synchronize()
    want = oracle_tree([(e[0], values[2 * i:2 * i + 2]) for i, e in enumerate(entries)], 2)
    same_tree(arrays(tree), want, "after the update")
    assert (want[1].reshape(-1, 32)[3] == 0).all() and (want[1].reshape(-1, 32)[0] == 0).all()      # r is 0


# ============================================================================= one update after another
def test_a_second_batch_and_the_way_back(gpu):
    """batches on one tree: the second one overlaps the first and reuses the work space; giving every touched leaf its first
    balances again restores the four arrays byte for byte"""
    from circuits_halo2_amd.merkle_sum_tree import DeviceMerkleSumTree
    nc = 2
    entries = start_entries(32, nc)
    tree = DeviceMerkleSumTree.from_entries(entries, nc)
    first = arrays(tree)
    a, b = [3, 4, 5, 17, 30], [0, 4, 5, 6, 7, 8, 9, 31]
    now = applied(entries, a, new_balances(a, nc))
    tree.update_leaves_at(a, new_balances(a, nc))
    same_tree(arrays(tree), oracle_tree(now, nc), "first batch")
    now = applied(now, b, new_balances(b, nc, shift=3))
    tree.update_leaves_at(b, new_balances(b, nc, shift=3))
    same_tree(arrays(tree), oracle_tree(now, nc), "second batch")
    touched = sorted(set(a) | set(b))
    tree.update_leaves([(entries[i][0], entries[i][1]) for i in reversed(touched)])
    same_tree(arrays(tree), first, "restored")
    assert tree.entries == entries


def test_update_leaf_on_the_references_case(gpu):
    """merkle_sum_tree/tests.rs `test_update_mst_leaf`: the tree of entry_16_modified.csv with RkLzkDun's balances put right is
    the tree of entry_16.csv; an unknown user raises and leaves the tree alone"""
    from circuits_halo2_amd.merkle_sum_tree import DeviceMerkleSumTree, parse_csv_to_entries
    tree = DeviceMerkleSumTree.from_csv(os.path.join(GOLDEN, "entry_16_modified.csv"), 2, 8)
    entries, _ = parse_csv_to_entries(os.path.join(GOLDEN, "entry_16.csv"), 2)
    want = oracle_tree(entries, 2)
    modified = arrays(tree)
    assert (modified[2][-32:] != want[2][-32:]).any()
    with pytest.raises(KeyError, match="Username not found"):
        tree.update_leaf("nobody", [1, 2])
    same_tree(arrays(tree), modified, "after a refused update")
    root = tree.update_leaf("RkLzkDun", [2087, 79731])
    assert bytes(root[0]) == want[2][-32:].tobytes() and bytes(root[1]) == want[3][-64:].tobytes()
    same_tree(arrays(tree), want, "entry_16.csv")
    assert tree.entries == entries and tree.get_entry(tree.index_of_username("RkLzkDun")) == ("RkLzkDun", [2087, 79731])
    oracle_root = P.mst_build([P.mst_entry(n, b) for n, b in entries])[0]               # the integer definition, once
    assert bytes(root[0]) == mont([oracle_root[0]]).tobytes() and oracle_root[1] == [556862, 556862]


def test_a_repeated_username_keeps_its_last_balances(gpu):
    from circuits_halo2_amd.merkle_sum_tree import DeviceMerkleSumTree
    entries = start_entries(16, 2)
    batch, single = DeviceMerkleSumTree.from_entries(entries, 2), DeviceMerkleSumTree.from_entries(entries, 2)
    updates = [("user9", [1, 2]), ("user2", [3, R + 4]), ("user9", [5, 6])]
    batch.update_leaves(updates)
    for name, bal in updates:
        single.update_leaf(name, bal)
    same_tree(arrays(batch), arrays(single), "batch against single updates")
    want = applied(entries, [2, 9], [[3, R + 4], [5, 6]])
    same_tree(arrays(batch), oracle_tree(want, 2), "batch")
    assert batch.entries == single.entries == want


def test_update_leaves_at_without_entries_and_on_a_padded_row(gpu):
    import torch
    from circuits_halo2_amd.merkle_sum_tree import DeviceMerkleSumTree, parse_csv_to_entries
    fr = [(username_fr(f"user{i}"), [i + 1, 2 * i + 1, 3 * i]) for i in range(8)]
    users = torch.from_numpy(mont([u for u, _ in fr])).cuda()
    bals = torch.from_numpy(mont([b for _, bal in fr for b in bal])).cuda()
    tree = DeviceMerkleSumTree(users, bals, 3, 3)
    assert tree.entries is None
    tree.update_leaves_at([6, 1, 6], [[9, 9, 9], [1, 0, R - 1], [4, 5, 6]])             # the last row for leaf 6 wins
    same_tree(arrays(tree), oracle_tree(applied(fr, [1, 6], [[1, 0, R - 1], [4, 5, 6]]), 3), "tree from field elements")
    assert tree.entries is None and tree.generate_proof(6)["entry"] == (fr[6][0], [4, 5, 6])
    with pytest.raises(IndexError, match="Index out of bounds"):
        tree.update_leaves_at([8], [[1, 2, 3]])
    with pytest.raises(KeyError, match="Username not found"):
        tree.update_leaf("user1", [1, 2, 3])
    # 13 entries in 16 rows: row 14 is a zero entry, and stays nameless
    entries, _ = parse_csv_to_entries(os.path.join(GOLDEN, "entry_13.csv"), 2)
    padded = DeviceMerkleSumTree.from_entries(entries, 2)
    padded.update_leaves_at([14, 12], [[77, 88], [1, 2]])
    want = applied(entries + [(None, [0, 0])] * 3, [12, 14], [[1, 2], [77, 88]])
    same_tree(arrays(padded), oracle_tree(want, 2), "padded row")
    assert padded.entries == want and padded.verify_proof(padded.generate_proof(14))


# ============================================================================= what is built on the tree
def test_merkle_proofs_and_public_inputs_follow_the_update(gpu):
    from circuits_halo2_amd.merkle_sum_tree import DeviceMerkleSumTree
    entries = start_entries(16, 2)
    tree = DeviceMerkleSumTree.from_entries(entries, 2)
    old_root = tree.root()                                    # (cached from here on)
    old_inputs = tree.public_inputs(6)
    old_proofs = {i: tree.generate_proof(i) for i in (6, 7, 12)}
    assert all(tree.verify_proof(p) for p in old_proofs.values())
    tree.update_leaf("user6", [123456, 0])
    want = oracle_tree(applied(entries, [6], [[123456, 0]]), 2)
    root = tree.root()
    assert bytes(root[0]) == want[2][-32:].tobytes() != bytes(old_root[0]) and bytes(root[1]) == want[3][-64:].tobytes()
    to_int = lambda row: int.from_bytes(bytes(row), "little") * pow(1 << 256, -1, R) % R
    inputs = tree.public_inputs(6)
    assert inputs[1] == to_int(root[0]) != old_inputs[1] and inputs[0] == to_int(want[2][32 * 6:32 * 7]) != old_inputs[0]
    assert inputs[2:] == [to_int(root[1][:32]), to_int(root[1][32:])]
    assert tree.public_inputs_many([12])[0][1:] == inputs[1:]
    for i in (6, 7, 12):                                      # the updated leaf, its sibling, a leaf far away
        proof = tree.generate_proof(i)
        assert bytes(proof["root"][0]) == bytes(root[0]) and tree.verify_proof(proof) is True, i
        stale = dict(old_proofs[i], root=root)                # what was proved before does not lead to the new root
        assert tree.verify_proof(stale) is False, i
    assert tree.generate_proof(6)["entry"] == ("user6", [123456, 0])


def test_inclusion_proof_of_an_updated_user_on_the_golden_srs(gpu):
    """the snapshot of entry_16.csv with one balance changed on the device: the witness of that user laid out from the tree
    (init_from_tree) gives a proof the verifier accepts, with the updated tree's root as public input"""
    from circuits_halo2_amd.api import MstInclusionCircuit, full_prover, full_verifier, generate_setup_artifacts
    from circuits_halo2_amd.merkle_sum_tree import DeviceMerkleSumTree, parse_csv_to_entries
    path = os.path.join(GOLDEN, "entry_16.csv")
    params, pk, vk = generate_setup_artifacts(11, os.path.join(GOLDEN, "hermez-raw-11"), MstInclusionCircuit.init_empty(4, 2, 8))
    try:
        tree = DeviceMerkleSumTree.from_csv(path, 2, 8)
        i = tree.index_of_username("RkLzkDun")
        tree.update_leaf("RkLzkDun", [2086, 79732])
        entries, _ = parse_csv_to_entries(path, 2)
        want = oracle_tree(applied(entries, [i], [[2086, 79732]]), 2)
        to_int = lambda row: int.from_bytes(bytes(row), "little") * pow(1 << 256, -1, R) % R
        circuit = MstInclusionCircuit.init_from_tree(tree, i)
        instances = circuit.instances()
        assert instances[0] == [to_int(want[2][32 * i:32 * i + 32]), to_int(want[2][-32:]), 556861, 556863]
        proof = full_prover(params, pk, circuit, instances)
        assert full_verifier(params, vk, proof, instances)
    finally:
        params.free()


def test_update_on_a_non_default_stream(gpu):
    import torch
    from circuits_halo2_amd.merkle_sum_tree import DeviceMerkleSumTree
    entries = start_entries(256, 2)
    idx = sorted(random.Random(5).sample(range(256), 129))
    rows = new_balances(idx, 2)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        tree = DeviceMerkleSumTree.from_entries(entries, 2)
        tree.update_leaves_at(idx, rows)
        tree.update_leaves_at([0], [[5, 6]])
    same_tree(arrays(tree), oracle_tree(applied(applied(entries, idx, rows), [0], [[5, 6]]), 2), "side stream")
