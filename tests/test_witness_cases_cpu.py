"""CPU checks of tests/witness_cases.py, the generators, case lists and the witness-program interpreter behind
tests/test_gpu_witness.py: the generators plant what they claim (every wrap class on every corner, 0x00 and 0xff on every byte
of a range check, balances that leave the range at a leaf, at a sibling and at a level-1 node), the case lists reach every
class of launch of the three kernels, the C oracle agrees with Python integers where the GPU tests rely on it, and the
interpreter -- which writes N_BYTES + 1 running sums per range check -- equals mst_inclusion.reference_assignment on every
cell of the three advice columns, for balances in and out of range."""
import pytest

import witness_cases as wc

R = wc.R


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def test_constants_and_edge_values():
    from oracle import pyref
    assert (wc.R, wc.MONT) == (pyref.R, pyref.MONT) and (wc.TREE_THREADS, wc.WITNESS_THREADS, wc.NC_MAX) == (128, 64, 64)
    e = wc.edge_values()
    assert len(set(e)) == len(e) == 14 and all(0 <= v < R for v in e) and {0, 1, 1 << 64, (1 << 64) + 5, R - 1} <= set(e)
    for name in ("random", "edges"):
        for n in (1, 5, 14, 40):
            w = wc.vector(name, n, 3)
            assert w.size == 32 * n and wc.is_canonical(w)
    assert wc.values_of(wc.vector("edges", 40, 3))[:14] == e
    w = wc.vector("noncanonical", 8, 3)
    first = [int.from_bytes(bytes(w[32 * i:32 * i + 32]), "little") for i in range(3)]
    assert first == [R, R + 1, (1 << 256) - 1] and not wc.is_canonical(w)
    assert wc.values_of(w)[:2] == wc.values_of(wc.to_words([0, 1]))      # r and r + 1 stand for the values of the words 0 and 1


def test_every_wrap_class_stands_on_every_corner():
    """over LEVEL_CASES each of the six pairs occurs at the first and last parent and in the first and last lane; a level with
    six slots or more has all six; the planted words are the pairs"""
    sums = {name: (a + b, (a + b) % R) for name, (a, b) in wc.WRAP_PAIRS.items()}
    assert sums["wraps far"] == (2 * R - 2, R - 2) and sums["wraps to zero"] == (R, 0) and sums["largest without a wrap"][0] == R - 1
    assert sums["zero"] == (0, 0) and sums["carry across the 64-bit word"][0] == (1 << 65) - 2 and sums["carry into the next word"][0] == 1 << 64
    corners = {c: set() for c in ("first parent", "last parent", "first lane", "last lane")}
    for m, nc in wc.LEVEL_CASES:
        pairs = wc.wrapping_pairs(nc, m)
        slots = len({(0, 0), (m - 1, nc - 1), (0, nc - 1), (m - 1, 0)}) + max(0, m - 2)
        assert len({(p, lane) for p, lane, _, _ in pairs}) == len(pairs) == min(12, slots)
        classes = {wc.wrap_class(a, b) for _, _, a, b in pairs}
        assert None not in classes and (len(pairs) < 6 or classes == set(wc.WRAP_PAIRS))
        for p, lane, a, b in pairs:
            assert 0 <= p < m and 0 <= lane < nc
            for corner, there in (("first parent", p == 0), ("last parent", p == m - 1), ("first lane", lane == 0), ("last lane", lane == nc - 1)):
                if there:
                    corners[corner].add(wc.wrap_class(a, b))
        _, bal = wc.level_children(m, nc, 5)
        v = wc.values_of(bal)
        assert wc.is_canonical(bal) and all((v[2 * p * nc + lane], v[(2 * p + 1) * nc + lane]) == (a, b) for p, lane, a, b in pairs)
    assert all(found == set(wc.WRAP_PAIRS) for found in corners.values()), corners
    # also where the lanes are many and the threads of a block differ in nothing but the parent
    wide = {(p, lane) for nc in wc.WIDE_NC for p, lane, _, _ in wc.wrapping_pairs(nc, wc.WIDE_N)}
    assert {(0, 0), (wc.WIDE_N - 1, 63), (0, 63), (wc.WIDE_N - 1, 0)} <= wide


def test_case_lists_reach_every_launch_class():
    wanted = {"below one block", "one block", "one past a block", "several blocks"}
    assert wanted <= set().union(*(wc.launch_classes(n, wc.TREE_THREADS) for n in wc.LEAF_SIZES))
    assert wanted <= set().union(*(wc.launch_classes(m, wc.TREE_THREADS) for m in wc.LEVEL_PARENTS + [wc.WIDE_N]))
    assert wc.launch_classes(127, 128) == {"below one block"} and wc.launch_classes(128, 128) == {"one block"}
    assert wc.launch_classes(129, 128) == wc.launch_classes(257, 128) == {"several blocks", "one past a block"}
    assert wc.launch_classes(130, 128) == {"several blocks"} and max(wc.LEAF_SIZES) > 2 * wc.TREE_THREADS
    assert {nc for _, nc in wc.LEAF_CASES} == {1, 2, 3, 63, 64} == {nc for _, nc in wc.LEVEL_CASES}
    assert [n for n, nc in wc.LEAF_CASES if nc > 3] == [129, 129] and max(n * nc for n, nc in wc.LEAF_CASES) == 129 * 64 <= 257 * 64
    # a whole tree: one leaf and nothing else, one level, 2^7 leaves (exactly one block) and 2^8 (two blocks, then one)
    assert wc.BUILD_DEPTHS == [0, 1, 7, 8] and (1 << 7) == wc.TREE_THREADS
    # the witness kernel: x-blocks of 64 items
    cfgs = wc.witness_configs()
    assert [(c.levels, c.nc, c.n_bytes) for c in cfgs] == wc.WITNESS_CONFIGS and len(cfgs) == 7
    assert [c.k for c in cfgs[:6]] == [9, 10, 10, 11, 11, 11]
    items = [c.n_items for c in cfgs]
    assert any(n % wc.WITNESS_THREADS == 1 and n > wc.WITNESS_THREADS for n in items) and any(n < wc.WITNESS_THREADS for n in items)
    assert wc.config(3, 2, 8).n_items == 65
    wide = wc.config(1, wc.NC_MAX, 8)
    assert wide.n_items > wc.WITNESS_THREADS and wide.k <= 14
    for c in cfgs:
        from circuits_halo2_amd import mst_inclusion as M
        assert c.rows_used + M.BLINDING_FACTORS + 1 <= 1 << c.k and (c.k == 4 or c.rows_used + M.BLINDING_FACTORS + 1 > 1 << (c.k - 1))
        prog = wc.program(c)
        assert prog.size == 5 * c.n_items + 3 * c.n_absorbs
        its = prog[:5 * c.n_items].reshape(-1, 5)
        sponges = its[its[:, 0] == 2]
        assert len(sponges) == len(wc.sponge_digests(c.levels)) and (its[:len(sponges), 0] == 2).all()
        # the fields of the widest configuration fit: lanes (a currency, or child 0 / 1 of a node) below 128, counts below 256
        assert int(((sponges[:, 4] >> 20) & 255).max()) == c.nc + 2 and int(((its[:, 3] >> 13) & 127).max()) == max(c.nc - 1, 1)
        assert all(int(e) == c.n_bytes for e in its[its[:, 0] == 1][:, 4])


def test_users_of_a_launch():
    for levels in (1, 2, 4):
        u = wc.witness_users(levels)
        size = 1 << levels
        assert len(u) == 2 * size + 1 and u[:size] == list(range(size)) and u[size:2 * size] == u[:size][::-1] and u[-1] in u[:size]


@pytest.mark.parametrize("shape", wc.WITNESS_CONFIGS)
def test_trees_reach_the_bytes_and_the_overflows_they_claim(shape):
    levels, nc, n_bytes = shape
    cfg = wc.config(*shape)
    size, top = 1 << levels, 1 << (8 * n_bytes)
    # in range: every range-checked value is, and every byte position sees 0x00 and 0xff
    t = wc.witness_tree(levels, nc, "in_range", n_bytes)
    seen = [set() for _ in range(n_bytes)]
    for idx in range(size):
        for _, v in wc.range_checked(cfg, t, idx):
            assert v < top
            for b in range(n_bytes):
                seen[b].add((v >> (8 * b)) & 0xFF)
    assert all({0x00, 0xFF} <= s for s in seen)
    assert ({0, 1, R - 1} <= set(t.users) if size > 2 else set(t.users) in ({1, R - 1}, {0, 1}))
    # out of range: a non-zero z_{N_BYTES} at the user's own leaf, at the sibling leaf and, with two levels, at a level-1 node
    # whose children are both in range
    t = wc.witness_tree(levels, nc, "out_of_range", n_bytes)
    where = set()
    for idx in range(size):
        for s, v in wc.range_checked(cfg, t, idx):
            if v >> (8 * n_bytes):
                level, mode, lane = (s >> 4) & 63, (s >> 10) & 7, (s >> 13) & 127
                where.add((level, mode))
                if level == 1:
                    node = (idx >> 1) ^ 1
                    if all(t.node_bal[0][2 * node + j][lane] < top for j in (0, 1)):
                        where.add("first at level 1")
    assert {(0, 0), (0, 1)} <= where and (levels < 2 or {(1, 1), "first at level 1"} <= where)
    leaf_values = {b for leaf in t.node_bal[0] for b in leaf}
    assert {top + 5, R - 1} <= leaf_values and (size * nc == 2 or top in leaf_values)
    pair_sums = [t.node_bal[0][2 * p][c] + t.node_bal[0][2 * p + 1][c] for p in range(size // 2) for c in range(nc)]
    assert any(v >= R for v in pair_sums) and (size * nc == 2 or R in pair_sums)          # a sum that wraps; one that wraps to 0


def test_the_oracle_equals_python_integers(O):
    """O.mst_leaves / O.mst_level (what the GPU tests compare with on canonical words) against pyref's Poseidon in Python
    integers, on the edge values and the wrapping pairs; and the integer path on non-canonical words against the oracle on the
    same words reduced"""
    for nc in (1, 3):
        n = 5
        users, bal = wc.leaf_inputs("edges", n, nc, 7)
        assert (O.mst_leaves(users, bal, nc) == wc.expected_leaves(O, users, bal, nc, canonical=False)).all()
        m = 3
        ch, cb = wc.level_children(m, nc, 9)
        assert len(wc.wrapping_pairs(nc, m)) >= 3
        h, b = O.mst_level(ch, cb, nc)
        h2, b2 = wc.expected_level(O, ch, cb, nc, canonical=False)
        assert (h == h2).all() and (b == b2).all() and wc.is_canonical(b)
    import poly_cases as pc
    n, nc = wc.NONCANONICAL_LEAVES
    users, bal = wc.leaf_inputs("noncanonical", n, nc, 11)
    assert (wc.expected_leaves(O, users, bal, nc, canonical=False) == O.mst_leaves(pc.reduced(users), pc.reduced(bal), nc)).all()
    # the whole tree in integers (witness_tree) is the oracle's
    t = wc.witness_tree(3, 2, "out_of_range", 8)
    users, bal = wc.tree_words(t)
    hashes, bals, _, _ = wc.expected_tree(O, users, bal, 3, 2)
    assert (hashes == wc.mont([h for lv in t.node_hash for h in lv])).all()
    assert (bals == wc.mont([b for lv in t.node_bal for node in lv for b in node])).all()


@pytest.mark.parametrize("kind", wc.TREE_KINDS)
@pytest.mark.parametrize("shape", wc.WITNESS_CONFIGS)
def test_run_program_equals_the_reference_assignment_on_every_cell(shape, kind):
    """whole-column equality of the three advice columns with reference_assignment(lenient=True), for every leaf of the tree:
    the program's semantics -- N_BYTES + 1 running sums per range check -- suffice for balances out of range too.  With
    N_BYTES rows instead (what the kernel wrote before), the columns differ exactly at the last rows of the range checks
    whose value has more than N_BYTES bytes."""
    cfg = wc.config(*shape)
    tree = wc.witness_tree(cfg.levels, cfg.nc, kind, cfg.n_bytes)
    prog = wc.program(cfg)
    assert sorted(set(wc.witness_users(cfg.levels))) == list(range(1 << cfg.levels))
    differing = 0
    for idx in range(1 << cfg.levels):
        want = wc.reference_columns(cfg, kind, idx)
        got = wc.run_program(prog, cfg.n_items, tree, idx, 1 << cfg.k)
        for c in range(3):
            assert len(got[c]) == len(want[c]) == 1 << cfg.k
            if got[c] != want[c]:
                bad = [r for r in range(1 << cfg.k) if got[c][r] != want[c][r]]
                raise AssertionError(f"leaf {idx}, column {c}: {len(bad)} rows differ, first at row {bad[0]}")
        if idx in (0, (1 << cfg.levels) - 1):
            short = wc.run_program(prog, cfg.n_items, tree, idx, 1 << cfg.k, range_rows=lambda n_bytes: n_bytes)
            last_rows = {int(row) + cfg.n_bytes: v >> (8 * cfg.n_bytes)
                         for (k_, _, row, _, _), (_, v) in zip([it for it in prog[:5 * cfg.n_items].reshape(-1, 5) if it[0] == 1],
                                                               wc.range_checked(cfg, tree, idx))}
            diff = {r for r in range(1 << cfg.k) if short[0][r] != want[0][r]}
            assert short[1:] == want[1:] and diff == {r for r, z in last_rows.items() if z}
            differing += len(diff)
    assert (differing > 0) == (kind == "out_of_range")
