"""The witness side of csrc/witness.hip through the C ABI (csrc/abi_mst.hip) -- sg_mst_leaves_dev, sg_mst_level_dev, sg_mst_build_dev (the
Poseidon Merkle sum tree) and sg_mst_inclusion_witness_dev (the advice columns of the inclusion circuit) -- at the sizes
where their launches change and on the values uniform sampling never gives: n off the 128-thread block edge (the threads
behind n leave after the staging barrier), up to 64 currencies, usernames and balances 0, 1, r - 1 and the 64-bit
boundaries, words >= r, child balances whose sums wrap mod r, range checks of 1 and 31 bytes, balances out of the range
check's range, 64 j + 1 program items, duplicate and reordered users in one launch.

tests/witness_cases.py lists the cases and restates the witness program in plain integers; tests/test_witness_cases_cpu.py
checks both without a GPU.  Every expected word comes from the CPU oracle, from Python integers or from
mst_inclusion.reference_assignment; every comparison is bit for bit; every output buffer starts as 0x5A bytes and ends in
guard rows that must come back untouched."""
import ctypes as C

import numpy as np
import pytest

import witness_cases as wc

pytestmark = pytest.mark.gpu

R = wc.R
GUARD_ROWS = 4
SG_ERR_INVALID = -1


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    import circuits_halo2_amd as sg
    from circuits_halo2_amd import ffi
    ffi.check(sg.lib().sg_init(0))
    yield sg
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def _L():
    from circuits_halo2_amd import ffi
    return ffi, ffi.lib()


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()      # (a copy: the shared inputs are read only)


def _out(rows):
    """`rows` output rows and the guard rows behind them, all 0x5A"""
    import torch
    return torch.full((32 * (rows + GUARD_ROWS),), 0x5A, dtype=torch.uint8, device="cuda")


def _fetch(buf, rows, what):
    """the first `rows` rows of an output buffer; the guard rows behind them must still be 0x5A"""
    import torch
    torch.cuda.synchronize()
    g = buf.cpu().numpy()
    assert (g[32 * rows:] == 0x5A).all(), f"{what}: the rows behind the output changed"
    return g[:32 * rows]


def _same(got, want, what):
    """bit for bit; on a mismatch say how many rows differ and where the first one is"""
    g = np.asarray(got).reshape(-1)
    assert g.size == want.size, f"{what}: {g.size} bytes, {want.size} expected"
    if g.size % 32 or (g != want).any():
        bad = (g.reshape(-1, 32) != want.reshape(-1, 32)).any(axis=1)
        assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} rows differ, first at row {int(np.argmax(bad))}"


def _leaves(users, bal, n, nc, rows=None):
    ffi, L = _L()
    out = _out(n if rows is None else rows)
    d = [_dev(users), _dev(bal)] if n else [None, None]
    rc = L.sg_mst_leaves_dev(ffi.dev_ptr(d[0]) if n else None, ffi.dev_ptr(d[1]) if n else None, C.c_size_t(n), C.c_uint32(nc),
                             ffi.dev_ptr(out), ffi.current_stream_ptr())
    return rc, out


def _level(child_hash, child_bal, m, nc):
    ffi, L = _L()
    h, b = _out(m), _out(m * nc)
    d = [_dev(child_hash), _dev(child_bal)]
    rc = L.sg_mst_level_dev(ffi.dev_ptr(d[0]), ffi.dev_ptr(d[1]), C.c_size_t(m), C.c_uint32(nc), ffi.dev_ptr(h), ffi.dev_ptr(b),
                            ffi.current_stream_ptr())
    return rc, h, b


def _build(users, leaf_bal, depth, nc):
    """-> (status, node hashes, node balances): device buffers of 2^(depth+1) - 1 nodes and the guard rows"""
    ffi, L = _L()
    nodes = (2 << depth) - 1
    h, b = _out(nodes), _out(nodes * nc)
    d = [_dev(users), _dev(leaf_bal)]
    rc = L.sg_mst_build_dev(ffi.dev_ptr(d[0]), ffi.dev_ptr(d[1]), C.c_uint32(depth), C.c_uint32(nc), ffi.dev_ptr(h), ffi.dev_ptr(b),
                            ffi.current_stream_ptr())
    return rc, h, b, d


# ============================================================================= leaves
@pytest.mark.parametrize("n,nc", wc.LEAF_CASES)
def test_leaves(gpu, O, n, nc):
    """sg_mst_leaves_dev against O.mst_leaves: n below, at and one past the 128-thread block, 1 to 3 currencies at every size
    and 63 / 64 at n = 129; random words, and the edge values (0, 1, the 64-bit boundaries, r - 1) as usernames and balances"""
    ffi, _ = _L()
    for name in ("random", "edges"):
        users, bal = wc.leaf_inputs(name, n, nc, 100 + n)
        rc, out = _leaves(users, bal, n, nc)
        ffi.check(rc)
        _same(_fetch(out, n, f"leaves n={n} nc={nc} {name}"), wc.expected_leaves(O, users, bal, nc), f"leaves n={n} nc={nc} {name}")


def test_leaves_of_words_not_below_r(gpu, O):
    """usernames and balances r, r + 1, 2^256 - 1 and uniform 256-bit words: the hashes are those of the words reduced mod r
    (Python integers), and canonical"""
    ffi, _ = _L()
    n, nc = wc.NONCANONICAL_LEAVES
    users, bal = wc.leaf_inputs("noncanonical", n, nc, 11)
    rc, out = _leaves(users, bal, n, nc)
    ffi.check(rc)
    got = _fetch(out, n, "leaves of non-canonical words")
    assert wc.is_canonical(got)
    _same(got, wc.expected_leaves(O, users, bal, nc, canonical=False), "leaves of non-canonical words")


def test_no_leaves(gpu):
    """n = 0: SG_OK, nothing written (with or without pointers)"""
    ffi, L = _L()
    rc, out = _leaves(None, None, 0, 2, rows=2)
    assert rc == 0 and (_fetch(out, 2, "no leaves") == 0x5A).all()
    d = _dev(wc.vector("random", 2, 1))
    assert L.sg_mst_leaves_dev(ffi.dev_ptr(d), ffi.dev_ptr(d), C.c_size_t(0), C.c_uint32(1), ffi.dev_ptr(out), ffi.current_stream_ptr()) == 0
    assert (_fetch(out, 2, "no leaves") == 0x5A).all()


# ============================================================================= one level
@pytest.mark.parametrize("m,nc", wc.LEVEL_CASES)
def test_level(gpu, O, m, nc):
    """sg_mst_level_dev against O.mst_level, hashes and summed balances: m parents around the block edge; child balances with
    the pairs planted whose sums wrap mod r (to r - 2, to 0), reach r - 1 or carry across a 64-bit word, at the first and last
    parent and lane; the sums are canonical words"""
    ffi, _ = _L()
    child_hash, child_bal = wc.level_children(m, nc, 200 + m)
    rc, h, b = _level(child_hash, child_bal, m, nc)
    ffi.check(rc)
    want_h, want_b = wc.expected_level(O, child_hash, child_bal, nc)
    what = f"level m={m} nc={nc}"
    got_b = _fetch(b, m * nc, what + " balances")
    assert wc.is_canonical(got_b)
    _same(got_b, want_b, what + " balances")
    _same(_fetch(h, m, what + " hashes"), want_h, what + " hashes")
    for p, lane, left, right in wc.wrapping_pairs(nc, m):        # (the oracle's sums are the integers')
        assert bytes(want_b[32 * (p * nc + lane):32 * (p * nc + lane + 1)]) == bytes(wc.mont([(left + right) % R]))


def test_level_of_words_not_below_r(gpu, O):
    ffi, _ = _L()
    m, nc = wc.NONCANONICAL_LEVEL
    child_hash, child_bal = wc.vector("noncanonical", 2 * m, 13), wc.vector("noncanonical", 2 * m * nc, 14)
    rc, h, b = _level(child_hash, child_bal, m, nc)
    ffi.check(rc)
    want_h, want_b = wc.expected_level(O, child_hash, child_bal, nc, canonical=False)
    got_h, got_b = _fetch(h, m, "level of non-canonical words"), _fetch(b, m * nc, "level of non-canonical words")
    assert wc.is_canonical(got_h) and wc.is_canonical(got_b)
    _same(got_b, want_b, "level of non-canonical words, balances")
    _same(got_h, want_h, "level of non-canonical words, hashes")


# ============================================================================= the whole tree
@pytest.mark.parametrize("nc", [1, 2])
@pytest.mark.parametrize("depth", wc.BUILD_DEPTHS)
def test_build(gpu, O, depth, nc):
    """sg_mst_build_dev: level-major, the leaves first and the root last, node for node the leaves followed by O.mst_level
    again and again; depth 0 is the one leaf and nothing else"""
    ffi, _ = _L()
    n = 1 << depth
    users, bal = wc.leaf_inputs("edges", n, nc, 300 + depth)
    rc, h, b, _ = _build(users, bal, depth, nc)
    ffi.check(rc)
    want_h, want_b, by_level, _ = wc.expected_tree(O, users, bal, depth, nc)
    nodes = 2 * n - 1
    assert want_h.size == 32 * nodes and want_b.size == 32 * nodes * nc and by_level[-1].size == 32
    what = f"tree depth={depth} nc={nc}"
    got_h, got_b = _fetch(h, nodes, what + " hashes"), _fetch(b, nodes * nc, what + " balances")
    _same(got_h, want_h, what + " hashes")
    _same(got_b, want_b, what + " balances")
    assert bytes(got_h[-32:]) == bytes(by_level[-1]) and bytes(got_b[:32 * n * nc]) == bytes(bal)
    if depth == 0:
        assert bytes(got_h) == bytes(O.mst_leaves(users, bal, nc))


# ============================================================================= the inclusion witness
_WITNESS = {}


def _witness(O, cfg, kind):
    """the device tree of witness_tree(kind) and the advice columns of wc.witness_users in one launch (computed once per
    configuration and shared, read only): (columns as a (users, 3, 32 rows) array, the user list, the oracle's node hashes by level)"""
    import torch
    key = (cfg, kind)
    if key not in _WITNESS:
        ffi, L = _L()
        tree = wc.witness_tree(cfg.levels, cfg.nc, kind, cfg.n_bytes)
        users_w, bal_w = wc.tree_words(tree)
        rc, h, b, (d_users, _) = _build(users_w, bal_w, cfg.levels, cfg.nc)
        ffi.check(rc)
        _, _, by_level, _ = wc.expected_tree(O, users_w, bal_w, cfg.levels, cfg.nc)
        idx = wc.witness_users(cfg.levels)
        rows = 1 << cfg.k
        d_prog = torch.from_numpy(wc.program(cfg).view(np.int32).copy()).cuda()
        d_idx = torch.tensor(idx, dtype=torch.int32, device="cuda")
        adv = _out(len(idx) * 3 * rows)
        ffi.check(L.sg_mst_inclusion_witness_dev(ffi.dev_ptr(d_prog), C.c_uint32(cfg.n_items), C.c_uint32(cfg.n_absorbs), ffi.dev_ptr(d_users),
                                                 ffi.dev_ptr(h), ffi.dev_ptr(b), C.c_uint32(cfg.levels), C.c_uint32(cfg.nc), ffi.dev_ptr(d_idx),
                                                 C.c_uint32(len(idx)), ffi.dev_ptr(adv), C.c_uint64(rows), ffi.current_stream_ptr()))
        got = _fetch(adv, len(idx) * 3 * rows, f"witness {cfg[:3]} {kind}").reshape(len(idx), 3, 32 * rows)
        got.setflags(write=False)
        _WITNESS[key] = (got, idx, by_level)
    return _WITNESS[key]


@pytest.mark.parametrize("kind", wc.TREE_KINDS)
@pytest.mark.parametrize("shape", wc.WITNESS_CONFIGS)
def test_inclusion_witness_equals_the_reference_assignment(gpu, O, shape, kind):
    """sg_mst_inclusion_witness_dev over a tree built by sg_mst_build_dev, every leaf in one launch, then every leaf again
    in reverse order and one a third time: all users x 3 x rows elements equal the advice columns of
    reference_assignment(lenient=True) -- what api.MstInclusionCircuit.synthesize lays out on the host -- for balances in
    range and for the overflow tree (2^(8 N_BYTES), 2^(8 N_BYTES) + 5, r - 1, and a sum that leaves the range one level up),
    whose range checks end in a non-zero running sum z_{N_BYTES}"""
    cfg = wc.config(*shape)
    got, users, _ = _witness(O, cfg, kind)
    assert got.shape == (len(users), 3, 32 << cfg.k)
    words = {idx: [wc.mont(col) for col in wc.reference_columns(cfg, kind, idx)] for idx in sorted(set(users))}
    for u, idx in enumerate(users):
        for c in range(3):
            _same(got[u, c], words[idx][c], f"witness {shape} {kind}: user {u} (leaf {idx}), column {c}")


@pytest.mark.parametrize("kind", wc.TREE_KINDS)
@pytest.mark.parametrize("shape", wc.WITNESS_CONFIGS)
def test_sponges_start_at_the_initial_state_and_end_in_the_trees_nodes(gpu, O, shape, kind):
    """independently of the replay: every sponge's initial-state row holds (0, count 2^64), and the column-0 cell at offset 36
    of its last permute region is the hash of the node it stands for in the oracle's tree -- the user's leaf, the path's
    sibling at each level, the next node of the path"""
    cfg = wc.config(*shape)
    got, users, by_level = _witness(O, cfg, kind)
    prog = wc.program(cfg)
    items = prog[:5 * cfg.n_items].reshape(-1, 5).tolist()
    absorbs = prog[5 * cfg.n_items:].reshape(-1, 3).tolist()
    sponges = [it for it in items if it[0] == 2]
    digests = wc.sponge_digests(cfg.levels)
    assert len(sponges) == len(digests)
    row = lambda u, c, r: bytes(got[u, c, 32 * r:32 * r + 32])
    for u, idx in enumerate(users):
        for (_, _, start, _, extra), (level, sibling) in zip(sponges, digests):
            first, count = extra & 0xFFFFF, (extra >> 20) & 255
            assert count == cfg.nc + (1 if level == 0 else 2)
            assert row(u, 0, start) == bytes(32) and row(u, 1, start) == bytes(wc.mont([count << 64])), (u, idx, level, sibling)
            node = (idx >> level) ^ (1 if sibling else 0)
            last = absorbs[first + count - 1][1] + wc.PERMUTE_ROWS - 1
            assert row(u, 0, last) == bytes(by_level[level][32 * node:32 * node + 32]), (u, idx, level, sibling)


@pytest.mark.parametrize("shape", [(2, 2, 1), (2, 2, 31)])
def test_mock_prover_reports_the_host_assignments_failures_for_the_device_witness(gpu, O, shape):
    """the overflow tree at k = 10 through the mock prover: with the device's advice columns it reports what it reports for
    the host's assignment -- the copies of the last running sums to the constant 0 fail (Permutation), no lookup does"""
    from circuits_halo2_amd.mock_prover import MockProver
    cfg = wc.config(*shape)
    assert cfg.k == 10
    got, users, _ = _witness(O, cfg, "out_of_range")
    for u in (0, 3):
        host = wc.reference(cfg, "out_of_range", users[u])
        dev = dict(host)
        dev["advice"] = [wc.values_of(got[u, c]) for c in range(3)]
        want = MockProver(cfg.k, host, cfg.nc).verify()
        assert want and "Permutation" in {f[0] for f in want} and "Lookup" not in {f[0] for f in want}
        assert MockProver(cfg.k, dev, cfg.nc).verify() == want


# ============================================================================= refusals
def _invalid(rc, L, what):
    assert rc == SG_ERR_INVALID, f"{what}: status {rc}"
    assert L.sg_last_error()


def test_refusals_of_the_tree_entry_points(gpu, O):
    """n_currencies 0 and 65, depth 31, a null pointer with n > 0: SG_ERR_INVALID, nothing written, and the next valid call is
    right.  (No call passes a pointer that is not a live device buffer.)"""
    ffi, L = _L()
    n, nc = 3, 2
    users, bal = wc.leaf_inputs("edges", 2 * n, nc, 400)
    want_leaves = wc.expected_leaves(O, users, bal, nc)
    want_level = wc.expected_level(O, users, bal, nc)
    want_tree = wc.expected_tree(O, users[:64], bal[:64 * nc], 1, nc)
    d_u, d_b = _dev(users), _dev(bal)
    s = ffi.current_stream_ptr()
    p = ffi.dev_ptr

    def leaves_ok():
        rc, out = _leaves(users, bal, 2 * n, nc)
        ffi.check(rc)
        _same(_fetch(out, 2 * n, "leaves after a refusal"), want_leaves, "leaves after a refusal")

    def level_ok():
        rc, h, b = _level(users, bal, n, nc)
        ffi.check(rc)
        _same(_fetch(h, n, "level after a refusal"), want_level[0], "level after a refusal, hashes")
        _same(_fetch(b, n * nc, "level after a refusal"), want_level[1], "level after a refusal, balances")

    def build_ok():
        rc, h, b, _ = _build(users[:64], bal[:64 * nc], 1, nc)
        ffi.check(rc)
        _same(_fetch(h, 3, "tree after a refusal"), want_tree[0], "tree after a refusal, hashes")
        _same(_fetch(b, 3 * nc, "tree after a refusal"), want_tree[1], "tree after a refusal, balances")

    out, out2 = _out(2 * n), _out(2 * n * nc)
    for bad_nc in (0, wc.NC_MAX + 1):
        _invalid(L.sg_mst_leaves_dev(p(d_u), p(d_b), C.c_size_t(n), C.c_uint32(bad_nc), p(out), s), L, f"leaves nc={bad_nc}")
        leaves_ok()
        _invalid(L.sg_mst_level_dev(p(d_u), p(d_b), C.c_size_t(n), C.c_uint32(bad_nc), p(out), p(out2), s), L, f"level nc={bad_nc}")
        level_ok()
        _invalid(L.sg_mst_build_dev(p(d_u), p(d_b), C.c_uint32(1), C.c_uint32(bad_nc), p(out), p(out2), s), L, f"build nc={bad_nc}")
        build_ok()
    _invalid(L.sg_mst_build_dev(p(d_u), p(d_b), C.c_uint32(31), C.c_uint32(nc), p(out), p(out2), s), L, "build depth=31")
    build_ok()
    for hole in range(3):
        a = [p(d_u), p(d_b), p(out)]
        a[hole] = None
        _invalid(L.sg_mst_leaves_dev(a[0], a[1], C.c_size_t(n), C.c_uint32(nc), a[2], s), L, f"leaves, null argument {hole}")
    leaves_ok()
    for hole in range(4):
        a = [p(d_u), p(d_b), p(out), p(out2)]
        a[hole] = None
        _invalid(L.sg_mst_level_dev(a[0], a[1], C.c_size_t(n), C.c_uint32(nc), a[2], a[3], s), L, f"level, null argument {hole}")
        _invalid(L.sg_mst_build_dev(a[0], a[1], C.c_uint32(1), C.c_uint32(nc), a[2], a[3], s), L, f"build, null argument {hole}")
    level_ok()
    build_ok()
    assert (_fetch(out, 2 * n, "refused calls") == 0x5A).all() and (_fetch(out2, 2 * n * nc, "refused calls") == 0x5A).all()


def test_refusals_of_the_inclusion_witness(gpu, O):
    """n_currencies 0 and 65, 65536 users, rows 0, depth 31, any null pointer: SG_ERR_INVALID and the advice buffer untouched;
    the valid call after each is right"""
    import torch
    ffi, L = _L()
    cfg = wc.config(1, 1, 8)
    tree = wc.witness_tree(cfg.levels, cfg.nc, "in_range", cfg.n_bytes)
    users_w, bal_w = wc.tree_words(tree)
    rc, h, b, (d_users, _) = _build(users_w, bal_w, cfg.levels, cfg.nc)
    ffi.check(rc)
    rows = 1 << cfg.k
    d_prog = torch.from_numpy(wc.program(cfg).view(np.int32).copy()).cuda()
    d_idx = torch.tensor([1, 0], dtype=torch.int32, device="cuda")
    adv = _out(2 * 3 * rows)
    want = np.concatenate([wc.mont(col) for idx in (1, 0) for col in wc.reference_columns(cfg, "in_range", idx)])
    p = ffi.dev_ptr
    good = dict(prog=p(d_prog), n_items=cfg.n_items, n_absorbs=cfg.n_absorbs, users=p(d_users), hashes=p(h), balances=p(b),
                depth=cfg.levels, nc=cfg.nc, idx=p(d_idx), n_users=2, advice=p(adv), rows=rows)

    def call(**change):
        a = dict(good, **change)
        return L.sg_mst_inclusion_witness_dev(a["prog"], C.c_uint32(a["n_items"]), C.c_uint32(a["n_absorbs"]), a["users"], a["hashes"],
                                              a["balances"], C.c_uint32(a["depth"]), C.c_uint32(a["nc"]), a["idx"], C.c_uint32(a["n_users"]),
                                              a["advice"], C.c_uint64(a["rows"]), ffi.current_stream_ptr())

    refused = [dict(nc=0), dict(nc=wc.NC_MAX + 1), dict(n_users=65536), dict(rows=0), dict(depth=31)]
    refused += [{name: None} for name in ("prog", "users", "hashes", "balances", "idx", "advice")]
    for change in refused:
        _invalid(call(**change), L, f"witness {change}")
        assert (_fetch(adv, 2 * 3 * rows, f"witness {change}") == 0x5A).all(), change
        ffi.check(call())
        _same(_fetch(adv, 2 * 3 * rows, f"witness after {change}"), want, f"witness after {change}")
        adv.fill_(0x5A)
