"""The cases that tests/test_gpu_witness.py runs against the kernels of csrc/witness.hip (the dense forms of mst_leaves_kernel and
mst_level_kernel, mst_inclusion_witness_kernel, reached through csrc/abi_mst.hip's sg_mst_leaves_dev / sg_mst_level_dev / sg_mst_build_dev /
sg_mst_inclusion_witness_dev): the sizes around the 128-thread blocks of the tree kernels and the 64-thread x-blocks of the
witness kernel, the input generators (edge values of the field, words >= r, child balances whose sums wrap mod r, trees with
balances in and out of the range check's range) and a plain-integer interpreter of the witness program, which restates what
the kernel has to write.  tests/test_witness_cases_cpu.py checks all of it without a GPU: the generators do what they claim,
the case lists reach every class of launch, the oracle agrees with Python integers, and the interpreter agrees with
mst_inclusion.reference_assignment on every cell.  Numpy and Python integers only."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

import poly_cases as pc

R = pc.R
MONT = pc.MONT
TREE_THREADS = 128          # mst_leaves_kernel, mst_level_kernel: one hash per thread
WITNESS_THREADS = 64        # mst_inclusion_witness_kernel: one program item per thread, blockIdx.y = the user
NC_MAX = 64                 # the C ABI's bound on n_currencies
PERMUTE_ROWS = 37           # a "permute state" region; the state after the permutation is at offset 36

to_words, mont, value_of = pc.to_words, pc.mont, pc.value_of


def edge_values():
    """canonical field values around the byte, 64-bit word and modulus boundaries"""
    return [0, 1, 0xFF, 0x100, (1 << 56) - 1, 1 << 56, (1 << 64) - 1, 1 << 64, (1 << 64) + 5, (1 << 72) - 1, 1 << 253, (R - 1) // 2,
            R - 2, R - 1]


def vector(name, n, seed):
    """n Montgomery words of one input class: `random` canonical words; `edges` the edge values, then random canonical words;
    `noncanonical` words >= r (r, r + 1, 2^256 - 1 first) between uniform 256-bit words"""
    if name == "random":
        return pc.fast_words(seed, n)
    if name == "edges":
        e = edge_values()[:n]
        return np.concatenate([mont(e), pc.fast_words(seed, n - len(e))])
    if name == "noncanonical":
        return pc.noncanonical_words(seed, n)
    raise ValueError(name)


def values_of(words):
    """Montgomery words (any 256-bit values) -> the field values they stand for"""
    b = bytes(words)
    inv = pow(MONT, -1, R)
    return [int.from_bytes(b[i:i + 32], "little") * inv % R for i in range(0, len(b), 32)]


def is_canonical(words):
    b = bytes(words)
    return all(int.from_bytes(b[i:i + 32], "little") < R for i in range(0, len(b), 32))


# ----------------------------------------------------------------------------- sizes
LEAF_SIZES = [1, 63, 64, 65, 127, 128, 129, 257]
LEVEL_PARENTS = [1, 2, 63, 64, 65, 127, 128, 129]
NC = [1, 2, 3]
WIDE_NC, WIDE_N = [63, 64], 129
LEAF_CASES = [(n, nc) for n in LEAF_SIZES for nc in NC] + [(WIDE_N, nc) for nc in WIDE_NC]
LEVEL_CASES = [(m, nc) for m in LEVEL_PARENTS for nc in NC] + [(WIDE_N, nc) for nc in WIDE_NC]
BUILD_DEPTHS = [0, 1, 7, 8]
NONCANONICAL_LEAVES = (8, 2)       # n, nc: 8 hashes of 3 words in Python integers
NONCANONICAL_LEVEL = (4, 2)        # parents, nc: 4 hashes of 4 words


def launch_classes(n, threads):
    """where n falls against the blocks of a one-item-per-thread launch (the threads behind n leave after the staging barrier)"""
    out = {"below one block" if n < threads else "one block" if n == threads else "several blocks"}
    if n > threads and n % threads == 1:
        out.add("one past a block")
    return out


# ----------------------------------------------------------------------------- child balances whose sums wrap
WRAP_PAIRS = {
    "wraps far": (R - 1, R - 1),                        # 2r - 2 -> r - 2
    "wraps to zero": (R - 1, 1),                        # r -> 0
    "largest without a wrap": (R - 1, 0),
    "zero": (0, 0),
    "carry across the 64-bit word": ((1 << 64) - 1, (1 << 64) - 1),
    "carry into the next word": ((1 << 64) - 1, 1),     # 2^64
}


def wrapping_pairs(nc, m):
    """[(parent, lane, left, right)] for a level of m parents: the six pairs of WRAP_PAIRS on distinct (parent, lane) slots, the
    corners first (first parent and first lane, last parent and last lane, first parent and last lane, last parent and first
    lane), then down the parents; the pair on the first slot rotates with m + nc, so that over the case list every pair stands
    on every corner.  A level with fewer than six slots takes as many pairs as it has slots; one with twelve has each twice."""
    slots = []
    for s in [(0, 0), (m - 1, nc - 1), (0, nc - 1), (m - 1, 0)] + [(p, p % nc) for p in range(1, m - 1)]:
        if s not in slots:
            slots.append(s)
    pairs = list(WRAP_PAIRS.values())
    return [(p, lane) + pairs[(i + m + nc) % len(pairs)] for i, (p, lane) in enumerate(slots[:2 * len(pairs)])]


def wrap_class(left, right):
    for name, pair in WRAP_PAIRS.items():
        if pair == (left, right):
            return name
    return None


def level_children(m, nc, seed):
    """child hashes (2 m words, edge values first) and child balances (2 m nc random words with the wrapping pairs planted)"""
    child_hash = vector("edges", 2 * m, seed)
    bal = vector("random", 2 * m * nc, seed + 1).reshape(2 * m, nc, 32).copy()
    for p, lane, left, right in wrapping_pairs(nc, m):
        bal[2 * p, lane] = mont([left])
        bal[2 * p + 1, lane] = mont([right])
    return child_hash, bal.reshape(-1)


def leaf_inputs(name, n, nc, seed):
    """usernames (n words) and balances (n nc words) of one input class"""
    return vector(name, n, seed), vector(name, n * nc, seed + 1)


# ----------------------------------------------------------------------------- expected hashes and sums
def expected_leaves(O, users, balances, nc, canonical=True):
    """leaf hashes: the C oracle for canonical words; Python integers of every word reduced mod r otherwise (the oracle is
    defined on canonical words only)"""
    if canonical:
        return O.mst_leaves(users, balances, nc)
    from oracle import pyref as P
    u, b = values_of(users), values_of(balances)
    return mont([P.poseidon_hash([u[i]] + b[i * nc:(i + 1) * nc]) for i in range(len(u))])


def expected_level(O, child_hash, child_bal, nc, canonical=True):
    """(parent hashes, parent balances)"""
    if canonical:
        return O.mst_level(child_hash, child_bal, nc)
    from oracle import pyref as P
    h, b = values_of(child_hash), values_of(child_bal)
    hashes, sums = [], []
    for p in range(len(h) // 2):
        s = [(b[2 * p * nc + c] + b[(2 * p + 1) * nc + c]) % R for c in range(nc)]
        sums += s
        hashes.append(P.poseidon_hash(s + [h[2 * p], h[2 * p + 1]]))
    return mont(hashes), mont(sums)


def expected_tree(O, users, leaf_bal, depth, nc):
    """level-major node hashes and balances of the tree over 2^depth leaves: the leaves, then O.mst_level again and again"""
    hs, bs = [O.mst_leaves(users, leaf_bal, nc)], [np.array(leaf_bal)]
    for _ in range(depth):
        h, b = O.mst_level(hs[-1], bs[-1], nc)
        hs.append(h)
        bs.append(b)
    return np.concatenate(hs), np.concatenate(bs), hs, bs


# ----------------------------------------------------------------------------- the witness program
WITNESS_CONFIGS = [(1, 1, 8), (2, 2, 1), (2, 2, 31), (2, 3, 8), (3, 2, 8), (4, 2, 8), (1, NC_MAX, 8)]     # (levels, nc, n_bytes)
Config = namedtuple("Config", "levels nc n_bytes k n_items n_absorbs rows_used")


@lru_cache(maxsize=None)
def config(levels, nc, n_bytes):
    """the smallest k with rows_used + BLINDING_FACTORS + 1 <= 2^k, and the program's sizes, all from witness_program"""
    from circuits_halo2_amd import mst_inclusion as M
    for k in range(4, 26):
        try:
            _, n_items, n_absorbs, _, rows_used = M.witness_program(k, levels, nc, n_bytes)
        except ValueError:          # "the circuit does not fit 2^k rows"
            continue
        assert rows_used + M.BLINDING_FACTORS + 1 <= 1 << k
        return Config(levels, nc, n_bytes, k, n_items, n_absorbs, rows_used)
    raise ValueError("no k fits")


def witness_configs():
    return [config(*s) for s in WITNESS_CONFIGS]


def program(cfg):
    from circuits_halo2_amd import mst_inclusion as M
    return M.witness_program(cfg.k, cfg.levels, cfg.nc, cfg.n_bytes)[0]


def sponge_digests(levels):
    """(level, sibling?) of the node every sponge of the program ends in, in the program's order: the user's leaf, then per
    level the path's sibling and the next node of the path"""
    out = [(0, False)]
    for level in range(levels):
        out += [(level, True), (level + 1, False)]
    return out


Tree = namedtuple("Tree", "levels nc users node_hash node_bal")      # integers; node_hash[level][i], node_bal[level][i][c]
TREE_KINDS = ("in_range", "out_of_range")


def _build(users, leaf_bal):
    from oracle import pyref as P
    nc = len(leaf_bal[0])
    node_hash, node_bal = [[P.poseidon_hash([u] + b) for u, b in zip(users, leaf_bal)]], [leaf_bal]
    while len(node_hash[-1]) > 1:
        hs, bs = node_hash[-1], node_bal[-1]
        sums = [[(bs[2 * p][c] + bs[2 * p + 1][c]) % R for c in range(nc)] for p in range(len(hs) // 2)]
        node_hash.append([P.poseidon_hash(sums[p] + [hs[2 * p], hs[2 * p + 1]]) for p in range(len(sums))])
        node_bal.append(sums)
    return node_hash, node_bal


@lru_cache(maxsize=None)
def witness_tree(levels, nc, kind, n_bytes=8):
    """A tree of 2^levels leaves as integers.  Usernames: 0, 1, r - 1, r - 2, then random values (a tree of two leaves takes
    two of the four, starting at the nc-th).

    `in_range`: every balance a range check sees is below 2^(8 n_bytes).  An even currency c holds 2^(8 n_bytes) - 1 (every
    byte 0xff) at leaf c / 2 and zeros elsewhere (every byte 0x00), so its sums stay in range up to the root; an odd currency
    holds the edge values below 2^(8 n_bytes) for as long as their total stays in range, from leaf c on.

    `out_of_range`: the same, and planted over it
      2^(8 n_bytes) and 2^(8 n_bytes) + 5 at leaves 0 and 1 of currency 0 (a leaf and its sibling out of range),
      r - 1 beside 1 (their parent's balance wraps to 0),
      2^(8 n_bytes) - 1 beside 1: two in-range siblings whose sum leaves the range at level 1 (a node that the users of the
      neighbouring pair check as their level-1 sibling);
    with four leaves or more the second pair stands at the last two leaves of currency 0 and the third at leaves 2 and 3 of
    currency 1, in a tree of two leaves they stand in currencies 1 and 2.  The one-currency tree of two leaves has two
    balances in all: it takes 2^(8 n_bytes) + 5 and r - 1."""
    assert kind in TREE_KINDS
    size, top = 1 << levels, 1 << (8 * n_bytes)
    rng = np.random.default_rng(1000 * levels + nc)
    special = [0, 1, R - 1, R - 2]
    if size == 2:
        special = special[nc % 4:] + special[:nc % 4]
    users = (special + [int.from_bytes(rng.bytes(32), "little") % R for _ in range(size)])[:size]
    bal = [[0] * nc for _ in range(size)]
    small = [v for v in edge_values() if 0 < v < top - 1]
    for c in range(nc):
        if c % 2 == 0:
            bal[(c // 2) % size][c] = top - 1
        else:
            total = 0
            for j, v in enumerate(small[:size]):
                if total + v < top:
                    bal[(c + j) % size][c] = v
                    total += v
    if kind == "out_of_range":
        if size * nc == 2:
            plants = [(0, 0, top + 5), (1, 0, R - 1)]
        elif size == 2:
            plants = [(0, 0, top), (1, 0, top + 5), (0, 1, R - 1), (1, 1, 1), (0, 2, top - 1), (1, 2, 1)]
        else:
            plants = [(0, 0, top), (1, 0, top + 5), (size - 2, 0, 1), (size - 1, 0, R - 1), (2, 1, top - 1), (3, 1, 1)]
            plants += [(i, 1, 0) for i in range(size) if i not in (2, 3)]       # currency 1: nothing else beside the pair
        for leaf, c, v in plants:
            if c < nc:
                bal[leaf][c] = v
    node_hash, node_bal = _build(users, bal)
    return Tree(levels, nc, users, node_hash, node_bal)


def witness_users(levels):
    """all 2^levels indices, then the same reversed, with one duplicate"""
    size = 1 << levels
    return list(range(size)) + list(reversed(range(size))) + [size // 2]


def tree_words(tree):
    """(usernames, leaf balances) as Montgomery words, what sg_mst_build_dev takes"""
    return mont(tree.users), mont([b for leaf in tree.node_bal[0] for b in leaf])


def symbol_value(tree, symbol, idx):
    """the value a witness-program symbol names for leaf idx (csrc/witness.hip: sym_words)"""
    kind, level, mode, lane = symbol & 15, (symbol >> 4) & 63, (symbol >> 10) & 7, (symbol >> 13) & 127
    at = idx >> level
    if kind == 0:
        return tree.users[idx ^ (mode & 1)]
    if kind == 3:
        return at & 1
    child = lane & 1 if kind == 1 else 0          # for a balance the lane is the currency
    node, lv = at, level
    if mode == 1:
        node = at ^ 1
    elif mode == 2:
        node, lv = 2 * (at ^ 1) + child, level - 1
    elif mode == 3:
        node = (at & ~1) + child
    return tree.node_hash[lv][node] if kind == 1 else tree.node_bal[lv][node][lane]


def range_checked(cfg, tree, idx):
    """[(symbol, value)] of the range checks of leaf idx's circuit"""
    prog = program(cfg)
    return [(int(s), symbol_value(tree, int(s), idx)) for kind, _, _, s, _ in prog[:5 * cfg.n_items].reshape(-1, 5) if kind == 1]


def run_program(prog, n_items, tree, idx, rows, range_rows=lambda n_bytes: n_bytes + 1):
    """The witness program in plain integers: the three advice columns (rows values each, zero where nothing is written) that
    mst_inclusion_witness_kernel has to produce for leaf idx.
      kind 0  one cell: the symbol's value
      kind 1  a range check: the N_BYTES + 1 running sums value >> 8 i in column 0 (the last one is what is left of a value of
              more than N_BYTES bytes)
      kind 2  a sponge: the initial state (0, count 2^64); per absorbed word the add-input rows (state; word; state + word)
              and the 37 permute rows -- the state before each of the first four full rounds, before each of the 28 pairs of
              partial rounds (column 2: the first s-box output of the pair), before each of the last four full rounds, and
              after the permutation -- recomputed round by round
    range_rows: the number of running sums per range check; tests/test_witness_cases_cpu.py passes N_BYTES to show where the
    columns would differ if the last one were left out"""
    from oracle import pyref as P
    rcs, mds, _ = P._poseidon_params()
    items = np.asarray(prog[:5 * n_items]).reshape(-1, 5).tolist()
    absorbs = np.asarray(prog[5 * n_items:]).reshape(-1, 3).tolist()
    adv = [[0] * rows for _ in range(3)]
    mix = lambda a, b: ((mds[0][0] * a + mds[0][1] * b) % R, (mds[1][0] * a + mds[1][1] * b) % R)
    full = lambda a, b, r: mix(pow((a + rcs[r][0]) % R, 5, R), pow((b + rcs[r][1]) % R, 5, R))
    for kind, col, row, symbol, extra in items:
        if kind == 0:
            adv[col][row] = symbol_value(tree, symbol, idx)
        elif kind == 1:
            v = symbol_value(tree, symbol, idx)
            for b in range(range_rows(extra)):
                adv[0][row + b] = v >> (8 * b)
        else:
            first, count = extra & 0xFFFFF, (extra >> 20) & 255
            s0, s1 = 0, (count << 64) % R
            adv[0][row], adv[1][row] = s0, s1
            for add_row, permute_row, symbol in absorbs[first:first + count]:
                w = symbol_value(tree, symbol, idx)
                adv[0][add_row], adv[1][add_row] = s0, s1
                adv[0][add_row + 1] = w
                s0 = (s0 + w) % R
                adv[0][add_row + 2], adv[1][add_row + 2] = s0, s1
                at, r = permute_row, 0
                for _ in range(4):
                    adv[0][at], adv[1][at] = s0, s1
                    s0, s1 = full(s0, s1, r)
                    at, r = at + 1, r + 1
                for _ in range(28):
                    adv[0][at], adv[1][at] = s0, s1
                    sbox = pow((s0 + rcs[r][0]) % R, 5, R)
                    adv[2][at] = sbox
                    s0, s1 = mix(sbox, (s1 + rcs[r][1]) % R)
                    s0, s1 = mix(pow((s0 + rcs[r + 1][0]) % R, 5, R), (s1 + rcs[r + 1][1]) % R)
                    at, r = at + 1, r + 2
                for _ in range(4):
                    adv[0][at], adv[1][at] = s0, s1
                    s0, s1 = full(s0, s1, r)
                    at, r = at + 1, r + 1
                adv[0][at], adv[1][at] = s0, s1
                assert at == permute_row + PERMUTE_ROWS - 1 and r == 64
    return adv


_REFERENCE = {}


def reference_columns(cfg, kind, idx):
    """the three advice columns of mst_inclusion.reference_assignment(lenient=True), what api.MstInclusionCircuit.synthesize
    lays out, for leaf idx of witness_tree(kind); computed once and shared (read only)"""
    key = (cfg, kind, idx)
    if key not in _REFERENCE:
        _REFERENCE[key] = reference(cfg, kind, idx)["advice"]
    return _REFERENCE[key]


def reference(cfg, kind, idx, instances=None):
    from circuits_halo2_amd import mst_inclusion as M
    t = witness_tree(cfg.levels, cfg.nc, kind, cfg.n_bytes)
    sib = idx ^ 1
    pre_mid = []
    for level in range(1, cfg.levels):
        s = (idx >> level) ^ 1
        pre_mid.append(t.node_bal[level][s] + [t.node_hash[level - 1][2 * s], t.node_hash[level - 1][2 * s + 1]])
    return M.reference_assignment(cfg.k, t.users[idx], t.node_bal[0][idx], [(idx >> l) & 1 for l in range(cfg.levels)],
                                  [t.users[sib]] + t.node_bal[0][sib], pre_mid, cfg.n_bytes, lenient=True, instances=instances)
