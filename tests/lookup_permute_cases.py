"""Cases and the expected result for the general lookup permutation (sg_lookup_permute_dev, arithmetic.lookup_permute): helpers
shared by test_lookup_permute_cpu.py and test_gpu_lookup_permute.py, no tests of their own.

THE RULE, stated here with Python integers and nothing else: A' is the input sorted as integers.  Walking A' from the top, a
row whose value differs from the row above (a first row) takes one table row of that value; a value the table no longer holds
means the input is not in the table.  The table values left over are sorted as integers and go, smallest first, into the rows
that repeat the row above them, topmost first.  (prover.permute_expression_pair orders multi-limb leftovers low limb first and
upstream fills the repeated rows from the bottom: both valid, neither is the expectation here.)

Every generator returns (input, table) as (rows, 4) uint64 arrays of canonical little-endian limbs, read-only; case(...)
caches them together with the expected pair, so a reference is computed once however many tests use it."""
import collections
import functools

import numpy as np

from oracle.pyref import R

USABLE_17 = (1 << 17) - 6
MISSING = ("between", "above", "below", "top_word", "low_word")
# a fixed full-width value with bits 253..255 clear (so below r whatever one of its 32-bit words is replaced by)
_C = int.from_bytes(bytes((37 * i + 11) % 251 + 1 for i in range(32)), "little") & ((1 << 253) - 1)


def expected(inp_ints, table_ints):
    """-> (A', S') as lists of integers, or None when an input value is not in the table"""
    a = sorted(v % R for v in inp_ints)
    pool = collections.Counter(v % R for v in table_ints)
    s = [None] * len(a)
    for i, v in enumerate(a):
        if i == 0 or v != a[i - 1]:
            if pool[v] == 0:
                return None
            pool[v] -= 1
            s[i] = v
    leftovers = sorted(pool.elements())
    repeated = [i for i in range(len(a)) if s[i] is None]
    assert len(leftovers) == len(repeated)
    for i, v in zip(repeated, leftovers):
        s[i] = v
    return a, s


def to_ints(limbs):
    return [int.from_bytes(row.tobytes(), "little") for row in np.ascontiguousarray(limbs)]


def to_limbs(ints):
    out = np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in ints), dtype=np.uint64).reshape(-1, 4).copy()
    return out


def _random_below_r(rng, count):
    return [int.from_bytes(rng.bytes(32), "little") % R for _ in range(count)]


def _from_pool(rng, pool, rows):
    """the table cycles through the pool and is shuffled; the inputs are drawn from the table"""
    table = [pool[i % len(pool)] for i in range(rows)]
    rng.shuffle(table)
    inp = [table[i] for i in rng.integers(0, rows, rows)]
    if rows > 100:                                       # a long run of one value
        for i in rng.integers(0, rows, rows // 3):
            inp[i] = table[rows // 2]
    return inp, table


def wide(rows, d, seed):
    """a pool of max(d, 4) values below r: 0, 1, r - 1, r - 2 and random ones (a table shorter than the pool holds its head)"""
    rng = np.random.default_rng(seed)
    pool = [0, 1, R - 1, R - 2] + _random_below_r(rng, max(d, 4) - 4)
    return _from_pool(rng, pool, rows)


def one_word(rows, w, seed):
    """all keys agree outside 32-bit word w: word order, the compare direction, the rule that skips constant digits"""
    rng = np.random.default_rng(seed)
    base = _C & ~(0xffffffff << (32 * w))
    top = 1 << (29 if w == 7 else 32)                    # word 7 stays below 2^29: the value below 2^253
    words = sorted({int(j) for j in rng.integers(0, top, min(rows, 300))} | {0, top - 1})
    rng.shuffle(words)
    return _from_pool(rng, [base | (j << (32 * w)) for j in words], rows)


def equal(rows):
    return [_C] * rows, [_C] * rows


def bijection(rows, seed):
    rng = np.random.default_rng(seed)
    table = list(dict.fromkeys(_random_below_r(rng, rows)))
    assert len(table) == rows
    inp = list(table)
    rng.shuffle(inp)
    return inp, table


def range_table(rows, seed):
    """an 8-bit range table with repeats, built as test_gpu_round5_oracle._permute_case builds its 16-bit one"""
    rng = np.random.default_rng(seed)
    table = [(i * 7919 + seed) % 256 for i in range(rows)]
    inp = [table[i] for i in rng.integers(0, rows, rows)]
    if rows > 100:
        for i in rng.integers(0, rows, rows // 3):
            inp[i] = table[rows // 2]
    return inp, table


def word32(rows, seed):
    """one-limb values in [2^16, 2^32): the range-table path refuses them"""
    rng = np.random.default_rng(seed)
    pool = [(1 << 16) + (i * 2654435761 + seed) % ((1 << 32) - (1 << 16)) for i in range(min(rows, 500))] + [1 << 16, (1 << 32) - 1]
    return _from_pool(rng, pool, rows)


def missing(rows, variant, seed):
    """a valid case with one input row replaced by a value the table does not hold"""
    rng = np.random.default_rng(seed)
    inp, table = _from_pool(rng, _random_below_r(rng, 17), rows)
    have, ordered = set(table), sorted(set(table))
    if variant == "between":
        bad = next(lo + 1 for lo, hi in zip(ordered, ordered[1:]) if hi - lo > 1)
    elif variant == "above":
        bad = ordered[-1] + 1
    elif variant == "below":
        bad = ordered[0] - 1
    elif variant == "top_word":
        bad = next(v ^ (1 << 224) for v in ordered if (v ^ (1 << 224)) < R and (v ^ (1 << 224)) not in have)
    else:
        assert variant == "low_word"
        bad = next(v ^ 1 for v in ordered if (v ^ 1) not in have)
    assert 0 <= bad < R and bad not in have
    inp[rows // 3] = bad
    return inp, table


_GENERATORS = {"wide": wide, "one_word": one_word, "equal": equal, "bijection": bijection, "range": range_table, "word32": word32,
               "missing": missing}


@functools.lru_cache(maxsize=None)
def case(kind, rows, *args):
    """-> (input limbs, table limbs, expected): expected = (A' limbs, S' limbs) or None; all arrays read-only"""
    inp, table = _GENERATORS[kind](rows, *args)
    want = expected(inp, table)
    out = [to_limbs(inp), to_limbs(table)]
    if want is not None:
        want = (to_limbs(want[0]), to_limbs(want[1]))
        out += list(want)
    for a in out:
        a.setflags(write=False)
    return out[0], out[1], want


def describe(spec):
    return "-".join(str(x) for x in spec)
