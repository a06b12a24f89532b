"""The host-side geometry of csrc/poly_plan.h restated in Python (the blocks of the prefix product, the Kate division and the grand
products, the width of the Kate scan, the levels of either evaluation path, the mid-sum reduction of the linear combination), the
input generators, and the list of cases that tests/test_gpu_poly_edges.py runs against the oracle.  tests/test_poly_cases_cpu.py
compares the restatement with the compiled rules (tests/cpp/poly_plan_check.cpp), checks the generators against the oracle and asserts that the case list
reaches every class of launch -- without a GPU."""
import numpy as np

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
MONT = 1 << 256

PP_CH, PP_THREADS = 8, 256
PP_BLOCK = PP_CH * PP_THREADS
KD_CH, KD_THREADS = 8, 256
KD_BLOCK = KD_CH * KD_THREADS
BI_CH = 8
EV_THREADS, EV_CH = 256, 32
EV_BATCH_CH_SMALL, EV_BATCH_CH_BIG, EV_BATCH_SMALL_MAX = 16, 32, 1 << 24
EVAL_BATCH_MAX = 40
LINCOMB_MAX, LINCOMB_LOW_MAX = 32, 8
KATE_BATCH_MAX, GRAND_MAX = 16, 8
KATE_POWERS_BYTES = (1 + 8 + 10) * 9 * 4     # b, b^(8 * 2^j) for j < 8, b^(2048 * 2^j) for j < 10, nine limbs each
SCAN_MAX = 1024                  # one workgroup scans the per-block values
FAST_ABOVE = 1 << 17             # longer random vectors come from fast_words


def _ceil(a, b):
    return (a + b - 1) // b


# ----------------------------------------------------------------------------- geometry
def prefix_blocks(n, count_out):
    """blocks of poly_prefix_product (None: refused): the blocks kernel covers a[0..n), the write kernel out[0..count_out)"""
    span = max(n, count_out)
    if count_out > n + 1 or span > SCAN_MAX * PP_BLOCK:
        return None
    return _ceil(span, PP_BLOCK)


def prefix_blocks_before_the_fix(n, count_out):
    nblk = _ceil(n + 1, PP_BLOCK)
    return None if nblk > SCAN_MAX or count_out > n + 1 else nblk


def grand_blocks(n):
    """blocks per product of poly_grand_products: n rows are read and n written"""
    nblk = _ceil(n, PP_BLOCK)
    return None if nblk > SCAN_MAX else nblk


def kate_blocks(n):
    nblk = _ceil(n, KD_BLOCK)
    return None if nblk > SCAN_MAX else nblk


def kate_scan_threads(nblk):
    """the power of two >= nblk, at least 64 (one block: no scan launch at all)"""
    t = 64
    while t < nblk:
        t <<= 1
    return t


def eval_levels(n):
    """the single path: elements read by each launch, until one workgroup is left"""
    per, out = EV_CH * EV_THREADS, [n]
    while _ceil(out[-1], per) > 1:
        out.append(_ceil(out[-1], per))
    return out


def eval_batch_plan(n, m):
    """the batched path: (coefficients per thread, partials per polynomial, launches of at most EVAL_BATCH_MAX); None: refused"""
    ch = EV_BATCH_CH_SMALL if n <= EV_BATCH_SMALL_MAX else EV_BATCH_CH_BIG
    blocks = _ceil(n, ch * EV_THREADS)
    if n == 0 or n > 1 << 26 or blocks > ch * EV_THREADS:
        return None
    return ch, blocks, [min(EVAL_BATCH_MAX, m - f) for f in range(0, m, EVAL_BATCH_MAX)]


def plan_constants():
    """the first line of tests/cpp/poly_plan_check.cpp"""
    c = dict(PP_CH=PP_CH, PP_THREADS=PP_THREADS, PP_BLOCK=PP_BLOCK, KD_CH=KD_CH, KD_THREADS=KD_THREADS, KD_BLOCK=KD_BLOCK, BI_CH=BI_CH,
             EV_THREADS=EV_THREADS, EV_CH=EV_CH, EV_LOG=(EV_CH * EV_THREADS).bit_length() - 1, EVAL_BATCH_MAX=EVAL_BATCH_MAX,
             EVAL_BATCH_SMALL_MAX=EV_BATCH_SMALL_MAX, EVAL_BATCH_MAX_N=(EV_BATCH_CH_BIG * EV_THREADS) ** 2, POLY_SCAN_MAX=SCAN_MAX,
             PREFIX_MAX_SPAN=SCAN_MAX * PP_BLOCK, KATE_MAX_N=SCAN_MAX * KD_BLOCK, KATE_BATCH_MAX=KATE_BATCH_MAX, KATE_POWERS_BYTES=KATE_POWERS_BYTES,
             GRAND_MAX=GRAND_MAX, GRAND_MAX_K=(SCAN_MAX * PP_BLOCK).bit_length() - 1, LINCOMB_MAX=LINCOMB_MAX, LINCOMB_LOW_MAX=LINCOMB_LOW_MAX,
             LINCOMB_SETS_MAX=8, LINCOMB_SETS_POLYS=48, LINCOMB_SETS_LOW=4)
    return " ".join(f"{k}={v}" for k, v in c.items())


def plan_line(n, m):
    """what tests/cpp/poly_plan_check.cpp answers to `size n m`, from the rules above and the work-space sizes restated here"""
    f = lambda v: "none" if v is None else str(v)
    kb, batch = kate_blocks(n), eval_batch_plan(n, m)
    ch = EV_BATCH_CH_SMALL if n <= EV_BATCH_SMALL_MAX else EV_BATCH_CH_BIG
    partials = _ceil(n, ch * EV_THREADS)
    launches = ",".join(str(min(EVAL_BATCH_MAX, m - first)) for first in range(0, m, EVAL_BATCH_MAX)) or "-"
    return (f"size n={n} m={m} prefix={f(prefix_blocks(n, n + 1))} prefix_rows={f(prefix_blocks(n, n))} prefix_tmp={_ceil(n + 1, PP_BLOCK) + 1} "
            f"grand={f(grand_blocks(n))} grand_mod={m * n} grand_tmp={m * _ceil(n + 1, PP_BLOCK) + 1} kate={f(kb)} "
            f"kate_scan={kate_scan_threads(kb) if kb is not None and kb > 1 else '-'} kate_tmp={SCAN_MAX + 1} kate_batch_tmp={m * _ceil(n, KD_BLOCK) + 1} "
            f"kate_batch_powers={m * KATE_POWERS_BYTES} eval_levels={','.join(map(str, eval_levels(n))) if n else '-'} "
            f"eval_tmp={_ceil(n, EV_CH * EV_THREADS) + 1} batch_ch={batch[0] if batch else '-'} batch_blocks={f(batch and batch[1])} "
            f"batch_partials={partials} batch_tmp={EVAL_BATCH_MAX * (partials + 1)} batch_launches={launches}")


def lincomb_mid_reductions(m):
    """the terms after which the lazy sum is reduced on the way: the pair that starts at an index = 30 (mod 32)"""
    return [j + 1 for j in range(0, m, 2) if j & 31 == 30]


# ----------------------------------------------------------------------------- inputs
VECTOR_CLASSES = ("random", "zero", "one", "max", "ramp", "first", "last")
SCALARS = ("random", 0, 1, R - 1)


def to_words(values):
    """integers -> 32-byte little-endian words, as they are (no Montgomery conversion)"""
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), dtype=np.uint8).copy()


def mont(values):
    """field values -> Montgomery words"""
    return to_words([v % R * MONT % R for v in values])


def value_of(word):
    """one 32-byte word (any 256-bit value) -> the field value it stands for"""
    return int.from_bytes(bytes(word), "little") * pow(MONT, -1, R) % R


def fast_words(seed, n):
    """n uniform words below 2^253 < r: canonical Montgomery words of field elements, at numpy's speed"""
    w = np.random.default_rng(seed).integers(0, 256, size=(n, 32), dtype=np.uint8)
    w[:, 31] &= 0x1F
    return w.reshape(-1)


def random_words(O, seed, n):
    return O.random_fr(seed, n) if n <= FAST_ABOVE else fast_words(seed, n)


def single_value(seed):
    """the value of the one non-zero element of `first` / `last`"""
    return 0x1234567 + seed


def vector(O, name, n, seed):
    """n Montgomery words of one input class"""
    if name == "random":
        return random_words(O, seed, n)
    if name == "zero":
        return np.zeros(32 * n, dtype=np.uint8)
    if name == "one":
        return np.tile(mont([1]), n)
    if name == "max":
        return np.tile(to_words([R - 1]), n)
    if name == "ramp":
        return to_words([R - 1 - i for i in range(n)])
    assert name in ("first", "last"), name
    v = np.zeros(32 * n, dtype=np.uint8)
    if n:
        at = 0 if name == "first" else n - 1
        v[32 * at:32 * at + 32] = mont([single_value(seed)])
    return v


def scalar(O, name, seed):
    """one Montgomery word: a random element, or the field value 0, 1 or r - 1"""
    return O.random_fr(seed, 1) if name == "random" else mont([name])


NONCANONICAL = (R, R + 1, (1 << 256) - 1)


def noncanonical_words(seed, n):
    """n words of which the first are r, r + 1 and 2^256 - 1, the last is 2^256 - 1 again and the rest uniform 256-bit values"""
    w = np.random.default_rng(seed).integers(0, 256, size=(n, 32), dtype=np.uint8)
    for i, v in enumerate(NONCANONICAL[:n]):
        w[i] = to_words([v])
    if n > len(NONCANONICAL):
        w[n - 1] = 0xFF
    return w.reshape(-1)


def reduced(words):
    """every 256-bit word reduced mod r (the same field values as canonical words), in Python integers"""
    b = bytes(words)
    return to_words([int.from_bytes(b[i:i + 32], "little") % R for i in range(0, len(b), 32)])


# ----------------------------------------------------------------------------- closed forms (field values, Python integers)
def eval_of_last(c, x, n):
    """the value at x of the polynomial whose only coefficient is c at degree n - 1"""
    return c * pow(x, n - 1, R) % R


def kate_of_last(c, b, n, i):
    """quotient coefficient i (< n - 1) of c X^(n-1) by (X - b); i = -1: the remainder"""
    return c * pow(b, n - 2 - i, R) % R


def eval_of_tiled(p_full, p_tail, x, L, n):
    """the value at x of the polynomial of n coefficients that repeats a period of L: P(x) (x^(Lq) - 1) / (x^L - 1) +
    x^(Lq) P_tail(x), with P the period's and P_tail the value of its first n mod L coefficients (x^L != 1)"""
    q, xl = n // L, pow(x, L, R)
    xlq = pow(xl, q, R)
    assert xl != 1
    return (p_full * (xlq - 1) * pow(xl - 1, -1, R) + xlq * p_tail) % R


# ----------------------------------------------------------------------------- the cases of tests/test_gpu_poly_edges.py
PREFIX_SIZES = (0, 1, 7, 8, 9, 2047, 2048, 2049, 4096, (1 << 17) + 1, (1 << 21) - 1)
PREFIX_REFUSED = 1 << 21
PREFIX_CLASSES, LARGE_CLASSES = ("random", "one", "max", "first"), ("random", "max")

INVERT_SIZES = (1, 7, 8, 9, 2047, 2048, 2049, (1 << 17) + 3)
INVERT_VALUES = ("random", "one", "max")
ZERO_PATTERNS = ("none", "all", "each position", "whole chunk", "tail", "alternating")


def zero_rows(pattern, n):
    """the rows a zero pattern clears in a vector of n elements (chunks of BI_CH)"""
    chunks = _ceil(n, BI_CH)
    if pattern == "none":
        return []
    if pattern == "all":
        return list(range(n))
    if pattern == "each position":         # position p of chunk c_p, eight different chunks where the vector has them
        step = max(1, chunks // BI_CH)
        return sorted({r for p in range(BI_CH) for r in [min(p * step, chunks - 1) * BI_CH + p] if r < n})
    if pattern == "whole chunk":           # the middle chunk, live chunks on either side where the vector has them
        c = chunks // 2
        return [r for r in range(c * BI_CH, (c + 1) * BI_CH) if r < n]
    if pattern == "tail":                  # the last element: inside the short chunk when n is no multiple of 8
        return [n - 1]
    assert pattern == "alternating", pattern
    return list(range(0, n, 2))


KATE_BLOCK_COUNTS = (2, 64, 65, 128, 129, 256, 257, 512, 513, 1024)
KATE_SIZES = tuple(sorted({KD_BLOCK * b for b in KATE_BLOCK_COUNTS} | {KD_BLOCK * (b - 1) + 1 for b in KATE_BLOCK_COUNTS}))
KATE_REFUSED = (1 << 21) + 1
KATE_CLASSES, KATE_LARGE_CLASSES = ("random", "zero", "max", "last"), ("random", "last")
KATE_ALL_CLASSES_UP_TO = KD_BLOCK * 65
KATE_BATCH_BLOCKS = (65, 1024)


# one block (no carries, one launch) and two blocks (the first carry): the paths the single and the batched division share
# now that both run one body.  n = 1 (a constant: empty quotient, the remainder is the constant) is accepted by the oracle.
KATE_SMALL_SIZES = (1, 2, 2047, 2048)
KATE_SMALL_CLASSES, KATE_SMALL_POINTS = ("random", "last"), ("random", R - 1)
KATE_BATCH_SMALL_SIZES = (1, 2, 2048, 2049, 4096)
KATE_BATCH_M = (1, 16)                   # 16: every division reads the one input, at sixteen different points
# the grid on which tests/test_poly_cases_cpu.py compares the restated rules with the compiled ones, beside the case lists
PLAN_EDGE_BLOCKS = (1, 2, 64, 128, 256, 512, 1024)
PLAN_EVAL_EDGES = ((1 << 24) - 1, (1 << 24) + 1, (1 << 26) - 1, (1 << 26) + 1)


def kate_classes(n):
    return KATE_CLASSES if n <= KATE_ALL_CLASSES_UP_TO else KATE_LARGE_CLASSES


EVAL_SIZES = (8191, 8192, 8193, 2 * 8192 + 1, (1 << 21) + 1)
EVAL_CLASSES = ("random", "max", "last")
EVAL_NONCANONICAL_SIZES = (8191, 8193)
EVAL_BATCH_SHAPES = ((4096, 1), (4097, 40), (4097, 41), ((1 << 20) + 1, 3))
EVAL_BATCH_TILED = (1 << 24, (1 << 24) + 1)        # m = 2 sharing one device buffer
EVAL_TILE_PERIOD = 4099
EVAL_BATCH_REFUSED = (1 << 26) + 1
EVAL_BATCH_NONCANONICAL = 4097

LINCOMB_M = (0, 1, 2, 3, 30, 31, 32)
LINCOMB_N = (1, 255, 256, 257)
LINCOMB_N_LOW = (0, 1, 8, "n")
LINCOMB_CLASSES = ("random", "max", "noncanonical")
MUL_SIZES = (255, 256, 257)

# single products: (what, k or n)
PRODUCT_CASES = (("permutation", 11), ("permutation", 21), ("lookup", (1 << 21) - 1), ("permutation vanishing", 11), ("lookup vanishing", 2048))
# batched: (k, (columns per permutation chunk), lookups, usable rows, vanishing denominators: False or which rows)
GRAND_CASES = (
    (18, (2, 1), 1, (1 << 18) - 6, False),
    (20, (1,), 1, (1 << 20) - 6, False),
    (21, (1,), 0, (1 << 21) - 6, False),
    (11, (2, 1), 1, 2048 - 6, "rows"),
    (11, (2, 1), 1, 2048 - 6, "late rows"),
    (12, (1, 1), 1, 0, False),
    (12, (1, 1), 1, 4095, False),
    (12, (1, 1), 1, 2048, False),
)


def vanishing_rows(n, which="rows"):
    """three rows, the first and the last among them; "late rows": without row 0, so that z is not zero from row 1 on"""
    return (0, n // 2 + 1, n - 1)[which == "late rows":]


def reached():
    """every class of launch the case list above runs, by name (tests/test_poly_cases_cpu.py asserts the full set)"""
    seen = set()
    for n in PREFIX_SIZES:
        nblk = prefix_blocks(n, n + 1)
        assert nblk is not None, n
        seen.add("prefix: one block" if nblk == 1 else "prefix: several blocks")
        if n and n % PP_BLOCK == 0:
            seen.add("prefix: out[n] alone in an extra block")
        if nblk == SCAN_MAX:
            seen.add("prefix: 1024 blocks")
    if prefix_blocks(PREFIX_REFUSED, PREFIX_REFUSED + 1) is None and prefix_blocks(PREFIX_REFUSED - 1, PREFIX_REFUSED) == SCAN_MAX:
        seen.add("prefix: first refused size")
    for n in INVERT_SIZES:
        seen.add("invert: short tail chunk" if n % BI_CH else "invert: whole chunks")
        if n > 256 * BI_CH:
            seen.add("invert: several workgroups")
        for pat in ZERO_PATTERNS:
            rows = zero_rows(pat, n)
            if pat == "each position" and {r % BI_CH for r in rows} == set(range(BI_CH)) and len({r // BI_CH for r in rows}) == BI_CH:
                seen.add("invert: a zero at each position, eight chunks")
            if pat == "whole chunk" and len(rows) == BI_CH and rows[0] >= BI_CH and rows[-1] + BI_CH < n:
                seen.add("invert: a chunk of zeros between live chunks")
            if pat == "tail" and n % BI_CH and rows == [n - 1]:
                seen.add("invert: a zero in the short tail chunk")
            if pat in ("none", "all", "alternating"):
                seen.add("invert: " + pat)
    for n in KATE_SIZES:
        nblk = kate_blocks(n)
        assert nblk is not None and nblk > 1, n
        t = kate_scan_threads(nblk)
        if nblk == t:
            seen.add(f"kate: scan of {t} threads, exactly full")
        if nblk == t // 2 + 1 or (t == 64 and nblk == 2):      # (the narrowest scan is entered with the second block)
            seen.add(f"kate: scan of {t} threads, just entered")
        if n % KD_BLOCK == 1:
            seen.add("kate: one coefficient in the last block")
        if nblk == SCAN_MAX and n % KD_BLOCK == 0:
            seen.add("kate: 1024 full blocks")
        seen.update(f"kate: class {c} at {'small' if n <= KATE_ALL_CLASSES_UP_TO else 'large'} sizes" for c in kate_classes(n))
    if kate_blocks(KATE_REFUSED) is None and kate_blocks(KATE_REFUSED - 1) == SCAN_MAX:
        seen.add("kate: first refused size")
    for b in KATE_BATCH_BLOCKS:
        seen.add(f"kate batch: scan of {kate_scan_threads(b)} threads")
    if {kate_blocks(n) for n in KATE_SMALL_SIZES} == {1}:
        seen.add("kate: one block")
    for n in KATE_BATCH_SMALL_SIZES:
        if kate_blocks(n) in (1, 2):
            seen.add("kate batch: one block" if kate_blocks(n) == 1 else "kate batch: two blocks")
    if max(KATE_BATCH_M) == KATE_BATCH_MAX:
        seen.add("kate batch: 16 divisions")
    for n in EVAL_SIZES:
        lv = eval_levels(n)
        seen.add(f"eval: {len(lv)} level{'s' * (len(lv) > 1)}")
        if n % (EV_CH * EV_THREADS) == 1 and len(lv) > 1:
            seen.add("eval: one coefficient in the last workgroup")
        if len(lv) > 1 and lv[1] > EV_THREADS:
            seen.add("eval: a thread of the second level has two rows")
    for n, m in EVAL_BATCH_SHAPES + tuple((n, 2) for n in EVAL_BATCH_TILED):
        ch, blocks, launches = eval_batch_plan(n, m)
        seen.add(f"eval batch: {ch} per thread")
        seen.add("eval batch: one partial" if blocks == 1 else "eval batch: several partials")
        if ch == EV_BATCH_CH_SMALL and blocks == ch * EV_THREADS:
            seen.add("eval batch: the last full second level of the 16-per-thread kernel")
        if len(launches) > 1:
            seen.add("eval batch: more than 40 polynomials")
        if launches[0] == EVAL_BATCH_MAX:
            seen.add("eval batch: 40 in one launch")
    if eval_batch_plan(EVAL_BATCH_REFUSED, 1) is None and eval_batch_plan(EVAL_BATCH_REFUSED - 1, 1) is not None:
        seen.add("eval batch: first refused size")
    for m in LINCOMB_M:
        seen.add("lincomb: low polynomial alone" if m == 0 else "lincomb: odd term count" if m % 2 else "lincomb: even term count")
        if lincomb_mid_reductions(m) == [31]:
            seen.add(f"lincomb: mid-sum reduction, {m} terms")
        if m == 30:
            assert not lincomb_mid_reductions(m)
            seen.add("lincomb: the longest sum without a mid-sum reduction")
    for n in LINCOMB_N + MUL_SIZES:
        seen.add("rows: one workgroup" if n <= 256 else "rows: two workgroups")
        if n % 256:
            seen.add("rows: ragged last workgroup")
    for what, size in PRODUCT_CASES:
        n = 1 << size if what.startswith("permutation") else size
        nblk = prefix_blocks(n, n)
        assert nblk is not None, (what, size)
        seen.add(f"{what}: {'1024' if nblk == SCAN_MAX else 'one' if nblk == 1 else 'several'} block{'s' * (nblk > 1)}")
        if nblk == SCAN_MAX and prefix_blocks_before_the_fix(n, n) is None:
            seen.add(f"{what}: refused before the fix")
    for k, chunks, lookups, usable, vanishing in GRAND_CASES:
        n = 1 << k
        assert grand_blocks(n) is not None and usable < n
        seen.add(f"grand: k = {k}")
        if len(chunks) > 1:
            seen.add("grand: a chunk continues the one before")
        if vanishing:
            seen.add("grand: vanishing denominators")
        if usable in (0, n - 1) or usable % PP_BLOCK == 0:
            seen.add("grand: usable rows " + ("0" if usable == 0 else "n - 1" if usable == n - 1 else "on a block boundary"))
    return seen


WANTED = {
    "prefix: one block", "prefix: several blocks", "prefix: out[n] alone in an extra block", "prefix: 1024 blocks", "prefix: first refused size",
    "invert: short tail chunk", "invert: whole chunks", "invert: several workgroups", "invert: a zero at each position, eight chunks",
    "invert: a chunk of zeros between live chunks", "invert: a zero in the short tail chunk", "invert: none", "invert: all", "invert: alternating",
    *(f"kate: scan of {t} threads, {f}" for t in (64, 128, 256, 512, 1024) for f in ("exactly full", "just entered")),
    "kate: one coefficient in the last block", "kate: 1024 full blocks", "kate: first refused size",
    *(f"kate: class {c} at small sizes" for c in KATE_CLASSES), *(f"kate: class {c} at large sizes" for c in KATE_LARGE_CLASSES),
    "kate batch: scan of 128 threads", "kate batch: scan of 1024 threads",
    "kate: one block", "kate batch: one block", "kate batch: two blocks", "kate batch: 16 divisions",
    "eval: 1 level", "eval: 2 levels", "eval: one coefficient in the last workgroup", "eval: a thread of the second level has two rows",
    "eval batch: 16 per thread", "eval batch: 32 per thread", "eval batch: one partial", "eval batch: several partials",
    "eval batch: the last full second level of the 16-per-thread kernel", "eval batch: more than 40 polynomials", "eval batch: 40 in one launch",
    "eval batch: first refused size",
    "lincomb: low polynomial alone", "lincomb: odd term count", "lincomb: even term count", "lincomb: mid-sum reduction, 31 terms",
    "lincomb: mid-sum reduction, 32 terms", "lincomb: the longest sum without a mid-sum reduction",
    "rows: one workgroup", "rows: two workgroups", "rows: ragged last workgroup",
    "permutation: one block", "permutation: 1024 blocks", "permutation: refused before the fix", "lookup: 1024 blocks",
    "permutation vanishing: one block", "lookup vanishing: one block",
    *(f"grand: k = {k}" for k in (11, 18, 20, 21)), "grand: a chunk continues the one before", "grand: vanishing denominators",
    "grand: usable rows 0", "grand: usable rows n - 1", "grand: usable rows on a block boundary",
}
