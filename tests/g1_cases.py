"""The launch geometry of csrc/g1_ops.hip restated in Python (block sizes, the level sizes of g1_prefix_sums), the input generators
and the list of cases that tests/test_gpu_g1_ops.py runs against the oracle: fixed-base products, the FFT over G1, the prefix
sums and window tables of a basis, the on-curve check and the scalar half of the KZG set-up (kzg_setup_scalars, csrc/summa_gpu.hip).

Every input point is s * G for a scalar s known here, so every expected point is e * G for an e computed in Fr, and -- G having
prime order r -- two points are equal, opposite or the identity exactly when their scalars are.  That is what lets
tests/test_g1_cases_cpu.py assert, from the scalars alone and without a GPU, that the cases reach the doubling, cancelling and
identity branches of every kernel at the stage or level they are meant to."""
import random

import numpy as np

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583
MONT = 1 << 256
S_ADICITY = 28
ROOT_OF_UNITY = 0x03DDB9F5166D18B798865EA93DD31F743215CF6DD39329C8D34F1ED960C37C9C

PFX_CHUNK = 32                  # elements per thread of g1_prefix_chunks
BLOCK_256 = 256                 # g1_fixed_base_mul, g1_on_curve_kernel
BLOCK_128 = 128                 # g1fft_*, g1_prefix_*, msm_table_step, kzg_setup_scalars


# ----------------------------------------------------------------------------- words
def mont(values):
    """integers -> 32-byte little-endian Montgomery words (one numpy buffer)"""
    return np.frombuffer(b"".join(((v % R) * MONT % R).to_bytes(32, "little") for v in values), dtype=np.uint8).copy()


def raw_words(words):
    """integers below 2^256 -> their 32 little-endian bytes, unchanged"""
    return np.frombuffer(b"".join(w.to_bytes(32, "little") for w in words), dtype=np.uint8).copy()


def unreduced(values):
    """the Montgomery words m~ of `values` as m~ + r: the same residues, not reduced (r < 2^254, so the sum fits 256 bits)"""
    words = [(v % R) * MONT % R + R for v in values]
    assert all(R <= w < MONT for w in words)
    return raw_words(words)


def omega(k):
    return pow(ROOT_OF_UNITY, 1 << (S_ADICITY - k), R)


def randoms(seed, n, nonzero=True):
    rng = random.Random(seed)
    return [rng.randrange(1 if nonzero else 0, R) for _ in range(n)]


def add_kind(a, b):
    """what the group law meets in a + b, from the scalars of the two points"""
    a, b = a % R, b % R
    kinds = set()
    if a == 0:
        kinds.add("a_identity")
    if b == 0:
        kinds.add("b_identity")
    if a and b:
        kinds.add("double" if a == b else "cancel" if (a + b) % R == 0 else "generic")
    return kinds


# ----------------------------------------------------------------------------- 1: fixed-base products
FIXED_BASE_SIZES = (1, 255, 256, 257, 513)       # below, at and past one and two blocks of 256 threads


def fixed_base_edges():
    """(name, scalar): 0, the ends of the field, the halves, every single bit of the word-shifting loop, full low words"""
    e = [("0", 0), ("1", 1), ("2", 2), ("r-1", R - 1), ("r-2", R - 2), ("(r-1)/2", (R - 1) // 2), ("(r+1)/2", (R + 1) // 2)]
    e += [(f"2^{b}", 1 << b) for b in range(254)]
    e += [(f"2^{32 * j}-1", (1 << (32 * j)) - 1) for j in range(1, 8)]
    return e


FIXED_BASE_EDGES_ALONE = (0, 1, 2, R - 1, R - 2, (R - 1) // 2, (R + 1) // 2, 1 << 31, 1 << 32, 1 << 253, (1 << 224) - 1)


def fixed_base_vectors(n, seed=1):
    """vectors of n scalars that between them hold every edge value; each keeps its edge values at the END (the last element of
    the last block is always one) behind random ones.  n = 1 is a launch per value: the named values, the bits next to a word
    boundary, the top bit and the longest run of ones, each alone -- the sizes from 255 on hold all of them"""
    edges = [v for _, v in fixed_base_edges()] if n >= BLOCK_256 - 1 else list(FIXED_BASE_EDGES_ALONE)
    out = []
    for first in range(0, len(edges), n):
        tail = edges[first:first + n]
        out.append(randoms(seed + first, n - len(tail)) + tail)
    return out


def fixed_base_unreduced_values(seed=2):
    """257 values whose Montgomery words are fed as m~ + r; the answer is that of the reduced twin"""
    edges = [v for _, v in fixed_base_edges()]
    return randoms(seed, 257 - 17) + edges[:7] + [1 << b for b in (0, 31, 32, 63, 64, 128, 252, 253)] + edges[-2:]


# ----------------------------------------------------------------------------- 2: FFT over G1
FFT_LOGS = (0, 1, 2, 3, 5, 8)                    # no stage at all ... two blocks of 128 butterflies
FFT_ROOTS = ("omega", "omega_inv")
FFT_SCALES = ("none", "n_inv", "one", "zero")    # none: scale == NULL
FFT_PATTERNS = ("random", "equal", "alternating", "half_negated", "upper_zero", "single", "late_equal")


def fft_root(name, log_n):
    w = omega(log_n)
    return w if name == "omega" else pow(w, -1, R)


def fft_scale(name, log_n):
    """the factor, or None for scale == NULL"""
    return {"none": None, "n_inv": pow(1 << log_n, -1, R), "one": 1, "zero": 0}[name]


def fft_scalars(pattern, log_n, root="omega", seed=3):
    n = 1 << log_n
    s = randoms(seed + log_n, n)
    a = s[0]
    if pattern == "equal":
        s = [a] * n
    elif pattern == "alternating":
        s = [a if i % 2 == 0 else R - a for i in range(n)]
    elif pattern == "half_negated":              # s[i + n/2] = -s[i]: the operands of stage 0 are opposite
        s = s[:n // 2] + [R - v for v in s[:n // 2]] if n > 1 else s
    elif pattern == "upper_zero":
        s = [v if i < max(1, n // 2) else 0 for i, v in enumerate(s)]
    elif pattern == "single":
        s = [a if i == min(1, n - 1) else 0 for i in range(n)]
    elif pattern == "late_equal" and log_n >= 2:
        # stage 1, butterfly j = 1 of block 0: u = s[0] - s[n/2], v = s[n/4] - s[3n/4], twiddle w^(n/4); make w^(n/4) v == u
        w = fft_root(root, log_n)
        s[0] = (s[n // 2] + pow(w, n // 4, R) * (s[n // 4] - s[3 * n // 4])) % R
    return s


def bitrev(i, bits):
    return int(bin(i)[2:].zfill(bits)[::-1], 2) if bits else 0


def fft_trace(s, w, log_n):
    """g1_fft on the scalars, butterfly by butterfly as g1fft_stage runs them -> (result, {(stage, kind, twiddled)}) where kind
    is what u + (twiddled v) meets (add_kind); u - v then meets the mirror image: a doubling for a cancellation and back"""
    n = 1 << log_n
    a = [0] * n
    for i, v in enumerate(s):
        a[bitrev(i, log_n)] = v % R
    seen = set()
    for st in range(log_n):
        h = 1 << st
        for q in range(n // 2):
            j, blk = q & (h - 1), q >> st
            i0 = (blk << (st + 1)) + j
            i1 = i0 + h
            u, v = a[i0], a[i1]
            if j:
                v = v * pow(w, j << (log_n - st - 1), R) % R
            seen |= {(st, kind, j > 0) for kind in add_kind(u, v)}
            a[i0], a[i1] = (u + v) % R, (u - v) % R
    return a, seen


def fft_claims(pattern, log_n):
    """(stage, kind, twiddled) entries that fft_trace must report for the pattern at this size"""
    c = []
    if pattern == "equal" and log_n >= 1:
        c.append((0, "double", False))                     # u + v doubles, u - v cancels
        if log_n >= 2:
            c += [(1, "double", False), (1, "a_identity", True), (1, "b_identity", True)]    # the cancelled halves travel on
    if pattern == "alternating" and log_n >= 1:
        c.append((log_n - 1, "cancel", False))             # sum of the even rows against the sum of the odd ones
        if log_n >= 2:
            c.append((0, "double", False))
    if pattern == "half_negated" and log_n >= 1:
        c.append((0, "cancel", False))                     # u + v cancels, u - v doubles
    if pattern == "upper_zero" and log_n >= 1:
        c.append((0, "b_identity", False))
    if pattern == "single" and log_n >= 1:
        c.append((log_n - 1, "a_identity", False))
        if log_n >= 2:
            c += [(0, "b_identity", False), (log_n - 1, "a_identity", True)]     # ... and a scalar multiplication of the identity
    if pattern == "late_equal" and log_n >= 2:
        c.append((1, "double", True))
    return c


FFT_ALL_SCALES = ("random", "single")               # the scale only meets the outputs (g1fft_store): generic ones and identities


def fft_cases():
    """(log_n, root, scale, pattern): every pattern with both roots, without a scale and with 1/n; every scale on the two
    patterns of FFT_ALL_SCALES"""
    return [(log_n, root, scale, pattern) for log_n in FFT_LOGS for pattern in FFT_PATTERNS for root in FFT_ROOTS
            for scale in (FFT_SCALES if pattern in FFT_ALL_SCALES else FFT_SCALES[:2])]


# ----------------------------------------------------------------------------- 3: prefix sums and window tables
def prefix_levels(n):
    """level sizes of g1_prefix_sums: n, ceil(n / 32), ... down to at most one chunk"""
    size = [n]
    while size[-1] > PFX_CHUNK:
        size.append((size[-1] + PFX_CHUNK - 1) // PFX_CHUNK)
    return size


PREFIX_KS = {4: [16], 5: [32], 6: [64, 2], 10: [1024, 32], 11: [2048, 64, 2], 16: [65536, 2048, 64, 2]}
PREFIX_PATTERNS = ("random", "equal", "alternating", "zeros", "cancel32")


def prefix_scalars(pattern, k, seed=5):
    n = 1 << k
    s = randoms(seed + k, n)
    a = s[0]
    if pattern == "equal":
        s = [a] * n
    elif pattern == "alternating":
        s = [a if i % 2 == 0 else R - a for i in range(n)]
    elif pattern == "zeros":                       # identity inputs: first and last of a chunk, a whole chunk, scattered
        for i in range(n):
            if i % 7 == 3 or i in (0, 31, 32, n - 1) or 64 <= i < 96:
                s[i] = 0
    elif pattern == "cancel32" and n > 32:         # Q_32 = O
        s[32] = (-sum(s[:32])) % R
    return s


def prefix_probe_rows(n):
    return sorted({j for j in (0, 31, 32, 33, 1023, 1024, 1025, n - 1) if j < n})


def running_sums(s):
    out, acc = [], 0
    for v in s:
        acc = (acc + v) % R
        out.append(acc)
    return out


def prefix_trace(s):
    """g1_prefix_sums on the scalars, kernel by kernel -> (Q, {(where, kind)}), where = chunks0 (madd of an affine input),
    chunks1 (the scan of chunk totals, every upper level), apply, store"""
    size = prefix_levels(len(s))
    seen = set()
    lvl = [[v % R for v in s]]
    for l in range(len(size)):
        run, totals = lvl[l], []
        for first in range(0, size[l], PFX_CHUNK):
            acc = 0
            for i in range(first, min(size[l], first + PFX_CHUNK)):
                seen |= {("chunks0" if l == 0 else "chunks1", kind) for kind in add_kind(acc, run[i])}
                acc = (acc + run[i]) % R
                run[i] = acc
            totals.append(acc)
        if l + 1 < len(size):
            assert len(totals) == size[l + 1]
            lvl.append(totals)
    for l in range(len(size) - 2, 0, -1):
        for i in range(PFX_CHUNK, size[l]):
            seen |= {("apply", kind) for kind in add_kind(lvl[l][i], lvl[l + 1][i // PFX_CHUNK - 1])}
            lvl[l][i] = (lvl[l][i] + lvl[l + 1][i // PFX_CHUNK - 1]) % R
    out = list(lvl[0])
    if len(size) > 1:
        for i in range(PFX_CHUNK, size[0]):
            seen |= {("store", kind) for kind in add_kind(out[i], lvl[1][i // PFX_CHUNK - 1])}
            out[i] = (out[i] + lvl[1][i // PFX_CHUNK - 1]) % R
    return out, seen


def prefix_claims(pattern, k):
    levels = len(PREFIX_KS[k])
    c = []
    if pattern == "equal":
        c.append(("chunks0", "double"))
        if levels >= 2:
            c += [("chunks1", "double"), ("store", "double")]
        if levels >= 3:
            c.append(("apply", "double"))
    if pattern == "alternating":
        c += [("chunks0", "cancel"), ("chunks0", "a_identity")]
        if levels >= 2:
            c += [("chunks1", "b_identity"), ("store", "b_identity")]
    if pattern == "zeros":
        c.append(("chunks0", "b_identity"))
    if pattern == "cancel32" and levels >= 2:
        c.append(("store", "cancel"))
    return c


def step_column(j, n):
    """1 on rows 0..j, 0 after: its difference-form commitment is Q_j alone"""
    col = np.zeros((n, 32), dtype=np.uint8)
    col[:j + 1] = mont([1])
    return col.reshape(-1)


def piecewise_values(n, seed=6):
    """a piecewise-constant column: runs of 1, 2, 31, 32, 33, ... rows, a run of zeros among them"""
    rng = random.Random(seed)
    out, run = [], [1, 2, 31, 32, 33, 5]
    while len(out) < n:
        for length in run:
            out += [rng.randrange(R) if len(out) % 3 else 0] * length
    return out[:n]


# the smallest k stays 5: sg_commit* reads the table whenever one exists (no routing to the one-launch MSM), which the GPU test
# asserts through the launch log
TABLE_KS = (5, 11)
TABLE_WINDOW_BITS = (4, 7, 13, 16, 0)            # 0: the library's choice for the size
TABLE_BITS = tuple(range(254))


def window_widths(c):
    """make_window_plan: W windows of c bits, the top one c - 1, the slack taken from the windows under it"""
    W = (255 + c - 1) // c
    width = [c] * (W - 1) + [c - 1]
    for i in range(W * c - 255):
        width[W - 2 - i] -= 1
    assert sum(width) == 254
    return width


def default_window_bits(n):
    return min(16, max(4, n.bit_length() - 1))


def table_row_of_bit(c, b):
    offset = 0
    for w, width in enumerate(window_widths(c)):
        if b < offset + width:
            return w
        offset += width
    raise AssertionError(b)


def table_basis_scalars(k, basis, seed=7):
    """basis 0 (g): identities and repeated points among the bases; basis 1 (g_lagrange): generic points"""
    n = 1 << k
    t = randoms(seed + 2 * k + basis, n)
    if basis == 0:
        for i in range(n):
            if i % 5 == 2:
                t[i] = 0
            elif i % 5 == 4:
                t[i] = t[1]
            elif i % 11 == 0:
                t[i] = R - t[1]
    return t


def table_bit_row(b, n):
    """the row that holds 2^b in the b-th single-entry column"""
    return (7 * b + 3) % n


# ----------------------------------------------------------------------------- 4: on-curve check
CURVE_KS = (1, 8, 9)                             # two points, exactly one block of 256, two blocks


def curve_scalars(k, seed=8):
    """(g, g_lagrange) scalars of a good SRS: generic points, identities, and P beside -P"""
    n = 1 << k
    out = []
    for b in (0, 1):
        s = randoms(seed + 2 * k + b, n)
        for i in range(n):
            if i % 9 == 4:
                s[i] = 0
            elif i % 9 == 7:
                s[i] = R - s[i - 1]
        out.append(s)
    return out


def fq_words(b):
    return int.from_bytes(bytes(b), "little")


def spoil(point, how):
    """a 64-byte point that the check must refuse, made from a good one that is not the identity"""
    x, y = fq_words(point[:32]), fq_words(point[32:])
    assert x or y
    if how == "y+1":
        y = (y + MONT) % Q                        # Montgomery words of y + 1
    elif how == "swap":
        x, y = y, x
    elif how == "x+q":
        x += Q                                    # the same residue, words not below q (q < 2^254: still 256 bits)
    elif how == "y+q":
        y += Q
    else:
        raise ValueError(how)
    return raw_words([x, y])


SPOILS = ("y+1", "swap", "x+q", "y+q")


def curve_cases():
    """(name, k, [(basis, index, how)]): the points to spoil; the check must report exactly as many"""
    cases = []
    for k in CURVE_KS:
        n = 1 << k
        cases.append((f"k={k} good", k, []))
        for basis in (0, 1):
            for idx in sorted({0, min(255, n - 1), n - 1}):
                for how in SPOILS:
                    cases.append((f"k={k} basis {basis} [{idx}] {how}", k, [(basis, idx, how)]))
    k, n = 9, 512
    spread = [i for i in range(n) if i % 9 != 4][::3][:150]           # both blocks, never an identity
    many = [(basis, idx, SPOILS[(m + basis) % 4]) for basis in (0, 1) for m, idx in enumerate(spread)]
    assert len({(b, i) for b, i, _ in many}) == 300
    cases.append(("k=9 300 bad points", k, many))
    assert all(idx % 9 != 4 for _, _, spoiled in cases for _, idx, _ in spoiled)   # curve_scalars: those are the identities
    return cases


# ----------------------------------------------------------------------------- 5: KZG set-up
SETUP_KS = (0, 1, 5, 8)


def setup_taus(k, seed=9):
    """(name, tau).  1, r - 1 = omega^(n/2) (k >= 1) and omega^3 are points of the domain: L_j(tau) is 1 for one j, 0 elsewhere"""
    taus = [("random", randoms(seed + k, 1)[0]), ("0", 0), ("1", 1), ("r-1", R - 1)]
    if k >= 2:
        taus.append(("omega^3", pow(omega(k), 3, R)))
    return taus


def lagrange_at(tau, k):
    """L_i(tau), i < 2^k, from the definition"""
    n, w = 1 << k, omega(k)
    tau %= R
    if pow(tau, n, R) == 1:
        return [1 if pow(w, i, R) == tau else 0 for i in range(n)]
    num = (pow(tau, n, R) - 1) * pow(n, -1, R) % R
    return [pow(w, i, R) * num * pow(tau - pow(w, i, R), -1, R) % R for i in range(n)]


def lagrange_as_the_kernel_had_it(tau, k):
    """omega^i (tau^n - 1) / (n (tau - omega^i)) with 1 / 0 = 0: what kzg_setup_scalars computed before it treated domain points"""
    n, w = 1 << k, omega(k)
    num = (pow(tau, n, R) - 1) % R
    inv = lambda v: pow(v, -1, R) if v % R else 0
    return [pow(w, i, R) * num * inv(n * (tau - pow(w, i, R))) % R for i in range(n)]
