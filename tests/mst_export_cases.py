"""The snapshot CSVs a tree is written back out from, on the host (test_mst_export_cpu.py: the serial steps of csrc/mst_export.h
behind the reader's and the sort's) and on the device (test_gpu_mst_export.py), and the model both are compared with: the text's
definition in pure Python over rows of (name bytes, [integers]).

A case is (name, source text as bytes, n_currencies, delimiter, rows): the file a tree is built from and, in FILE order, the rows
the test chose -- the expected values, never values read back through the library.  A tree in file order writes `rows`, a sorted
tree `sorted_rows(rows)`.

The positions of the rows come from a sum per TILE = 64 rows, a scan per workgroup over GROUP = 256 tile sums and the groups'
totals, which a wave adds up LANES = 64 at a trip (MST_EXPORT_TILE, MST_EXPORT_GROUP and MST_EXPORT_THREADS of csrc/mst_export.h,
restated; the check program prints them): the edges are 64 and 16384 rows, and BIG is past the 2^20 rows whose 64 group totals
one trip adds up -- 65 totals, and a last tile of one row behind a full one."""
import numpy as np

from mst_csv_cases import header, write_case  # noqa: F401  (write_case: for the tests that import this module)
from mst_names_cases import fixed_rows, write_fixed

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
THREADS, TILE, GROUP, LANES = 256, 64, 256, 64
GROUP_ROWS = TILE * GROUP
TRIP_ROWS = LANES * GROUP_ROWS
BIG = TRIP_ROWS + TILE + 1
BIG_WIDTH = 7
NAME_CAP, MAX_DIGITS = 64, 77
MAX_ROW = NAME_CAP + 64 * (1 + MAX_DIGITS) + 1
SIZES = (63, 64, 65, GROUP_ROWS - 1, GROUP_ROWS, GROUP_ROWS + 1)
EDGE_VALUES = ([0, 1, 9] + [10 ** k - 1 for k in range(1, 77)] + [10 ** k for k in range(1, 77)]
               + [2 ** 32 - 1, 2 ** 32, 2 ** 64 - 1, 2 ** 64, R - 1, 10 ** 9, 10 ** 18 + 1, 7 * 10 ** 27, 10 ** 27 + 10 ** 9, R // 3])


def body_of(rows, delim: str = ",") -> bytes:
    """THE MODEL: one row per named leaf -- the name's bytes, for each currency the delimiter and the canonical integer in [0, r) in
    decimal, a line feed"""
    d = delim.encode()
    return b"".join(name + b"".join(d + str(v % R).encode() for v in bal) + b"\n" for name, bal in rows)


def offsets_of(rows):
    """every row's start in the body, and the body's length"""
    lengths = [len(name) + sum(1 + len(str(v % R)) for v in bal) + 1 for name, bal in rows]
    starts = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return starts[:-1].tolist(), int(starts[-1])


def sorted_rows(rows):
    """the leaves of a sorted tree: by the names' bytes, equal names in file order"""
    return sorted(rows, key=lambda row: row[0])


def text_of(rows, nc: int, delim: str = ",", eol: str = "\n", final: bool = True, show=str) -> bytes:
    """a source file of `rows`: `show` writes a balance (str: canonical)"""
    lines = [delim.join([name.decode()] + [show(v) for v in bal]) for name, bal in rows]
    text = header(nc, delim, eol) + eol.join(lines) + (eol if final else "")
    return text.encode()


def varied(n: int, nc: int = 2, tag: int = 0):
    """n distinct names of 2 to 19 bytes and balances of 1 to 20 digits: the rows start at every offset mod 16"""
    rows = []
    for i in range(n):
        name = f"u{i}".encode() + b"x" * ((i * 5 + tag) % 13)
        rows.append((name, [((i + 1) * 2654435761 + c * 40503) % 10 ** (1 + (i + 5 * c + tag) % 20) for c in range(nc)]))
    return rows


def cases():
    out = []

    def add(name, rows, nc, delim=",", text=None):
        out.append((name, text_of(rows, nc, delim) if text is None else text, nc, delim, rows))

    add("one_row_zero", [(b"a", [0])], 1)
    add("empty_name", [(b"alice", [1, 2]), (b"", [3, 4]), (b"bob", [5, 0])], 2)
    add("name_64_bytes", [(b"n" * 64, [7, 8]), (b"m" * 63, [9, 10]), (b"o" * 64, [0, 0])], 2)
    add("one_currency", varied(37, 1), 1)
    add("two_currencies", varied(41, 2, 3), 2)
    # the longest row: 64 bytes of name, 64 balances of 77 digits each
    longest = [(bytes([ord("a") + i]) * 64, [R - 1 - 1000 * i - c for c in range(64)]) for i in range(3)]
    assert all(len(str(v)) == MAX_DIGITS for _, bal in longest for v in bal)
    assert max(len(row) for row in body_of(longest).split(b"\n")) + 1 == MAX_ROW
    add("sixty_four_currencies_longest_rows", longest, 64)
    # 10^k - 1 and 10^k for every k, the word edges, r - 1, all-zero inner chunks
    add("powers_of_ten", [(f"p{k}".encode(), [10 ** k - 1, 10 ** k]) for k in range(1, 77)], 2)
    words = [2 ** 32 - 1, 2 ** 32, 2 ** 64 - 1, 2 ** 64, R - 1, 10 ** 9, 10 ** 18 + 1, 7 * 10 ** 27, 10 ** 27 + 10 ** 9, 0, 1, 10 ** 18]
    add("word_edges_and_zero_chunks", [(f"w{i}".encode(), words[2 * i:2 * i + 2]) for i in range(len(words) // 2)], 2)
    # what the source text may hold and the output does not keep
    few = varied(9, 2, 1)
    add("leading_zeros", few, 2, text=text_of(few, 2, show=lambda v: "00" + str(v)))
    over = [(b"a", [R + 5, 1]), (b"b", [2 * R, R]), (b"c", [R - 1, 10 ** 80 + 3])]
    add("values_at_or_above_r", over, 2)
    add("crlf", few, 2, text=text_of(few, 2, eol="\r\n"))
    add("no_final_newline", few, 2, text=text_of(few, 2, final=False))
    add("semicolon", few, 2, delim=";")
    add("semicolon_names_with_commas", [(b"a,b", [1, 2]), (b",", [3, 4])], 2, delim=";")
    dup = [(b"bob", [1, 2]), (b"alice", [3, 4]), (b"bob", [5, 6]), (b"carol", [7, 8]), (b"bob", [9, 10]), (b"alice", [11, 12])]
    add("duplicate_names", dup, 2)
    for n in SIZES:
        add(f"varied_{n}", varied(n, 2, n), 2)
    names = [c[0] for c in out]
    assert len(set(names)) == len(names)
    return out


def canonical(case) -> bool:
    """does a tree in file order give this source back byte for byte?"""
    name, text, nc, delim, rows = case
    return text == header(nc, delim).encode() + body_of(rows, delim)


# ----------------------------------------------------------------------------- past 64 groups: numpy and fixed-width text
def big_case(n: int = BIG):
    """(keys, balances [n, 2]): n distinct 7-digit names in a seeded permutation, balances of one digit -- short rows: what the big
    case is about is where they start"""
    seed = int.from_bytes(f"mst_export_cases.big.{n}".encode(), "little") % (1 << 63)
    keys = np.random.default_rng(seed).permutation(n).astype(np.int64)
    rows = np.arange(n, dtype=np.int64)
    return keys, np.stack([rows % 10, (rows // 7 + 3) % 10], axis=1)


def big_body(keys, bal, sorted_tree: bool) -> np.ndarray:
    """the model of the big case: rows of one width, canonical as they stand -> uint8"""
    order = np.argsort(keys, kind="stable") if sorted_tree else np.arange(keys.size)
    return fixed_rows(keys[order], BIG_WIDTH, list(bal[order].T), 1)


def write_big(path, keys, bal):
    return write_fixed(path, bal.shape[1], fixed_rows(keys, BIG_WIDTH, list(bal.T), 1))
