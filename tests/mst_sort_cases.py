"""The fixed list of snapshot CSVs the device sort of the usernames is checked with, on the host (test_mst_sort_cpu.py: the steps of
csrc/mst_sort.h run serially) and on the device (test_gpu_mst_sort.py).  Every case is (name, text or golden file name,
n_currencies, refusal): refusal None for a file the device sorts -- the leaves must come out in Python's stable order of the
names' bytes -- or the (row, code) it must report.  `tile` is the rows a workgroup ranks in one pass (MST_SORT_TILE, from
ss_mst_sort_geometry): the sizes sit at its edges, and the duplicates lie more than a tile apart.  Balances are distinct in
every generated file, so that the file order of equal names shows in the leaves.  LARGE, a list of its own, names generated
files of 32768 rows and more (`large`): the sizes at which the one-workgroup scan of a pass takes one full step, a second and a
third, and the files in which a row's place depends on the sum a step carries into the next."""
import functools
import random

from mst_csv_cases import GOLDENS, header, write_case  # noqa: F401  (write_case: for the tests that import this module)

NAME_CAP = 64
NAME_TOO_LONG = 7
ALPHABET = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789"


def rows_text(names, nc: int = 2, delim: str = ",", eol: str = "\n") -> str:
    return "".join(delim.join([name] + [str(1000 * i + c + 1) for c in range(nc)]) + eol for i, name in enumerate(names))


def random_names(rng, n: int):
    return ["".join(rng.choice(ALPHABET) for _ in range(rng.randint(1, 12))) for _ in range(n)]


def cases(tile: int):
    rng = random.Random(20240607)
    h = header(2)
    out = []
    for n in (1, 2, 63, 64, 65, tile - 1, tile, tile + 1, 3 * tile + 5):
        out.append((f"random_{n}", h + rows_text(random_names(rng, n)), 2, None))
    out.append(("all_equal", h + rows_text(["same"] * 70), 2, None))                      # no pass runs: file order
    last = [f"sharedprefix{c}" for c in ALPHABET]
    first = [f"{c}sharedsuffix" for c in ALPHABET]
    rng.shuffle(last)
    rng.shuffle(first)
    out.append(("last_byte_differs", h + rows_text(last), 2, None))
    out.append(("first_byte_differs", h + rows_text(first), 2, None))
    chain = ["a" * k for k in range(NAME_CAP + 1)]                                        # "", "a", .., 64 bytes
    rng.shuffle(chain)
    out.append(("prefix_chain", h + rows_text(chain), 2, None))
    far = random_names(rng, 2 * tile + 10)
    for at in (3, tile + 7, 2 * tile + 5):
        far[at] = "dup"
    for at in (0, tile + 1, 2 * tile + 9):
        far[at] = "Zed"
    far[5] = far[tile + 5]                                                                # a random name twice, a tile apart
    out.append(("duplicates_a_tile_apart", h + rows_text(far), 2, None))
    ordered = sorted(set(random_names(rng, 100)), key=str.encode)
    out.append(("already_sorted", h + rows_text(ordered), 2, None))
    out.append(("reverse_sorted", h + rows_text(ordered[::-1]), 2, None))
    out.append(("bytes_01_and_7f", h + rows_text(["\x7f", "a\x7f", "\x01", "a", "a\x01", "\x01\x7f", "\x7f\x01", "a\x01\x01", "\x7f\x7f"]), 2, None))
    long64 = ["b" * NAME_CAP, "m", "a" * NAME_CAP, "b" * (NAME_CAP - 1) + "a", "z"]
    out.append(("name_of_64_bytes", h + rows_text(long64), 2, None))
    out.append(("name_of_65_bytes", h + rows_text(["m", "z", "c" * (NAME_CAP + 1), "a", "b" * (NAME_CAP + 2), "k"]), 2, (2, NAME_TOO_LONG)))
    semi = random_names(rng, 40)
    out.append(("semicolon", header(2, ";") + rows_text(semi, delim=";"), 2, None))
    out.append(("crlf", header(2, eol="\r\n") + rows_text(random_names(rng, 40), eol="\r\n"), 2, None))
    out += [(g[:-4], g, 2, None) for g in GOLDENS]
    names = [c[0] for c in out]
    assert len(set(names)) == len(names)
    return out


# ----------------------------------------------------------------------------- files beyond one step of a pass's scan
# A pass scans hist[digit][tile] with one workgroup, SCAN_ITEMS words a thread and step (MST_SORT_SCAN_BLOCK, MST_SORT_SCAN_ITEMS
# and MST_SORT_BINS of csrc/mst_sort.h, restated; the check program prints them): above 16 tiles -- 32768 rows -- a step's sum is
# carried into the next.  A step's words are the tiles of some digits: word digit * tiles + tile belongs to step
# (digit * tiles + tile) // 4096, and a row reads the word of its own digit alone.  Names inside the reader's subset hold no byte
# above 0x7f, so up to 32 tiles no row reads a word behind the first step; ALPHABET's highest byte, 'z', reads one from 34 tiles.
SCAN_BLOCK, SCAN_ITEMS, BINS = 1024, 4, 256
HIGH = "{|}~\x7f"                                # the bytes of the subset above 'z'


def tiles_of(n_rows: int, tile: int) -> int:
    return -(-n_rows // tile)


def scan_steps(n_rows: int, tile: int) -> int:
    return -(-BINS * tiles_of(n_rows, tile) // (SCAN_ITEMS * SCAN_BLOCK))


def steps_read(names, tile: int):
    """the steps of the scan whose words some row of the file reads in some pass: those of the digits -- the names' bytes and
    the zero that pads them -- whose tiles all lie in one step"""
    tiles = tiles_of(len(names), tile)
    digits = set(b"".join(names)) | {0}
    step = SCAN_ITEMS * SCAN_BLOCK
    return {d * tiles // step for d in digits if d * tiles // step == (d * tiles + tiles - 1) // step}


def rows_text_wide(names, eol: str = "\r\n") -> str:
    """two balances of 30 digits a row, distinct per row"""
    return "".join(f"{name},{10 ** 29 + 1000 * i + 1},{10 ** 29 + 1000 * i + 2}{eol}" for i, name in enumerate(names))


# the sizes at the edges of one, two and three steps, the 64-byte, pooled, skewed and prefix files, and two that read a carried sum
LARGE = ["rows_32768", "rows_32769", "rows_65537", "hex64_32769", "pool_300_32769", "skew_32769", "skew_tile0_32769",
         "prefix_tail_32769", "high_bytes_65537", "rows_196609"]


@functools.lru_cache(maxsize=None)
def large(name: str, tile: int):
    """(text, n_currencies) of a LARGE case: two currencies, balances distinct per row.
    rows_N             random names of 1 to 12 ALPHABET bytes: one full step (16 tiles), two steps, three steps
    hex64_32769        64 lowercase hex digits a name, 64 passes; 30-digit balances and "\\r\\n" make a row 128 bytes and the body
                       4 MiB + 128: the CSV reader's scan takes its second round in the same call
    pool_300_32769     300 names, each about a hundred times in all 17 tiles: every tile's offset decides where equal names go
    skew_32769         "samename" + 'a' in the first 16 tiles, another byte in the 17th; skew_tile0_32769: the other bytes in tile 0
    prefix_tail_32769  "a" * k, k = 0 .. 64, spread over all tiles among random names: the zero padding ranks them
    high_bytes_65537   33 tiles, names over ALPHABET and the five bytes above 'z': from '|' on their words lie in the second step
    rows_196609        97 tiles, seven steps: digits and capitals read the second step's words, small letters the third's"""
    n = int(name.rsplit("_", 1)[1])
    rng = random.Random(f"mst_sort_cases.large.{name}")
    h = header(2)
    if name.startswith("rows_"):
        names = random_names(rng, n)
    elif name == "hex64_32769":
        names = [rng.randbytes(32).hex() for _ in range(n)]
        return header(2, eol="\r\n") + rows_text_wide(names), 2
    elif name == "pool_300_32769":
        pool = sorted(set(random_names(rng, 400)))[:300]
        rng.shuffle(pool)
        names = [rng.choice(pool) for _ in range(n)]
        assert len(pool) == 300 and set(names) == set(pool)
    elif name in ("skew_32769", "skew_tile0_32769"):
        lo = 16 * tile if name == "skew_32769" else 0                # the tile whose rows cycle through ALPHABET, from 'b' on
        names = ["samename" + (ALPHABET[(i - lo + 1) % len(ALPHABET)] if lo <= i < lo + tile else "a") for i in range(n)]
    elif name == "prefix_tail_32769":
        names = random_names(rng, n)
        chain = list(range(NAME_CAP + 1))
        rng.shuffle(chain)
        for j, k in enumerate(chain):                                # about four of them in every tile, one in the last row
            names[n - 1 if j == NAME_CAP else (j * n) // len(chain) + 11] = "a" * k
    elif name == "high_bytes_65537":
        names = ["".join(rng.choice(ALPHABET + HIGH) for _ in range(rng.randint(1, 12))) for _ in range(n)]
    else:
        raise KeyError(name)
    return h + rows_text(names), 2


def names_of(text: str):
    """the names of a case's rows, as bytes"""
    eol = "\r\n" if text.index("\n") and text[text.index("\n") - 1] == "\r" else "\n"
    return [row.split(",", 1)[0].encode() for row in text.split(eol)[1:-1]]


def stable_order(names):
    """the file rows in leaf order: Python's sort is stable"""
    return sorted(range(len(names)), key=lambda i: names[i])
