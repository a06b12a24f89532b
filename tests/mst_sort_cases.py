"""The fixed list of snapshot CSVs the device sort of the usernames is checked with, on the host (test_mst_sort_cpu.py: the steps of
csrc/mst_sort.h run serially) and on the device (test_gpu_mst_sort.py).  Every case is (name, text or golden file name,
n_currencies, refusal): refusal None for a file the device sorts -- the leaves must come out in Python's stable order of the
names' bytes -- or the (row, code) it must report.  `tile` is the rows a workgroup ranks in one pass (MST_SORT_TILE, from
ss_mst_sort_geometry): the sizes sit at its edges, and the duplicates lie more than a tile apart.  Balances are distinct in
every generated file, so that the file order of equal names shows in the leaves."""
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


def stable_order(names):
    """the file rows in leaf order: Python's sort is stable"""
    return sorted(range(len(names)), key=lambda i: names[i])
