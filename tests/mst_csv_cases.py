"""The two fixed lists of CSV files the device CSV reader is checked with, on the host (test_mst_csv_cpu.py: the four passes of
csrc/mst_csv.h run serially) and on the device (test_gpu_mst_csv.py).  ACCEPTED: files inside the reader's subset -- it must take
every one and find the fields `parse_csv_to_entries` finds.  REFUSED: files outside it, each with what the reader must
report: a flag of the scan, or the lowest offending row and its code.  `tile` and `cap` are the reader's geometry
(MST_CSV_TILE, MST_CSV_ROW_CAP): newlines and carriage returns are placed at the tile edges by the length of a name.
LARGE_ACCEPTED and LARGE_REFUSED, lists of their own, name generated files of 4 and 9 MiB (`large`): the bodies at which the
reader's one-workgroup scan takes exactly one full round, a second and a third."""
import functools
import os
import random

from conftest import GOLDEN

GOLDENS = ["entry_13.csv", "entry_16.csv", "entry_16_bigints.csv", "entry_16_modified.csv", "entry_16_overflow.csv",
           "entry_16_switched_order.csv", "entry_17.csv"]
FLAG_BYTE, FLAG_BARE_CR = 0x40000000, 0x80000000
ROW_TOO_LONG, ROW_EMPTY, ROW_DELIMITERS, ROW_EMPTY_BALANCE, ROW_NOT_DECIMAL = 1, 2, 3, 4, 5


def header(nc: int, delim: str = ",", eol: str = "\n") -> str:
    return delim.join(["username"] + [f"balance_C{c}_ETH" for c in range(nc)]) + eol


def few(first: int, count: int = 5, nc: int = 2, delim: str = ",", eol: str = "\n") -> str:
    return "".join(delim.join([f"user{i}"] + [str(1000 * i + c) for c in range(nc)]) + eol for i in range(first, first + count))


def accepted(tile: int, cap: int):
    """[(name, text or golden file name, n_currencies)]"""
    h = header(2)
    cases = [(g[:-4], g, 2) for g in GOLDENS]
    cases += [
        ("crlf", header(2, eol="\r\n") + few(0, 7, eol="\r\n"), 2),
        ("crlf_body_lf_header", h + few(0, 7, eol="\r\n"), 2),
        ("no_trailing_newline", h + few(0, 4) + "last,7,8", 2),
        ("semicolon", header(2, ";") + few(0, 6, delim=";"), 2),
        ("semicolon_names_with_commas", header(2, ";") + "a,b;1;2\n,;3;4\n", 2),
        ("empty_name", h + "a,1,2\n,5,6\nb,3,4\n", 2),
        ("digits80", h + "a," + "9" * 80 + ",1\nb,2," + "1" + "0" * 79 + "\n", 2),
        ("leading_zeros", h + "a,0005,000\nb,00,01\n", 2),
        ("nc1", header(1) + few(0, 9, nc=1), 1),
        ("nc4", header(4) + few(0, 9, nc=4), 4),
        ("one_row", h + "only,1,2\n", 2),
        ("one_row_open_end", h + "only,1,2", 2),
        ("blank_last_line", h + few(0, 3) + "\n", 2),
        ("blank_last_line_crlf", h + few(0, 3, eol="\r\n") + "\r\n", 2),
        ("names_with_spaces_and_signs", h + " a b ,1,2\n-x+,3,4\n", 2),
    ]
    for at in (tile - 1, tile, tile + 1):                    # row 0's newline at this offset of the body
        cases.append((f"newline_at_{at}", h + "n" * (at - 4) + ",1,2\n" + few(1), 2))
    cases += [
        ("crlf_across_tiles", h + "n" * (tile - 5) + ",1,2\r\n" + few(1, eol="\r\n"), 2),     # '\r' at tile - 1, '\n' at tile
        ("row_longer_than_a_tile", h + few(0, 2) + "L" * (tile + 100) + ",1,2\n" + few(2, 2), 2),
        ("row_of_cap_bytes", h + few(0, 2) + "L" * (cap - 4) + ",1,2\n" + few(2, 2), 2),
        ("rows_ending_at_every_offset_of_a_lane", h + "".join("x" * k + ",1,2\n" for k in range(40)), 2),
    ]
    return cases


def refused(tile: int, cap: int):
    """[(name, text, n_currencies, flag or None, (row, code) or None)]: rows count from 0 behind the header"""
    h = header(2)
    bad_row = lambda row, code, text: (text, 2, None, (row, code))
    flag = lambda f, text: (text, 2, f, None)
    cases = {
        "quoted_field": flag(FLAG_BYTE, h + few(0, 2) + 'q,"1",2\n'),
        "quote_in_name": flag(FLAG_BYTE, h + few(0, 2) + 'q"q,1,2\n'),
        "byte_c3": flag(FLAG_BYTE, (h + few(0, 2)).encode() + "zoé,1,2\n".encode()),
        "nul": flag(FLAG_BYTE, h + few(0, 2) + "a\0b,1,2\n"),
        "bare_cr_mid_row": flag(FLAG_BARE_CR, h + few(0, 2) + "a\rb,1,2\n" + few(2, 2)),
        "bare_cr_ends_a_tile": flag(FLAG_BARE_CR, h + "n" * (tile - 1) + "\rn,1,2\n" + few(1)),
        "bare_cr_ends_the_file": flag(FLAG_BARE_CR, h + few(0, 3) + "a,1,2\r"),
        "cr_cr_lf": flag(FLAG_BARE_CR, h + few(0, 3) + "a,1,2\r\r\n"),
        "blank_middle_line": bad_row(3, ROW_EMPTY, h + few(0, 3) + "\n" + few(3, 2)),
        "blank_middle_line_crlf": bad_row(3, ROW_EMPTY, h + few(0, 3, eol="\r\n") + "\r\n" + few(3, 2, eol="\r\n")),
        "two_blank_last_lines": bad_row(3, ROW_EMPTY, h + few(0, 3) + "\n\n"),
        "field_short": bad_row(2, ROW_DELIMITERS, h + few(0, 2) + "s,1\n" + few(2, 2)),
        "field_long": bad_row(2, ROW_DELIMITERS, h + few(0, 2) + "s,1,2,3\n" + few(2, 2)),
        "empty_balance": bad_row(1, ROW_EMPTY_BALANCE, h + few(0, 1) + "e,,2\n" + few(1, 2)),
        "empty_last_balance": bad_row(1, ROW_EMPTY_BALANCE, h + few(0, 1) + "e,1,\n" + few(1, 2)),
        "12a": bad_row(4, ROW_NOT_DECIMAL, h + few(0, 4) + "x,12a,2\n"),
        "minus_1": bad_row(0, ROW_NOT_DECIMAL, h + "x,1,-1\n" + few(0, 4)),
        "space_before_digit": bad_row(2, ROW_NOT_DECIMAL, h + few(0, 2) + "x, 1,2\n"),
        "row_of_cap_plus_1_bytes": bad_row(2, ROW_TOO_LONG, h + few(0, 2) + "L" * (cap - 3) + ",1,2\n" + few(2, 2)),
        "two_bad_rows_lower_wins": bad_row(2, ROW_NOT_DECIMAL, h + few(0, 2) + "x,12a,2\n" + few(2, 2) + "e,,2\n"),
        "two_bad_rows_in_two_tiles": bad_row(1, ROW_EMPTY_BALANCE, h + few(0, 1) + "e,,2\n" + "n" * tile + ",1,2\n" + "x,1,2,3\n"),
    }
    return [(name,) + case for name, case in cases.items()]


# ----------------------------------------------------------------------------- bodies beyond one round of the scan
# Pass 2 is one workgroup that takes SCAN_BLOCK tiles' words a round (MST_CSV_SCAN_BLOCK of csrc/mst_csv.h, restated; the
# check program prints it): a body over SCAN_BLOCK * tile bytes -- 4 MiB -- carries the newlines before a round into the next.
SCAN_BLOCK = 1024
ALPHABET = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789"
_LETTERS = bytes(ord(ALPHABET[b % len(ALPHABET)]) for b in range(256))


def tiles_of(body_len: int, tile: int) -> int:
    return -(-body_len // tile)


def scan_rounds(body_len: int, tile: int) -> int:
    return -(-tiles_of(body_len, tile) // SCAN_BLOCK)


def large_rows(tile: int, body_len: int, open_end: bool = False):
    """The rows (line ends included) of a body of exactly body_len bytes.  Names of 900 to 1100 ALPHABET letters, so that a few
    thousand rows fill it and every round of the scan holds hundreds of newlines; every 37th row is short; one row longer than
    a tile lies across the edge between tile SCAN_BLOCK - 1 and tile SCAN_BLOCK where the body goes on behind it; the last
    row, stretched to end the body exactly, is longer than a tile as well.  Balances are distinct per row."""
    rng = random.Random(20240611)
    edge = SCAN_BLOCK * tile
    rows, pos, crossed = [], 0, body_len < edge + 2 * tile
    fields = lambda i: f",{1000 * i + 1},{1000 * i + 2}\n"
    while body_len - pos > tile + 1200:
        i = len(rows)
        if not crossed and pos + 1200 > edge - 2000:
            name, crossed = "X" * (tile + 100), True                 # starts in tile SCAN_BLOCK - 1, ends in tile SCAN_BLOCK
            assert edge - tile < pos < edge < pos + len(name)
        elif i % 37 == 5:
            name = f"s{i}"
        else:
            name = rng.randbytes(rng.randint(900, 1100)).translate(_LETTERS).decode()
        rows.append(name + fields(i))
        pos += len(rows[-1])
    tail = fields(len(rows))
    if open_end:
        tail = tail[:-1]
    rows.append("Z" * (body_len - pos - len(tail)) + tail)
    assert sum(map(len, rows)) == body_len and tile < len(rows[-1]) < 2 * tile and crossed
    return rows


def _shorter(row: str, by: int) -> str:
    """the row with its name cut by `by` letters"""
    name, rest = row.split(",", 1)
    assert len(name) > by
    return name[:-by] + "," + rest


LARGE_ACCEPTED = ["tiles_1024", "tiles_1025", "tiles_1025_open_end", "tiles_2049"]
# each a copy of tiles_1025 with one edit that only the scan's second round, or a flag kept through it, can report
LARGE_REFUSED = ["quote_in_the_last_tile", "bare_cr_in_tile_1024", "quote_in_tile_3_only", "12a_in_the_last_row", "bad_rows_in_two_rounds"]


@functools.lru_cache(maxsize=None)
def large(name: str, tile: int):
    """(text, n_currencies, flag or None, (row, code) or None) of a LARGE_ACCEPTED or LARGE_REFUSED case: the last two None
    for an accepted one.  tiles_1024 ends with the last byte of tile 1023, a newline; tiles_1025 is that one byte longer, its
    last newline alone in tile 1024; tiles_2049 takes a third round of 281 tiles, with a thousand newlines of its own."""
    h, edge = header(2), SCAN_BLOCK * tile
    if name in LARGE_ACCEPTED:
        body_len = {"tiles_1024": edge, "tiles_1025": edge + 1, "tiles_1025_open_end": edge + 1, "tiles_2049": 2 * edge + 280 * tile + 777}[name]
        return h + "".join(large_rows(tile, body_len, open_end=name.endswith("open_end"))), 2, None, None
    rows = large_rows(tile, edge + 1)
    last = len(rows) - 1
    if name == "quote_in_the_last_tile":
        rows[last] = rows[last][:-1] + '"'                           # tile 1024 is this one byte
        return h + "".join(rows), 2, FLAG_BYTE, None
    if name == "bare_cr_in_tile_1024":
        rows[last] = rows[last][:-1] + "\r"
        return h + "".join(rows), 2, FLAG_BARE_CR, None
    if name == "quote_in_tile_3_only":
        body = "".join(rows)
        at = 3 * tile + 5
        while not (body[at].isalnum() and body[at + 1].isalnum()):    # inside a name
            at += 1
        assert at < 4 * tile
        return h + body[:at] + '"' + body[at + 1:], 2, FLAG_BYTE, None
    if name == "12a_in_the_last_row":                                # 'x,12a,2' ends tile 1023, its newline is tile 1024
        rows[last] = _shorter(rows[last], 8)
        return h + "".join(rows + ["x,12a,2\n"]), 2, None, (last + 1, ROW_NOT_DECIMAL)
    if name == "bad_rows_in_two_rounds":                             # the lower row wins, though the later row's code is lower
        rows[last] = _shorter(rows[last], 8)
        low = len(rows) // 2
        assert len(rows[low]) > 900 and sum(map(len, rows[:low + 1])) < edge - tile
        rows[low] = rows[low][:len(rows[low]) - 7].replace(",", "c") + ",12a,2\n"       # as long as it was
        return h + "".join(rows + ["x,1,2,3\n"]), 2, None, (low, ROW_NOT_DECIMAL)
    raise KeyError(name)


def write_case(directory, name: str, content) -> str:
    """the path of a case's file: the golden itself, or the text written into `directory` byte for byte"""
    if isinstance(content, str) and content.endswith(".csv") and "\n" not in content:
        return os.path.join(GOLDEN, content)
    path = os.path.join(str(directory), name + ".csv")
    with open(path, "wb") as f:
        f.write(content if isinstance(content, bytes) else content.encode())
    return path
