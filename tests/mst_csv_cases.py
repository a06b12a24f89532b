"""The two fixed lists of CSV files the device CSV reader is checked with, on the host (test_mst_csv_cpu.py: the four passes of
csrc/mst_csv.h run serially) and on the device (test_gpu_mst_csv.py).  ACCEPTED: files inside the reader's subset -- it must take
every one and find the fields `parse_csv_to_entries` finds.  REFUSED: files outside it, each with what the reader must
report: a flag of the scan, or the lowest offending row and its code.  `tile` and `cap` are the reader's geometry
(MST_CSV_TILE, MST_CSV_ROW_CAP): newlines and carriage returns are placed at the tile edges by the length of a name."""
import os

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


def write_case(directory, name: str, content) -> str:
    """the path of a case's file: the golden itself, or the text written into `directory` byte for byte"""
    if isinstance(content, str) and content.endswith(".csv") and "\n" not in content:
        return os.path.join(GOLDEN, content)
    path = os.path.join(str(directory), name + ".csv")
    with open(path, "wb") as f:
        f.write(content if isinstance(content, bytes) else content.encode())
    return path
