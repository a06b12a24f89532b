"""The rounds a tree in HBM settles in full -- new users admitted into its padding, the name index extended, gone users zeroed
(csrc/mst_admit.h) -- as pairs of snapshot CSVs, on the host (test_mst_admit_cpu.py: the header's serial steps behind the reader's,
the sort's and the diff's) and on the device (test_gpu_mst_admit.py), and the model both are compared with, in pure Python.

A case is (name, rows of A, rows of B, n_currencies, refusal): rows as in mst_diff_cases, A the file the tree was built from in
FILE order, B the next round's file, refusal None or what the settle refuses it for: "no_room" (n_tree + n_new > 2^depth),
"name_too_long" (a NEW name of more than 64 bytes), "cap_new" / "cap_gone" (a diff whose cap, CAP_SHORT, left the list incomplete).

The edges: 64, a wave's tile; 256, a workgroup; 16384, a group of the scan; 2048, the sort's tile.  Trees of 1, 2, 3, 63, 65, 257
and 2049 rows admit 0, 1, 2, 64, 65, 257 and exactly 2^depth - n_tree rows, each where the tree has room; one tree of 32769 rows
(depth 16) admits 16386, the first size with list positions 16383, 16384 and 16385."""
import random

import mst_diff_cases as D
from mst_diff_cases import base, model, text_of, write_case  # noqa: F401

R = D.R
TREES = (1, 2, 3, 63, 65, 257, 2049)
NEW_COUNTS = (0, 1, 2, 64, 65, 257)
BIG_TREE, BIG_NEW = 32769, 16386
CAP_SHORT = 1
OPEN_END = "open_end_5"


def text_a(name: str, a, nc: int) -> str:
    """the text of a case's file A: text_of, without the final newline for OPEN_END"""
    text = text_of(a, nc)
    return text[:-1] if name == OPEN_END else text


def free_of(n: int) -> int:
    return (1 << max(0, (n - 1).bit_length())) - n


def fresh_name(k: int) -> bytes:
    """before all old names ('#' is below '0'), between them (an extension of what may be an old name), after all"""
    return (b"#%05d" % k, b"%06dx" % k, b"zz%05d" % k)[k % 3]


def next_round(a, n_new: int, nc: int, tag: str):
    """B of A: every third row's balance bumped, the rows of the edge leaves gone (where more than two rows are left), n_new fresh
    rows spread over the file with the first before row 0, and behind it all one old name once more (a shadowed row)"""
    n = len(a)
    gone = set(D.edge_leaves(n)) if n > 3 else ({n - 1} if n > 1 else set())
    rows = [D.bump(row, i % nc) if i % 3 == 0 else row for i, row in enumerate(a) if i not in gone]
    fresh = [(fresh_name(k), [str(7 * k + c) for c in range(nc)]) for k in range(n_new)]
    random.Random(f"mst_admit_cases.{tag}.{n}.{n_new}").shuffle(fresh)
    step = max(1, len(rows) // max(1, n_new))
    for k, row in enumerate(fresh):
        rows.insert(min(len(rows), k * (step + 1)), row)
    if rows:
        keep = next((row for row in rows if row[0][:1].isdigit() and not row[0].endswith(b"x")), None)
        if keep is not None:
            rows.append(D.bump(keep, 0))
    return rows or [(b"lonely", ["1"] * nc)]


def cases():
    out = []
    add = lambda name, a, b, nc=2, refusal=None: out.append((name, a, b, nc, refusal))
    for n in TREES:
        a = base(n)
        for k in sorted({c for c in NEW_COUNTS if c <= free_of(n)} | {free_of(n)}):
            add(f"tree_{n}_new_{k}", a, next_round(a, k, 2, "grid"))
    a = base(BIG_TREE)
    add(f"tree_{BIG_TREE}_new_{BIG_NEW}", a, next_round(a, BIG_NEW, 2, "big"))
    # contents: a proper prefix and an extension of an old name, the empty name, 64 bytes, field-equal texts, the same NEW name
    # twice more than 256 rows apart, NEW rows between changed and shadowed ones
    a = base(300)
    old = a[5][0]
    b = [D.bump(row, 1) if i % 2 else row for i, row in enumerate(a) if i not in (0, 299, 64)]
    twice = (b"twice", ["11", "12"])
    special = [(old[:5], ["007", str(R + 5)]), (old + b"0", ["1", "2"]), (b"", ["3", "4"]), (b"n" * 64, ["5", "6"]), twice,
               (b"!first", ["0", "0"]), (b"~last", [str(R - 1), "9"])]
    for k, row in enumerate(special):
        b.insert(k * 3, row)
    b.insert(len(b) - 2, (twice[0], ["21", "22"]))            # ... the later one is a shadowed leaf
    b.append(D.bump(a[7], 0))                                  # a shadowed row of an old name
    add("contents_300", a, b)
    a = base(5) + [(b"", ["11", "12"])]
    add("empty_name_in_tree", a, [(b"", ["11", "13"]), a[1], (b"new", ["1", "2"])])
    for nc in (1, 3):
        a = base(65, nc)
        add(f"currencies_{nc}_65", a, next_round(a, 10, nc, f"nc{nc}"), nc)
    # a padding leaf that update_leaves_at gave balances is overwritten: the GPU test does that to this one
    a = base(5)
    add("padding_with_balances_5", a, next_round(a, 3, 2, "padding"))
    # file A without a final newline, which the reader takes: the admitted names follow the last row's last digit in the tree's text,
    # the first of them digits itself, and the round leaves that last leaf as it was
    a = base(5)
    add(OPEN_END, a, [(b"55", ["9", "9"]), D.bump(a[0], 0)] + list(a[1:]) + [(b"new", ["1", "2"])])
    # refusals
    a = base(63)
    add("refused_one_row_too_many_63", a, next_round(a, 2, 2, "many"), refusal="no_room")
    a = base(64)
    add("refused_no_padding_64", a, next_round(a, 1, 2, "full"), refusal="no_room")
    a = base(65)
    add("refused_name_of_65_bytes", a, list(a[:40]) + [(b"n" * 65, ["1", "2"])] + list(a[40:]) + [(b"m" * 66, ["1", "2"])], refusal="name_too_long")
    add("refused_cap_below_new_65", a, next_round(a, 3, 2, "capnew"), refusal="cap_new")
    add("refused_cap_below_gone_65", a, next_round(a, 1, 2, "capgone"), refusal="cap_gone")
    names = [c[0] for c in out]
    assert len(set(names)) == len(names)
    return out


def settled(a, b, nc: int, admit: bool = True, zero: bool = True):
    """The tree of A after the round B: {"diff": the model of mst_diff_cases, "refusal": None | "no_room" | ("name_too_long", row),
    "n": the named leaves, "entries": [(name bytes | None, [integers mod r])] of all 2^depth leaves, "order": the leaf at every
    sorted position, "names": the name at every sorted position, "leaves": the union of the changed, zeroed and admitted leaves,
    "balances": their integers in that order}"""
    m = model(a, b, nc, False)
    n_tree, size = len(a), 1 << m["depth"]
    new = m["new"] if admit else []
    out = {"diff": m, "refusal": None}
    if n_tree + len(new) > size:
        out["refusal"] = "no_room"
        return out
    long_rows = [r for r, (name, _) in enumerate(b) if len(name) > 64]
    if new and long_rows:
        out["refusal"] = ("name_too_long", long_rows[0])
        return out
    value = lambda bal: [int(x) % R for x in bal]
    entries = [(name, value(bal)) for name, bal in a]
    for leaf, bal in zip(m["changed"], m["balances"]):
        entries[leaf] = (entries[leaf][0], bal)
    gone = m["gone"] if zero else []
    for leaf in gone:
        entries[leaf] = (entries[leaf][0], [0] * nc)
    entries += [(b[r][0], value(b[r][1])) for r in new]
    n = len(entries)
    order = sorted(range(n), key=lambda i: entries[i][0])    # stable: equal names in leaf order
    leaves = sorted(m["changed"] + gone) + list(range(n_tree, n))
    out.update(n=n, order=order, names=[entries[i][0] for i in order], leaves=leaves, balances=[entries[i][1] for i in leaves],
               entries=entries + [(None, [0] * nc)] * (size - n))
    return out


def csv_of(entries, nc: int) -> str:
    """`to_csv` of the settled entries: the named leaves in leaf order, canonical integers"""
    return text_of([(name, [str(v) for v in bal]) for name, bal in entries if name is not None], nc)


def duplicates_of(entries):
    """(repeated names, [(shadowed leaf, the leaf a lookup finds)] by name and within a name by leaf)"""
    named = sorted((name, i) for i, (name, _) in enumerate(entries) if name is not None)
    pairs, repeated, head = [], 0, None
    for at in range(1, len(named)):
        if named[at][0] == named[at - 1][0]:
            if head is None or named[head][0] != named[at][0]:
                head, repeated = at - 1, repeated + 1
            pairs.append((named[at][1], named[head][1]))
    return repeated, pairs
