"""CPU checks behind the general lookup permutation (sg_lookup_permute_dev): the rule tests/lookup_permute_cases.py states is a
valid permuted pair on every generator and is the host twin's where the twin sorts by integer; the header, the ctypes list and
the Rust shim name both entry points; the work-space size the launch function and the C ABI take from csrc/poly_plan.h is the
formula restated here."""
import os
import subprocess

import numpy as np
import pytest

import lookup_permute_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "circuits_halo2_amd", "csrc")

VALID = [("wide", 1, 3, 1), ("wide", 2, 2, 2), ("wide", 7, 3, 3), ("wide", 7, 7, 4), ("wide", 257, 3, 5), ("wide", 257, 257, 6), ("wide", 4090, 17, 7),
         ("wide", 4090, 4090, 8), ("equal", 7), ("equal", 4090), ("bijection", 7, 9), ("bijection", 4090, 10), ("range", 7, 11),
         ("range", 4090, 12), ("word32", 7, 13), ("word32", 4090, 14)] + [("one_word", rows, w, 20 + w) for rows in (7, 4090) for w in range(8)]
INVALID = [("missing", rows, v, 40 + i) for rows in (7, 4090) for i, v in enumerate(lc.MISSING)]


@pytest.mark.parametrize("spec", VALID, ids=lc.describe)
def test_the_rule_gives_a_valid_permuted_pair(spec):
    inp, table, want = lc.case(*spec)
    assert want is not None
    a, s = lc.to_ints(want[0]), lc.to_ints(want[1])
    assert a == sorted(lc.to_ints(inp))                                            # A' is the input sorted
    assert all(a[i] == s[i] or (i and a[i] == a[i - 1]) for i in range(len(a)))    # the row property
    assert sorted(s) == sorted(lc.to_ints(table))                                  # S' is a permutation of the table
    assert max(a + s) < lc.R
    # the leftovers ascend down the repeated rows
    rep = [s[i] for i in range(len(a)) if i and a[i] == a[i - 1]]
    assert rep == sorted(rep)


@pytest.mark.parametrize("spec", [s for s in VALID if s[0] in ("range", "word32")], ids=lc.describe)
def test_the_rule_is_the_host_twin_on_one_limb_tables(spec):
    from circuits_halo2_amd.prover import permute_expression_pair
    inp, table, want = lc.case(*spec)
    twin_a, twin_s = permute_expression_pair(np.array(inp), np.array(table))
    assert (twin_a == want[0]).all() and (twin_s == want[1]).all()


@pytest.mark.parametrize("spec", VALID + INVALID, ids=lc.describe)
def test_none_exactly_where_the_twin_raises(spec):
    from circuits_halo2_amd.prover import permute_expression_pair
    inp, table, want = lc.case(*spec)
    try:
        permute_expression_pair(np.array(inp), np.array(table))
        raised = False
    except ValueError:
        raised = True
    assert raised == (want is None) == (spec[0] == "missing")


def test_generators_are_what_they_claim():
    for w in range(8):
        inp, table, _ = lc.case("one_word", 4090, w, 20 + w)
        words = np.concatenate([inp, table]).view(np.uint32).reshape(-1, 8)
        varying = [j for j in range(8) if len(set(words[:, j].tolist())) > 1]
        assert varying == [w], (w, varying)
        assert all(len(set((words[:, w] >> (8 * b) & 255).tolist())) > 1 for b in range(4 if w < 7 else 3))   # every digit of the word varies
    inp, table, _ = lc.case("wide", 4090, 4090, 8)
    assert {0, 1, lc.R - 1, lc.R - 2} <= set(lc.to_ints(table)) and len(set(lc.to_ints(table))) > 4000
    inp, table, _ = lc.case("word32", 4090, 14)
    assert not table[:, 1:].any() and int(table[:, 0].min()) == 1 << 16 and int(table[:, 0].max()) == (1 << 32) - 1
    inp, table, _ = lc.case("range", 4090, 12)
    assert not table[:, 1:].any() and set(table[:, 0].tolist()) == set(range(256))
    inp, table, want = lc.case("bijection", 4090, 10)
    assert (want[0] == want[1]).all() and len(set(lc.to_ints(table))) == 4090
    for rows in (7, 4090):
        ints = {v: lc.to_ints(lc.case("missing", rows, v, 40 + i)[0])[rows // 3] for i, v in enumerate(lc.MISSING)}
        tabs = {v: sorted(lc.to_ints(lc.case("missing", rows, v, 40 + i)[1])) for i, v in enumerate(lc.MISSING)}
        assert tabs["between"][0] < ints["between"] < tabs["between"][-1] and ints["above"] > tabs["above"][-1] and ints["below"] < tabs["below"][0]
        assert ints["top_word"] ^ (1 << 224) in tabs["top_word"] and ints["low_word"] ^ 1 in tabs["low_word"]


def test_header_exports_and_shim_name_both_entry_points():
    from circuits_halo2_amd import ffi
    from test_rust_shim_abi import c_functions, rust_functions
    decl = c_functions()
    assert decl["sg_lookup_permute_dev"] == decl["sg_lookup_permute_small_dev"] == ("int", ["ptr", "ptr", "size", "ptr", "ptr", "ptr"])
    assert decl["sg_lookup_permute_async_dev"] == decl["sg_lookup_permute_small_async_dev"] == ("int", ["ptr", "ptr", "size", "ptr", "ptr", "ptr", "ptr"])
    assert {"sg_lookup_permute_dev", "sg_lookup_permute_async_dev"} <= set(ffi.EXPORTS)
    rust = rust_functions(open(os.path.join(ROOT, "integration", "halo2_gpu_shim", "src", "lib.rs")).read())
    for fn in ("sg_lookup_permute_dev", "sg_lookup_permute_async_dev"):
        assert rust[fn] == decl[fn]
    header = open(os.path.join(ROOT, "include", "summa_gpu.h")).read()
    assert "#define SG_ABI_VERSION 4" in header
    from circuits_halo2_amd import arithmetic
    assert callable(arithmetic.lookup_permute)


# ---- the work space: csrc/poly_plan.h restated
TILE, BINS, HEAD = 1024, 256, 64


def work_words(rows):
    """head | 4 key arrays of 8 words a row | hist[2][256][tiles] | used, repeat, rank, left: a word a row | sums[2][tiles up to 4]"""
    tiles = -(-rows // TILE)
    return HEAD + 4 * 8 * rows + 2 * BINS * tiles + 4 * rows + 2 * (-(-tiles // 4) * 4)


def test_work_space_size(tmp_path):
    exe = str(tmp_path / "lookup_sort_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "lookup_sort_plan_check.cpp"),
                           "-o", exe])
    sizes = [1, 255, 256, 257, 1023, 1024, 1025, 4090, 8186, lc.USABLE_17, (1 << 31) - 1]
    got = subprocess.run([exe] + [str(n) for n in sizes], capture_output=True, text=True, check=True).stdout.split("\n")[:-1]
    assert got[0] == f"digit_bits=8 bins={BINS} passes=32 threads=256 items=4 tile={TILE} head={HEAD} flag=32 launches=103 max_rows={(1 << 31) - 1}"
    last = 0
    for rows, line in zip(sizes, got[1:]):
        f = dict(kv.split("=") for kv in line.split())
        f = {k: int(v) for k, v in f.items()}
        tiles = -(-rows // TILE)
        assert f["rows"] == rows and f["tiles"] == tiles
        assert f["words"] == work_words(rows) and f["bytes"] == 4 * work_words(rows)
        assert (f["keys"], f["hist"], f["used"]) == (HEAD, HEAD + 32 * rows, HEAD + 32 * rows + 2 * BINS * tiles)
        assert (f["repeat"], f["rank"], f["left"], f["sums"]) == tuple(f["used"] + j * rows for j in (1, 2, 3, 4))
        assert f["stride"] == -(-tiles // 4) * 4 and f["words"] == f["sums"] + 2 * f["stride"]
        assert all(f[k] % 4 == 0 for k in ("keys", "hist", "used", "sums"))          # what is read 16 bytes at a time starts on 16
        assert f["bytes"] > last                                                     # monotone
        last = f["bytes"]
    assert all(work_words(n + 1) >= work_words(n) for n in list(range(1, 3000)) + [lc.USABLE_17 - 1, lc.USABLE_17])
