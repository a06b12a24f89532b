"""The gate compiler without a GPU (csrc/gates_compile.h through tests/cpp/gates_compile_check.cpp, built with the address and
undefined-behaviour sanitizers and run as a program of its own): every graph of tests/gates_cases.py lowers to what
tests/golden/gates_lowering.json recorded before the compiler moved out of gates.hip, the library gives the same words, the
tile rule is the restated one, the program cache behaves, and an interpreter in Python reads the lowered words back: same value
as the graph itself, operand bounds within the compiler's rules, no slot read before it is written.  For the device corpus of
the GPU tests: the C oracle's rows are those of halo2's definition in Python integers on every program and word pattern, the
lowered programs reach the compiler's bounds, and the device's arithmetic replayed in integers stays within them."""
import json
import os
import subprocess

import numpy as np
import pytest

import gates_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "circuits_halo2_amd", "csrc")


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gates") / "gates_compile_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1", "-pthread",
                           "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "gates_compile_check.cpp"), "-o", exe])

    def ask(lines):
        r = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout.split("\n")[:-1]
    return ask


@pytest.fixture(scope="module")
def lowered(check, O):
    """name -> the check program's answer for every corpus graph: a list of words, or the message"""
    cases = gc.corpus(O)
    out = {}
    for c, line in zip(cases, check([c.line() for c in cases])):
        kind, _, rest = line.partition(" ")
        out[c.name] = [int(x) for x in rest.split()] if kind == "words" else rest
        assert kind in ("words", "error")
    return out


def test_corpus_is_what_the_issue_names(O):
    names = [c.name for c in gc.corpus(O)]
    assert sum(n.startswith("random_") for n in names) >= 40
    assert {n_calc for _, n_calc, _, _ in gc.RANDOM_SEEDS} == {1, 8, 40, 120, 300}
    for n_calc in (1, 8, 40, 120, 300):
        shapes = {(ni, nch) for _, n, ni, nch in gc.RANDOM_SEEDS if n == n_calc}
        assert {(1, 2), (0, 0)} <= shapes and any(ni == 0 for ni, _ in shapes) and any(nch == 0 for _, nch in shapes)


def test_every_graph_lowers_as_recorded(lowered):
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "gates_lowering.json")))
    assert list(want) == list(lowered)
    for name, w in want.items():
        got = lowered[name]
        assert ({"error": got} if isinstance(got, str) else {"sha256": gc.digest(got)}) == w, name
    messages = {w["error"] for w in want.values() if "error" in w}
    assert messages == {"empty program", "null array in graph", "more than 65536 calculations", "intermediate used before it is defined",
                        "horner parts out of range", "dependency chain deeper than 4096 calculations", "constant index out of range",
                        "column query out of range", "challenge index out of range", "unknown value source", "unknown calculation",
                        "program too large (slot or constant index above 65535)"}
    assert all("sha256" in want[n] for n in ("unreached_constant_index", "unreached_calculation_and_column", "depth_4096", "live_values_70"))
    assert lowered["live_values_70"][0] == 71 and lowered["lifo_chain_40"][0] == 2    # (values consumed in reverse order do not wait)


def test_the_library_gives_the_same_words(lowered, O):
    from circuits_halo2_amd import arithmetic as A
    from circuits_halo2_amd.ffi import SummaGpuError
    for c in gc.corpus(O):
        if isinstance(lowered[c.name], str):
            with pytest.raises(SummaGpuError, match="sg_gates_program_words: " + lowered[c.name].replace("(", r"\(").replace(")", r"\)")):
                A.gates_program_words(c.graph, *c.dims)
        else:
            assert A.gates_program_words(c.graph, *c.dims) == lowered[c.name], c.name
            assert A.gates_program_info(c.graph, *c.dims) == (lowered[c.name][3], lowered[c.name][0])


def test_a_fault_before_an_intermediate_is_an_error_not_a_crash(check):
    """ADD(constant out of range, an intermediate): the emission goes on with placeholders after the first fault"""
    A = gc.A
    g = gc.RawGraph(1, [0], [(A.NEGATE, (A.ADVICE, 0, 0), gc.NO_B, 0, 0), (A.ADD, (A.CONSTANT, 5, 0), (A.INTERMEDIATE, 0, 0), 0, 0)])
    assert check([gc.Case("fault_then_intermediate", g, 0, 1, 0, 0).line()]) == ["error constant index out of range"]


def test_lowering_knobs_and_listing(check, O):
    case = next(c for c in gc.corpus(O) if c.name == "mst_gates_nc2")
    plain, again, far, convert = check([case.line(), case.line(reload_distance=12), case.line(reload_distance=48), case.line(convert_above=1)])
    assert plain == again and far != plain and convert != plain
    words = [int(x) for x in plain.split()[1:]]
    listing = check([case.line("dump")])
    assert listing[-1] == "end" and len(listing) == words[3] + 1
    live = [int(l.split("live ")[1].split()[0]) for l in listing[:-1]]
    assert max(live) == words[0] and listing[0].split()[:2] == ["0", "loadcol"]
    assert listing[-2].endswith("(last use of dst: 4294967295)")


def test_tile_rule(check):
    grid = [(s, c) for s in range(1, 65) for c in (5, 40, 200)]
    got = check([f"tile {s} {c}" for s, c in grid])
    for (s, c), line in zip(grid, got):
        rows, lds, fits, waves = gc.interpreter_tile(s, c)
        assert line == f"tile slots={s} consts={c} rows={rows} lds={lds} fits={int(fits)} waves={waves}"
    for rows, slots in gc.TILE_ROWS_AT_5_CONSTANTS.items():
        for s in slots:
            r, _, fits, _ = gc.interpreter_tile(s, 5)
            assert (r if fits else None) == rows, s
    assert sorted(s for v in gc.TILE_ROWS_AT_5_CONSTANTS.values() for s in v) == list(range(1, 65))
    # more live values than GATES_MAX_SLOTS fit nothing, whatever the constants
    assert not any(gc.interpreter_tile(65, c)[2] for c in (0, 5)) and gc.interpreter_tile(64, 0)[2] and not gc.interpreter_tile(64, 1)[2]


def test_a_program_for_every_tile_size(lowered):
    """what the GPU test of the three tile sizes relies on: 8, 20 and 40 live values, four constants"""
    for rows, n in gc.INTERPRETER_TILE_PROGRAMS.items():
        assert lowered[f"live_values_{n}"][0] == n + 1 and gc.interpreter_tile(n + 1, 4)[::2] == (rows, True)
    assert [n + 1 for n in gc.INTERPRETER_TILE_PROGRAMS.values()] == [8, 20, 40]


def test_program_cache(check):
    assert check(["cache", "cache"]) == ["cache ok", "cache ok"]      # (twice: the check leaves nothing behind)


def test_lowered_words_read_back(lowered, O):
    """every accepted program on three random rows: the value of the graph (oracle/pyref.py), bounds and slots within the rules"""
    from oracle import pyref
    A = gc.A
    top = 0
    for ci, c in enumerate(gc.corpus(O)):
        words = lowered[c.name]
        if isinstance(words, str):
            continue
        g = c.graph
        for row in range(3):
            *consts, previous = pyref.random_fr(7000 + 10 * ci + row, g.n_constants + c.n_challenges + 5)
            seed = 1 + 3 * ci + row
            cell = lambda col, rot: (seed * 0x9E3779B97F4A7C15 + col * 0x1000003 + (rot + 64) * 0x10001) ** 3 % gc.R   # any fixed function of (column, rotation)
            base = {A.FIXED: 0, A.ADVICE: c.n_fixed, A.INSTANCE: c.n_fixed + c.n_advice}
            nc = g.n_constants
            want = pyref.eval_graph(g.as_dict(consts[:nc]), lambda kind, index, rot: cell(base[kind] + index, rot), consts[nc:nc + c.n_challenges],
                                    *consts[nc + c.n_challenges:], previous)
            got, bound = gc.run_program(words, consts, cell, previous)
            assert got == want, (c.name, row)
            top = max(top, bound)
    assert top <= 120   # additions and doublings stop at 80, a fused addend at 80 + 2, a subtraction's result at 120


# ----------------------------------------------------------------------------- the device corpus (tests/test_gpu_gates_edges.py runs it)
K, EXT_K, COSETS = 2, 3, 2     # 8 rows either way: one block of 2^3 with rotations two rows apart, two blocks of 2^2


@pytest.fixture(scope="module")
def device_lowered(check, O):
    """name -> words of every device-corpus graph, by the check program; the library agrees"""
    from circuits_halo2_amd import arithmetic as A
    cases = gc.device_corpus(O)
    out = {}
    for c, line in zip(cases, check([c.line() for c in cases])):
        kind, _, rest = line.partition(" ")
        assert kind == "words", (c.name, line[:80])
        out[c.name] = [int(x) for x in rest.split()]
        assert A.gates_program_words(c.graph, *c.dims) == out[c.name], c.name
    return out


def _model_rows(words, case, inp, k, ext_k, cosets, **kw):
    n, _, step = gc._blocks(k, ext_k, cosets)
    cols = [gc._ints(x) for grp in ("fixed", "advice", "instance") for x in inp[grp]]
    table = gc._ints(inp["constants"]) + gc._ints(inp["challenges"]) + [gc._ints(inp[x])[0] for x in ("beta", "gamma", "theta", "y")]
    prev = gc._ints(inp["previous"])
    out = []
    for i in range(len(prev)):
        base, at = i - i % n, i % n
        out.append(gc.run_device_model(words, table, lambda col, rot: cols[col][base + (at + rot * step) % n], prev[i], **kw))
    return gc._words(out)


def test_device_corpus_is_what_the_issue_names(O, device_lowered):
    cases = gc.device_corpus(O)
    names = [c.name for c in cases]
    assert not any(n.startswith("error_") for n in names)
    assert {c.name for c in gc.corpus(O) if not c.name.startswith("error_")} <= set(names)
    assert sum(n.startswith("random_seed") for n in names) == 40
    assert {"result_constant", "result_column", "result_previous_value", "horner_without_parts", "depth_4096", "unreached_constant_index",
            "unreached_calculation_and_column", "many_constants", "large_program", "live_values_62", "live_values_63",
            *gc.BOUND_FILLERS, *[f"rotations_k{k}" for k in gc.ROTATION_KS]} <= set(names)
    assert len(names) - len(gc.REFUSED) > 64                                   # the cache turns over within one pass
    assert len(device_lowered["large_program"]) - 4 > 4 * 16384                # 16 bytes an instruction: above 256 KiB
    for k in gc.ROTATION_KS:
        n = 1 << k
        assert {0, 1, -1, n - 1, 1 - n, n, -n, n + 1, -n - 1, -5, 17} == set(gc.device_case(O, f"rotations_k{k}").graph.rotations)
    # a random_graph's last calculation reaches a handful of the others; the folded ones lower every calculation
    assert max(device_lowered[n][3] for n in names if n.startswith("random_seed")) < 40
    assert all(device_lowered[f"random_folded_seed{s}_calc{n}"][3] > 2 * n for s, n, _ in gc.FOLDED_SEEDS)


@pytest.mark.parametrize("pattern", gc.PATTERNS)
def test_oracle_against_definition(O, device_lowered, pattern):
    """every device-corpus program on every pattern, both layouts: the C oracle's rows (what the GPU tests expect) are the rows of
    halo2's definition in Python integers, and the rows of the device's arithmetic replayed in integers over the lowered words,
    with every value within its tracked bound and no subtraction below zero"""
    for ci, c in enumerate(gc.device_corpus(O)):
        for cosets in (0, COSETS):
            inp = gc.make_inputs(O, c, pattern, (cosets << K) if cosets else (1 << EXT_K), seed=ci)
            want = gc.expected_rows(O, c, inp, K, EXT_K, cosets)
            assert (gc.definition_rows(c, inp, K, EXT_K, cosets) == want).all(), (c.name, cosets)
            assert (_model_rows(device_lowered[c.name], c, inp, K, EXT_K, cosets) == want).all(), (c.name, cosets)
            assert max(gc._ints(want)) < gc.R


def test_patterns_are_what_the_issue_names(O):
    c = gc.device_case(O, "random_folded_seed505_calc120")      # 2 fixed, 5 advice, 1 instance, 3 challenges
    flat = lambda inp: [gc._ints(a) for a in (*inp["fixed"], *inp["advice"], *inp["instance"], inp["previous"], inp["constants"], inp["challenges"],
                                               np.concatenate([inp[n] for n in ("beta", "gamma", "theta", "y")]))]
    for pattern, word in (("top", gc.R - 1), ("zero", 0), ("one", (1 << 256) % gc.R)):
        assert all(set(a) == {word} for a in flat(gc.make_inputs(O, c, pattern, 8)))
    fwd, rev = flat(gc.make_inputs(O, c, "columns_alternate", 8)), flat(gc.make_inputs(O, c, "columns_alternate_reversed", 8))
    assert [set(a) for a in fwd] == [{gc.R - 1} if j % 2 == 0 else {0} for j in range(len(fwd))]
    assert [set(a) for a in rev] == [{0} if j % 2 == 0 else {gc.R - 1} for j in range(len(rev))]
    for a in flat(gc.make_inputs(O, c, "rows_cycle", 8)):
        assert [a[i] for i in range(len(a)) if i % 6 != 5] == [[0, 1, gc.R - 1, gc.R - 2, 1 << 253][i % 6] for i in range(len(a)) if i % 6 != 5]
    for pattern in gc.PATTERNS:                                 # canonical words only
        assert all(w < gc.R for a in flat(gc.make_inputs(O, c, pattern, 8)) for w in a)


def test_reach(O, check, device_lowered):
    """what run_program's bounds show over the lowered device corpus: the numbers are the compiler's own rules (a product up to
    Ba Bb = 170, additions and doublings up to 80, a fused addend up to 80 - 2, a subtraction's result up to 120, loads at 32)"""
    codes, sub_k, neg_k, kinds = set(), set(), set(), set()
    mul = sqr = add = sub = dbl = 0
    muladd = set()
    for c in gc.device_corpus(O):
        trace = []
        gc.run_program(device_lowered[c.name], [1] * (c.graph.n_constants + c.n_challenges + 4), lambda col, rot: 1, 1, trace=trace)
        kinds.add(gc.decode(device_lowered[c.name])[1])
        for code, kidx, bx, by, bz, out in trace:
            codes.add(code)
            sub_k |= {kidx} if code == gc.G_SUB else set()
            neg_k |= {kidx} if code == gc.G_NEG else set()
            mul = max(mul, bx * by if code == gc.G_MUL else 0)
            sqr = max(sqr, bx if code == gc.G_SQR else 0)
            add = max(add, out if code == gc.G_ADD else 0)
            dbl = max(dbl, out if code == gc.G_DBL else 0)
            sub = max(sub, out if code == gc.G_SUB else 0)
            if code == gc.G_MULADD:
                muladd.add((bx * by, bz))
    assert codes == set(range(10))                                   # G_RED, G_MULADD, G_LOADPREV and G_DBL among them
    assert sub_k == neg_k == set(range(6))
    assert mul == 160 and sqr == 12 and add == 80 and dbl == 80 and sub == 120
    assert (160, 78) in muladd and max(z for _, z in muladd) == 78   # (an addend above 78 is reduced first: 2 + 78 = 80)
    assert kinds == {gc.SLOT, gc.CONST}
    # SG_GATES_CONVERT's lowering: loads with kidx 1, and the same rows from them
    for name in ("mst_gates_nc2", "random_folded_seed504_calc120"):
        c = gc.device_case(O, name)
        words = [int(x) for x in check([c.line(convert_above=1)])[0].split()[1:]]
        loads = [o["kidx"] for o in gc.decode(words)[3] if o["code"] == gc.LOADCOL]
        assert 1 in loads and 0 in loads and words != device_lowered[name]
        inp = gc.make_inputs(O, c, "top", 1 << EXT_K)
        assert (_model_rows(words, c, inp, K, EXT_K, 0) == gc.expected_rows(O, c, inp, K, EXT_K)).all()


def test_tile_rule_at_the_lds_budget(check, device_lowered):
    slots = lambda name: device_lowered[name][0]
    assert (slots("live_values_62"), slots("live_values_63"), slots("many_constants"), slots("live_values_39")) == (63, 64, 40, 40)
    assert gc.interpreter_tile(63, 4) == (64, 145296, True, 1) and gc.LDS_BUDGET == 147456
    assert gc.interpreter_tile(64, 4)[2] is False
    rows, lds, fits, _ = gc.interpreter_tile(40, gc.MANY_CONSTANTS + 4)
    assert (rows, fits) == (64, True) and gc.LDS_BUDGET - 64 * gc.LIMB_BYTES < lds <= gc.LDS_BUDGET      # within one slot of 64 rows
    assert check(["tile 63 4", "tile 64 4", f"tile 40 {gc.MANY_CONSTANTS + 4}"]) == [
        "tile slots=63 consts=4 rows=64 lds=145296 fits=1 waves=1", f"tile slots=64 consts=4 rows=256 lds={(4 + 64 * 256) * 36} fits=0 waves=0",
        f"tile slots=40 consts={gc.MANY_CONSTANTS + 4} rows=64 lds={lds} fits=1 waves=1"]
    # a forced tile of 256 rows on 40 live values does not fit either (SG_GATES_ROWS)
    assert 4 * gc.LIMB_BYTES + 40 * 256 * gc.LIMB_BYTES > gc.LDS_BUDGET


def test_the_cases_tell_a_broken_evaluator_apart(O, device_lowered):
    """three wrong evaluators, each noticed by a named case (tests/gates_cases.py: run_device_model, definition_rows)"""
    rows = 1 << EXT_K

    def wrong_rows(name, pattern, **kw):
        c = gc.device_case(O, name)
        inp = gc.make_inputs(O, c, pattern, rows, seed=5)
        got, want = _model_rows(device_lowered[name], c, inp, K, EXT_K, 0, check=False, **kw), gc.expected_rows(O, c, inp, K, EXT_K)
        return int((got.reshape(-1, 32) != want.reshape(-1, 32)).any(axis=1).sum())
    # a subtraction with kidx - 1, half the K: the largest words fill the subtrahend, uniform ones do so on some rows only
    for name in ("fill_sub_neg_kidx4", "fill_sub_neg_kidx5", "fill_sub_neg_small_minuend_kidx5"):
        assert wrong_rows(name, "top", kidx_delta=-1) == rows and 0 < wrong_rows(name, "random", kidx_delta=-1) < rows
    # a reduction skipped before a product, Ba Bb = 196 in place of 98: the value that stayed unreduced is read again with the K
    # of a reduced one.  (A product at 171 .. 340 alone stays below 3 p and is the right residue: of the 36 reductions whose
    # omission gives such a product, in the programs of up to 2000 calculations, this is the one any words notice -- the largest
    # words and uniform ones alike, all-zero words not; run_program's own product rule refuses all 36.)
    products = []
    c = gc.device_case(O, "random_folded_seed505_calc120")
    inp = gc.make_inputs(O, c, "top", rows, seed=5)
    _model_rows(device_lowered[c.name], c, inp, K, EXT_K, 0, check=False, skip_reduction=11, products=products)
    assert max(products) == 196 and wrong_rows(c.name, "top", skip_reduction=11) == rows
    assert wrong_rows(c.name, "random", skip_reduction=11) == rows and wrong_rows(c.name, "zero", skip_reduction=11) == 0
    with pytest.raises(gc.DeviceModelFault):
        _model_rows(device_lowered[c.name], c, inp, K, EXT_K, 0, skip_reduction=11)
    # a rotation that wraps at 2^k inside the extended domain: only words that differ from row to row can tell
    c = gc.device_case(O, f"rotations_k{K}")
    for pattern, noticed in (("rows_cycle", True), ("random", True), ("top", False), ("zero", False)):
        inp = gc.make_inputs(O, c, pattern, rows, seed=5)
        flipped = gc.definition_rows(c, inp, K, EXT_K, rotation_wraps_at_k=True)
        assert (flipped != gc.expected_rows(O, c, inp, K, EXT_K)).any() == noticed, pattern
