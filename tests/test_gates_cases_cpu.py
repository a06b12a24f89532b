"""The gate compiler without a GPU (csrc/gates_compile.h through tests/cpp/gates_compile_check.cpp, built with the address and
undefined-behaviour sanitizers and run as a program of its own): every graph of tests/gates_cases.py lowers to what
tests/golden/gates_lowering.json recorded before the compiler moved out of gates.hip, the library gives the same words, the
tile rule is the restated one, the program cache behaves, and an interpreter in Python reads the lowered words back: same value
as the graph itself, operand bounds within the compiler's rules, no slot read before it is written."""
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
