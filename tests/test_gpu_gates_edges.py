"""The gate evaluator (csrc/gates.hip, csrc/gates_device.cuh and the plumbing of csrc/abi_quotient.hip behind sg_quotient_gates_dev and
sg_quotient_gates_cosets_dev) on the device corpus of tests/gates_cases.py: every graph that lowers, bound fillers that bring an
operand to the top of what the compiler lets through, rotations beyond the domain, a constant table and a live-value count at the
LDS budget, a program above the blob ring's slot size; on words uniform sampling never gives (every word r - 1, every word 0,
columns and rows that alternate between them); on row counts below a workgroup and off every tile; through the interpreter, the
three ahead-of-time kernels, forced tiles and the lowering's knobs; back to back through the blob ring and past the program
cache's capacity.

Every expected row comes from the C oracle (gates_cases.expected_rows), which tests/test_gates_cases_cpu.py holds against halo2's
definition in Python integers on every one of these programs and patterns; every comparison is equality of 32-byte words."""
import contextlib
import os
import re
import threading

import numpy as np
import pytest

import gates_cases as gc

pytestmark = pytest.mark.gpu

EXTENDED = [(1, 1), (2, 5), (5, 7), (6, 6)]                    # (k, ext_k)
COSET_MAJOR = [(5, 1), (5, 5), (5, 8), (6, 5), (1, 1)]         # (k, cosets): 32, 160, 256, 320 = 256 + 64 and 2 rows
MAIN = [(5, 7, 0), (5, 5, 5)]                                  # (k, ext_k, cosets) of the runs that take the whole corpus
OTHER = [(k, e, 0) for k, e in EXTENDED if (k, e) != (5, 7)] + [(k, k, c) for k, c in COSET_MAJOR if (k, c) != (5, 5)]
_REF = {}


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    import circuits_halo2_amd as sg
    from circuits_halo2_amd import ffi
    ffi.check(sg.lib().sg_init(0))
    yield sg
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@contextlib.contextmanager
def _env(**knobs):
    """SG_GATES_<knob> for the calls inside (the library reads them at every call)"""
    names = ["SG_GATES_" + k.upper() for k in knobs]
    for n, v in zip(names, knobs.values()):
        os.environ[n] = str(v)
    try:
        yield
    finally:
        for n in names:
            os.environ.pop(n, None)


def _rows(k, ext_k, cosets):
    return (cosets << k) if cosets else (1 << ext_k)


def _expect(O, case, pattern, k, ext_k, cosets, seed=0):
    """(inputs, expected rows), computed once and shared (read only)"""
    key = (case.name, case.dims, pattern, k, ext_k, cosets, seed)
    if key not in _REF:
        inp = gc.make_inputs(O, case, pattern, _rows(k, ext_k, cosets), seed)
        want = gc.expected_rows(O, case, inp, k, ext_k, cosets)
        want.setflags(write=False)
        _REF[key] = (inp, want)
    return _REF[key]


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def _upload(inp):
    return {"values": _dev(inp["previous"]), **{g: [_dev(c) for c in inp[g]] for g in ("fixed", "advice", "instance")}}


def _launch(case, inp, d, k, ext_k, cosets):
    """the asynchronous call; the rows land in d["values"]"""
    from circuits_halo2_amd import arithmetic as A
    args = (d["values"], gc.GraphWithConstants(case, inp["constants"]), d["fixed"], d["advice"], d["instance"], inp["challenges"], inp["beta"],
            inp["gamma"], inp["theta"], inp["y"], k)
    return A.quotient_gates_cosets(*args, cosets) if cosets else A.quotient_gates(*args, ext_k)


def _run(case, inp, k, ext_k, cosets):
    return _launch(case, inp, _upload(inp), k, ext_k, cosets).cpu().numpy()


def _same(got, want, what):
    bad = (got.reshape(-1, 32) != want.reshape(-1, 32)).any(axis=1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} rows differ, first at row {int(np.argmax(bad))}"


def _check(O, case, pattern, k, ext_k, cosets, seed=0):
    inp, want = _expect(O, case, pattern, k, ext_k, cosets, seed)
    _same(_run(case, inp, k, ext_k, cosets), want, (case.name, pattern, k, ext_k, cosets))


def _refused(O, case, pattern, k, ext_k, cosets):
    from circuits_halo2_amd.ffi import SummaGpuError
    inp = gc.make_inputs(O, case, pattern, _rows(k, ext_k, cosets))
    with pytest.raises(SummaGpuError):
        _run(case, inp, k, ext_k, cosets)


# ----------------------------------------------------------------------------- the interpreter
@pytest.mark.parametrize("pattern", gc.PATTERNS)
def test_interpreter_on_the_whole_corpus(gpu, O, pattern):
    """every device-corpus program at k = 5 over the extended domain (ext_k = 7) and over 5 cosets of 2^5 rows; the two programs
    of 64 and more live values are refused"""
    with _env(generic=1):
        for case in gc.device_corpus(O):
            for k, ext_k, cosets in MAIN:
                if case.name in gc.REFUSED:
                    _refused(O, case, pattern, k, ext_k, cosets)
                else:
                    _check(O, case, pattern, k, ext_k, cosets)


def _edge_programs(O):
    names = [f"rotations_k{k}" for k in gc.ROTATION_KS] + gc.BOUND_FILLERS + ["result_constant", "result_column", "result_previous_value"]
    names += ["random_seed80_calc8_inst1_chal2", "random_seed400_calc40_inst1_chal2", "random_seed1200_calc120_inst1_chal2",
              "random_seed3000_calc300_inst1_chal2", "random_folded_seed501_calc8", "random_folded_seed502_calc40",
              "random_folded_seed505_calc120", "random_folded_seed507_calc300"]
    return [gc.device_case(O, n) for n in names]


@pytest.mark.parametrize("k,ext_k,cosets", OTHER)
def test_interpreter_at_the_other_shapes(gpu, O, k, ext_k, cosets):
    """two rows, ext_k = k, fewer rows than a workgroup, the most cosets, a row total off every tile: the rotation programs (their
    rotations wrap more than once at k = 1 and 2), the bound fillers, a random program of each size and the three results that
    are no computed value"""
    with _env(generic=1):
        for case in _edge_programs(O):
            for pattern in gc.PATTERNS:
                _check(O, case, pattern, k, ext_k, cosets)


def test_interpreter_tile_at_the_lds_budget(gpu, O, capfd):
    """63 slots, and 40 slots beside 1504 constants: 64 rows per workgroup, within one slot of the budget"""
    for name, line in (("live_values_62", "63 slots, 4 constants -> 64 rows per workgroup"),
                       ("many_constants", "40 slots, 1504 constants -> 64 rows per workgroup")):
        for k, ext_k, cosets in MAIN:
            capfd.readouterr()
            with _env(generic=1, debug=1):
                _check(O, gc.device_case(O, name), "top", k, ext_k, cosets)
            err = capfd.readouterr().err
            assert line in err, err


# ----------------------------------------------------------------------------- the three ahead-of-time kernels
def _circuit_case(O, nc, n_advice=None):
    from circuits_halo2_amd import mst_inclusion as M
    if n_advice is None:
        return gc.device_case(O, f"mst_gates_nc{nc}")
    return gc.Case(f"mst_gates_nc{nc}_advice{n_advice}", M.gate_graph(nc), M.NUM_FIXED, n_advice, 0, len(M.gate_challenge_exponents(nc)))


@pytest.mark.parametrize("nc", [1, 2, 3, 4])
def test_ahead_of_time_gate_programs(gpu, O, capfd, nc):
    """the circuit's gate program with its 14 columns as kernel arguments, with 25 columns in the blob (11 fixed, 14 advice of which
    it reads three: one more than travel by value), and through the interpreter: the oracle's rows each way, by the kernel named"""
    ways = [(_circuit_case(O, nc), {}, lambda err: f"ahead-of-time program MstGatesNc{nc} (arguments by value)" in err),
            (_circuit_case(O, nc, 14), {}, lambda err: f"ahead-of-time program MstGatesNc{nc}," in err and "(arguments by value)" not in err),
            (_circuit_case(O, nc), {"generic": 1}, lambda err: "ahead-of-time" not in err and "rows per workgroup" in err)]
    for case, knobs, named in ways:
        for pattern in gc.PATTERNS:
            for k, ext_k, cosets in MAIN:
                capfd.readouterr()
                with _env(debug=1, **knobs):
                    _check(O, case, pattern, k, ext_k, cosets)
                err = capfd.readouterr().err
                assert named(err), (case.name, knobs, err)


def test_ahead_of_time_lookup_input(gpu, O, capfd):
    """the lookup's input expression by value and through the interpreter (its blob form is the interpreter by design)"""
    case = gc.device_case(O, "mst_lookup_input")
    for knobs, named in (({}, lambda err: "ahead-of-time program MstLookupInput (arguments by value)" in err),
                         ({"generic": 1}, lambda err: "ahead-of-time" not in err and "rows per workgroup" in err)):
        for pattern in gc.PATTERNS:
            for k, ext_k, cosets in MAIN:
                capfd.readouterr()
                with _env(debug=1, **knobs):
                    _check(O, case, pattern, k, ext_k, cosets)
                err = capfd.readouterr().err
                assert named(err), (knobs, err)


# ----------------------------------------------------------------------------- forced tiles, lowering variants
@pytest.mark.parametrize("forced", [64, 128, 256])
def test_forced_tiles(gpu, O, capfd, forced):
    """8 live values (256 rows per workgroup by the rule) at every forced size, on 160 and on 320 rows"""
    case = gc.device_case(O, "live_values_7")
    for k, cosets in ((5, 5), (6, 5)):
        for pattern in gc.PATTERNS:
            capfd.readouterr()
            with _env(debug=1, rows=forced):
                _check(O, case, pattern, k, k, cosets)
            err = capfd.readouterr().err
            assert f"8 slots, 4 constants -> {forced} rows per workgroup" in err, err


def _counts(err):
    """(instructions, slots) of the interpreter's debug line"""
    m = re.search(r"gates: (\d+) ops, (\d+) slots", err)
    assert m, err
    return int(m.group(1)), int(m.group(2))


def test_lowering_variants_after_the_default(gpu, O, capfd):
    """SG_GATES_RELOAD and SG_GATES_CONVERT on graphs this lane has already compiled with the default lowering: the oracle's rows,
    and the program that ran is the one of the lowering in force (its instruction and slot counts are those of
    gates_program_words, which compiles afresh), not the cached one"""
    from circuits_halo2_amd import arithmetic as A
    cases = [gc.device_case(O, n) for n in ("random_folded_seed504_calc120", "long_lazy_chain", "mst_gates_nc2")]
    k, ext_k, cosets = 5, 7, 0

    def run(case, **knobs):
        capfd.readouterr()
        with _env(generic=1, debug=1, **knobs):
            _check(O, case, "rows_cycle", k, ext_k, cosets)
            _check(O, case, "top", k, ext_k, cosets)
            words = A.gates_program_words(case.graph, *case.dims)
        got = _counts(capfd.readouterr().err)
        assert got == (words[3], words[0]), (case.name, knobs, got)
        return got
    default = {c.name: run(c) for c in cases}
    for knobs in ({"reload": 0}, {"reload": 48}, {"convert": 0}, {"convert": 1}):
        variant = {c.name: run(c, **knobs) for c in cases}
        assert variant != default, knobs
        assert {c.name: run(c) for c in cases} == default        # and back


# ----------------------------------------------------------------------------- refusals
def test_refusals_leave_the_lane_usable(gpu, O):
    """64 live values fit no tile (every program carries beta, gamma, theta and y), a forced tile may not fit either: error
    returns, and the next call is right"""
    k, ext_k, cosets = 5, 7, 0
    _refused(O, gc.device_case(O, "live_values_63"), "random", k, ext_k, cosets)
    _check(O, gc.device_case(O, "live_values_62"), "random", k, ext_k, cosets)
    with _env(rows=256):
        _refused(O, gc.device_case(O, "live_values_39"), "random", k, ext_k, cosets)
    _check(O, gc.device_case(O, "live_values_39"), "random", k, ext_k, cosets)


# ----------------------------------------------------------------------------- the blob ring, the program cache
RING_PROGRAMS = ["random_folded_seed506_calc300", "many_constants", "large_program", "mst_gates_nc2", "long_lazy_chain"]


def _back_to_back(O, n_calls, seed0):
    """n_calls on one stream of its own with no host wait between them, rotating through five programs (the large one grows a ring
    slot on the way), each call with constants, challenges and an output buffer of its own; one synchronise, then every output is
    compared.  Returns the mismatches."""
    import torch
    k, cosets = 5, 5
    cases = [gc.device_case(O, n) for n in RING_PROGRAMS]
    calls = []
    for i in range(n_calls):
        case = cases[i % len(cases)]
        inp, want = _expect(O, case, "random" if i % 2 else "rows_cycle", k, k, cosets, seed=seed0 + i)
        calls.append((case, inp, want, _upload(inp)))
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        for case, inp, _, d in calls:
            _launch(case, inp, d, k, k, cosets)
    stream.synchronize()
    wrong = []
    for i, (case, _, want, d) in enumerate(calls):
        got = d["values"].cpu().numpy()
        if (got != want).any():
            wrong.append((i, case.name, int((got.reshape(-1, 32) != want.reshape(-1, 32)).any(axis=1).sum())))
    return wrong


def test_blob_ring_back_to_back(gpu, O):
    """40 calls through the 16 slots: a slot is reused only behind the event of the launch that read it"""
    with _env(generic=1):
        assert _back_to_back(O, 40, 1000) == []


def test_blob_ring_from_two_threads(gpu, O):
    """the same from two host threads at once, 20 calls each on a stream of their own"""
    out = {}

    def work(t):
        try:
            out[t] = _back_to_back(O, 20, 2000 + 100 * t)
        except BaseException as e:      # noqa: BLE001  (reported by the assertion below)
            out[t] = repr(e)
    for t in range(2):                  # (the expectations first, one thread at a time: the oracle's work is not under test)
        for i in range(20):
            _expect(O, gc.device_case(O, RING_PROGRAMS[i % 5]), "random" if i % 2 else "rows_cycle", 5, 5, 5, seed=2000 + 100 * t + i)
    with _env(generic=1):
        threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
    assert out == {0: [], 1: []}


def test_program_cache_turnover(gpu, O):
    """more than 64 distinct programs through one lane (the cache is cleared wholesale at 64), then the first four again with
    new constants"""
    k, cosets = 5, 1
    cases = [c for c in gc.device_corpus(O) if c.name not in gc.REFUSED]
    assert len(cases) > 64
    with _env(generic=1):
        for case in cases:
            _check(O, case, "random", k, k, cosets)
        for case in cases[:4]:
            _check(O, case, "random", k, k, cosets, seed=77)
            _check(O, case, "top", k, k, cosets)
