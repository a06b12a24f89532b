"""The host side of the commitments, without a GPU: csrc/commit_plan.h (which basis and table a commitment runs against, how
a batch is cut into fused jobs, how a host-pointer call is cut into chunks and in which order they run) and
csrc/commit_combiner.h (the commit combiner), each built by the host compiler into a stand-alone program of tests/cpp/ --
once plainly, once under address / undefined sanitizers, the combiner a third time under the thread sanitizer -- and compared
with the rules restated here.  Nothing is loaded into Python."""
import itertools
import os
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "circuits_halo2_amd", "csrc")
MAX_FUSED, SPARSE = 64, 16
SAN = {"plain": [], "sanitized": ["-fsanitize=address,undefined"],
       # the thread sanitizer's runtime of g++ 11 does not intercept pthread_cond_clockwait, which a wait_until on steady_clock
       # makes: it then reports a mutex locked twice and races under a held mutex that are not there.  The deadline's clock is
       # one alias, and this build names system_clock through it; the other two keep the production clock
       "thread": ["-fsanitize=thread", "-DSG_COMBINER_CLOCK=std::chrono::system_clock"]}


def build(tmp_path_factory, name, variant):
    out = str(tmp_path_factory.mktemp(name) / f"{name}_{variant}")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-pthread"] + SAN[variant] + \
          ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", out]
    if variant == "thread":
        probe = out + "_probe.cpp"
        with open(probe, "w") as f:
            f.write("int main() { return 0; }\n")
        r = subprocess.run(["g++", "-fsanitize=thread", probe, "-o", out + "_probe"], capture_output=True, text=True)
        if r.returncode != 0 or subprocess.run([out + "_probe"], capture_output=True).returncode != 0:
            pytest.skip("g++ -fsanitize=thread does not build a program that starts on this machine: " + r.stderr[-300:])
    subprocess.check_call(cmd)
    return out


def run(exe, args=(), stdin=""):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1", TSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe] + list(args), input=stdin, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert not re.search(r"runtime error|AddressSanitizer|ThreadSanitizer", r.stderr), r.stderr[-3000:]
    return r.stdout.splitlines()


# ============================================================================= commit_plan.h
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def plan_exe(request, tmp_path_factory):
    return build(tmp_path_factory, "commit_plan_check", request.param)


def ask(exe, commands):
    out = run(exe, stdin="\n".join(commands) + "\n")
    assert len(out) == len(commands)
    return out


def tables(present, plans=None):
    """three (present, c, n) triples; plans: {table: (c, n)} where a table is not on the plan (9, 16)"""
    return " ".join(f"{int(j in present)} {c} {n}" for j in range(3) for c, n in [(plans or {}).get(j, (9, 16))])


def test_one_basis_resolves_to_a_basis_a_form_and_a_table(plan_exe):
    """basis 2 is basis 1 unless the prefix table exists and the column has all 2^k rows; fixed-base if the table of the
    basis that runs exists; a host-pointer commitment goes in chunks if it is not fixed-base and has 2^18 scalars"""
    k = 4
    cases = [(basis, set(present), n) for basis in range(3) for r in range(4) for present in itertools.combinations(range(3), r)
             for n in (0, 1, (1 << k) - 1, 1 << k)]
    assert len(cases) == 3 * 8 * 4
    out = ask(plan_exe, [f"s {k} {basis} {n} {tables(present)}" for basis, present, n in cases])
    for (basis, present, n), line in zip(cases, out):
        diff = basis == 2 and 2 in present and n == 1 << k
        b = basis if basis < 2 or diff else 1
        fixed = b in present
        assert [int(x) for x in line.split()] == [b, int(diff), int(fixed), b if fixed else -1, 0], (basis, present, n)
    # the chunk predicate where it can hold: k = 18, all 2^18 rows and one row fewer
    big = [(basis, set(present), n) for basis in range(3) for r in range(4) for present in itertools.combinations(range(3), r)
           for n in ((1 << 18) - 1, 1 << 18)]
    out = ask(plan_exe, [f"s 18 {basis} {n} {tables(present)}" for basis, present, n in big])
    for (basis, present, n), line in zip(big, out):
        b = 2 if basis == 2 and 2 in present and n == 1 << 18 else min(basis, 1)
        assert int(line.split()[4]) == int(b not in present and n >= 1 << 18), (basis, present, n)
    assert sum(int(line.split()[4]) for line in out) == 10       # of the 24 full-length cases; never one of the short ones


# the table sets tests/test_gpu_parity.py walks on the device (test_difference_form_commitments, ..._large_known_answer)
MIXED_TABLES = {"tables 1 and 2 only": ({1, 2}, None),
                "all three on one plan": ({0, 1, 2}, None),
                "the prefix table on another c": ({0, 1, 2}, {2: (8, 16)}),
                "the prefix table on another n": ({0, 1, 2}, {2: (9, 32)}),
                "tables 0 and 1 on different plans": ({0, 1, 2}, {1: (8, 16)})}
MIXED_COLUMNS = [[2, 2, 2, 1], [1, 1, 1, 2, 2], [0 | SPARSE, 1 | SPARSE, 2 | SPARSE], [0 | SPARSE, 1, 2 | SPARSE]]


def test_a_mixed_job_runs_on_one_path(plan_exe):
    k = 4
    cases = [(name, cols, n) for name in MIXED_TABLES for cols in MIXED_COLUMNS for n in (1 << k, (1 << k) - 1)]
    out = ask(plan_exe, [f"m {k} {n} {tables(*MIXED_TABLES[name])} {len(cols)} " + " ".join(map(str, cols)) for name, cols, n in cases])
    for (name, cols, n), line in zip(cases, out):
        present, plans = MIXED_TABLES[name]
        plan = lambda j: (plans or {}).get(j, (9, 16))
        fixed = {0, 1} <= present and plan(0) == plan(1)
        diff_ok = fixed and 2 in present and n == 1 << k and plan(2) == plan(0)
        b = [(2 if diff_ok else 1) if c & ~SPARSE == 2 else c & ~SPARSE for c in cols]
        head, got_b, got_flags = ([int(x) for x in part.split()] for part in line.split("|"))
        assert head == [int(fixed), int(diff_ok), int(all(c & SPARSE for c in cols))], (name, cols, n)
        assert got_b == b and got_flags == [int(x == 2) for x in b], (name, cols, n)
    # what the cases are there for
    answers = {(name, n): line.split("|")[0].split()[:2] for (name, cols, n), line in zip(cases, out)}
    assert answers["tables 1 and 2 only", 16] == ["0", "0"] and answers["all three on one plan", 16] == ["1", "1"]
    assert answers["all three on one plan", 15] == ["1", "0"]
    assert answers["the prefix table on another c", 16] == answers["the prefix table on another n", 16] == ["1", "0"]
    assert ask(plan_exe, [f"m {k} 16 {tables({0, 1, 2})} 0"]) == ["1 1 0 | |"]            # no column is not "all sparse"


def test_the_sparse_hint_is_for_small_fixed_base_jobs_of_sparse_columns(plan_exe):
    cases = list(itertools.product((0, 1), (0, 1), (5, 6), (0, 3), ((1 << 14) - 1, 1 << 14)))
    out = ask(plan_exe, ["h " + " ".join(map(str, c)) for c in cases])
    for (all_sparse, fixed, count, log_seg, n), line in zip(cases, out):
        assert int(line) == int(bool(all_sparse and fixed and count <= 5 and log_seg == 0 and n >= 1 << 14)), (all_sparse, fixed, count, log_seg, n)
    assert [c for c, line in zip(cases, out) if line == "1"] == [(1, 1, 5, 0, 1 << 14)]


def test_groups_cover_a_batch_in_order_without_mixing_lengths(plan_exe):
    a, b = 1 << 17, 700
    lengths = [a, a, a, b, b, a, 0, 0]
    limits = [1, 2, 64]
    out = ask(plan_exe, [f"g {lim} {len(lengths)} " + " ".join(map(str, lengths)) for lim in limits])
    want = {1: [(0, 1), (1, 1), (2, 1), (3, 1), (4, 1), (5, 1), (6, 2)],          # (a length of 0 has the limit MAX_FUSED in the program)
            2: [(0, 2), (2, 1), (3, 2), (5, 1), (6, 2)],
            64: [(0, 3), (3, 2), (5, 1), (6, 2)]}
    for lim, line in zip(limits, out):
        groups = [tuple(int(x) for x in g.split(":")) for g in line.split()]
        assert [i for first, count in groups for i in range(first, first + count)] == list(range(len(lengths))), lim
        for first, count in groups:
            assert len(set(lengths[first:first + count])) == 1 and 1 <= count <= (lim if lengths[first] else MAX_FUSED), (lim, first)
        assert groups == want[lim], lim
    assert ask(plan_exe, ["g 4 0"]) == [""]


def test_chunks_of_a_host_pointer_call(plan_exe):
    sizes = [0, 1, 3, (1 << 18) - 1, 1 << 18, (1 << 20) + 7]
    cases = [(p, n) for p in range(9) for n in sizes]
    out = ask(plan_exe, [f"c {p} {n}" for p, n in cases])
    for (p, n), line in zip(cases, out):
        K, *lo = (int(x) for x in line.split())
        want = min(p if p else (1 if n < 1 << 18 else 2), 8)
        assert K == (1 if n < 2 * want else want) and 1 <= K <= 8, (p, n)
        assert len(lo) == K + 1 and lo[0] == 0 and lo[K] == n and lo == sorted(lo) and lo == [n * i // K for i in range(K + 1)], (p, n)
        if K > 1:
            assert min(hi - low for low, hi in zip(lo, lo[1:])) >= 2, (p, n)
    assert [line.split()[0] for (p, n), line in zip(cases, out) if p == 0] == ["1", "1", "1", "1", "2", "2"]    # 2 exactly from 2^18
    assert ask(plan_exe, ["c -1 1000", "c 100 1000"]) == ask(plan_exe, ["c 8 1000"]) * 2                        # clamped to 8


# ----------------------------------------------------------------------------- the chunk pipeline
CLEAN = {2: "S0 B0 F0 b0 S1 B1 F1 b1 f0 f1",
         3: "S0 B0 F0 b0 S1 B1 F1 b1 S2 B2 f0 F2 b2 f1 f2"}


def expand_order_comment(K):
    """`[S0 B0] front(0) { back(i) [S i+1 B i+1] finish(i-1) front(i+1) } ... finish`, the line in msm_host_chunked's comment
    block, written out for K chunks: the braces once per chunk, what names a chunk that does not exist left out, and every
    job still open finished at the end"""
    src = open(os.path.join(CSRC, "abi_msm.hip")).read()
    assert "//   [S0 B0] front(0) { back(i) [S i+1 B i+1] finish(i-1) front(i+1) } ... finish, sum\n" in src
    calls = ["S0", "B0", "F0"]
    for i in range(K):
        calls.append(f"b{i}")
        if i + 1 < K:
            calls += [f"S{i + 1}", f"B{i + 1}"] + ([f"f{i - 1}"] if i >= 1 else []) + [f"F{i + 1}"]
    return calls + [f"f{i}" for i in range(max(K - 2, 0), K)]


def pipeline(exe, cases):
    out = ask(exe, [f"p {K} {op} {i}" for K, op, i in cases])
    res = []
    for line in out:
        *calls, ret = line.split()
        res.append((calls, int(ret[len("ret="):])))
    return res


def check_record(K, calls, ret, what):
    """the rules of run_chunk_pipeline on one record (a call that failed ends in `!`)"""
    failed = [c for c in calls if c.endswith("!")]
    names = [c.rstrip("!") for c in calls]
    assert len(set(names)) == len(names), what                                  # nothing is called twice
    at = {c: j for j, c in enumerate(names)}
    ok = lambda c: c in at and c + "!" not in calls
    # the first error is the one returned, and after it nothing new starts: no copy, no front
    assert len(failed) <= 1 and (ret == 0) == (not failed), what
    if failed:
        op, i = failed[0][0], int(failed[0][1:-1])
        assert ret == 1000 + 10 * ord(op) + i, what
        assert not [c for c in names[at[failed[0][:-1]] + 1:] if c[0] in "SBF"], what
    for i in range(K):
        # every fronted chunk gets exactly one back, every chunk whose back succeeded exactly one finish; nothing else gets either
        assert (f"b{i}" in at) == ok(f"F{i}") and (f"f{i}" in at) == ok(f"b{i}"), (what, i)
        if f"F{i}" in at:
            assert at[f"S{i}"] < at[f"B{i}"] < at[f"F{i}"], (what, i)             # a chunk's copies are on their way before its job starts
        if f"F{i + 1}" in at and i >= 1:
            assert at[f"f{i - 1}"] < at[f"F{i + 1}"], (what, i)                   # finish(i - 1) precedes front(i + 1): they share an engine
    # per engine: front, back, finish, front, ... -- never a front on an engine with an open job, and no job left open
    for e in range(2):
        state = "idle"
        for c in calls:
            if int(c.rstrip("!")[1:]) & 1 != e or c[0] in "SB":
                continue
            assert (state, c[0]) in (("idle", "F"), ("fronted", "b"), ("backed", "f")), (what, e, c)
            state = "idle" if c.endswith("!") or c[0] == "f" else {"F": "fronted", "b": "backed"}[c[0]]
        assert state == "idle", (what, e)


def test_the_chunk_pipeline_keeps_its_order_and_closes_every_job(plan_exe):
    for K in range(2, 9):
        (clean, ret), = pipeline(plan_exe, [(K, "-", 0)])
        assert clean == expand_order_comment(K) and ret == 0, K
        assert len(clean) == 5 * K
        check_record(K, clean, ret, f"K = {K}")
        if K in CLEAN:
            assert " ".join(clean) == CLEAN[K], K
        cases = [(K, c[0], int(c[1:])) for c in clean]
        for (_, op, i), (calls, ret) in zip(cases, pipeline(plan_exe, cases)):
            what = f"K = {K}, {op}{i} fails: " + " ".join(calls)
            assert f"{op}{i}!" in calls, what
            assert calls[:calls.index(f"{op}{i}!")] == clean[:clean.index(f"{op}{i}")], what     # up to the failure, the clean order
            check_record(K, calls, ret, what)
    (one, ret), = pipeline(plan_exe, [(1, "-", 0)])
    assert one == ["S0", "B0", "F0", "b0", "f0"] and ret == 0


# ============================================================================= commit_combiner.h
@pytest.fixture(scope="module", params=["plain", "sanitized", "thread"])
def combiner_exe(request, tmp_path_factory):
    return build(tmp_path_factory, "commit_combiner_check", request.param)


def figures(lines):
    assert lines[-1] == "ok" and len(lines) == 2, lines
    return {k: int(v) for k, v in (kv.split("=") for kv in lines[0].split())}


@pytest.mark.parametrize("runners", [1, 2])
def test_combiner_under_load_serves_every_request_once(combiner_exe, runners):
    """eight member threads, 50 requests of 3 polynomials each over two SRS handles and two lengths; target 4, a wait of
    100 000 us.  The program checks that every request returns once with its own outputs, that no job mixes (SRS, n) or
    exceeds MAX_FUSED polynomials, that the jobs' sizes add up to the requests, and that the combiner is empty at the end"""
    f = figures(run(combiner_exe, ["load", str(runners)]))
    assert f["requests"] == 400 and f["isolated"] == 0 and 1 <= f["max_running"] <= runners
    assert 400 // 8 <= f["jobs"] <= 400               # no job holds two requests of one thread


def test_one_bad_member_costs_the_others_nothing(combiner_exe):
    """four requests pending together, one with a null scalar pointer: the fused job fails as a whole, every member is re-run
    alone, the poisoned one gets the failure code and the message of its own job, the others their outputs"""
    assert figures(run(combiner_exe, ["bad_member"])) == {"jobs": 5, "requests": 4, "isolated": 4, "max_running": 1}


def test_an_injected_failure_isolates_and_a_single_member_job_leaves_the_flag(combiner_exe):
    """the debug hook fails the fused job of four before it runs: four re-runs, all good, the flag taken; set again, a job of
    one member does not ask the hook and leaves the flag set"""
    assert figures(run(combiner_exe, ["injected"])) == {"jobs": 5, "requests": 5, "isolated": 4, "max_running": 1}


def test_nobody_waits_for_a_member_that_never_submits(combiner_exe):
    assert figures(run(combiner_exe, ["absent"])) == {"jobs": 1, "requests": 1, "isolated": 0, "max_running": 1}


def test_requests_that_do_not_fit_one_job_run_as_two(combiner_exe):
    """two requests of 40 polynomials, same SRS and length, pending together: MAX_FUSED is 64"""
    assert figures(run(combiner_exe, ["oversized"])) == {"jobs": 2, "requests": 2, "isolated": 0, "max_running": 1}


# ============================================================================= where the decisions live
def test_abi_msm_holds_no_decision_of_its_own():
    src = open(os.path.join(CSRC, "abi_msm.hip")).read()
    assert "condition_variable" not in src and "<deque>" not in src and "diff_form_ready" not in src
    for signature, header in (("BasisChoice resolve_basis(", "commit_plan.h"), ("MixedChoice resolve_mixed(", "commit_plan.h"),
                              ("run_chunk_pipeline(uint32_t K", "commit_plan.h"), ("struct Combiner {", "commit_combiner.h")):
        sources = [name for name in sorted(os.listdir(CSRC)) if name.endswith((".h", ".hip", ".cuh", ".inc"))]
        assert [name for name in sources if signature in open(os.path.join(CSRC, name)).read()] == [header], signature
    for header in ("commit_plan.h", "commit_combiner.h"):
        text = open(os.path.join(CSRC, header)).read()
        assert "#include <hip" not in text and "abi_internal.h" not in text, header
        assert header in open(os.path.join(CSRC, "Makefile")).read()
