"""CPU checks of tests/ntt_cases.py, the plan rules and the case list behind tests/test_gpu_ntt_plans.py: the restatement says
what the engine's own rules say (csrc/ntt_plan.h through tests/cpp/ntt_plan_check.cpp), every launch the parameter table allows
stays within the LDS and thread limits of the kernels, the default plans are the recorded ones, and the GPU cases reach every
variant of a pass.  A case list that silently stopped reaching the three-pass transposing store fails here, without a GPU."""
import itertools
import os
import subprocess

import pytest

import ntt_cases as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = [(0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (1, 1, 0, 0)]   # scale, pre3, post3, pre_tab


def test_defaults_and_ranges_are_the_documented_ones():
    from param_doc import ROOT as root, documented_defaults
    import re
    doc = documented_defaults()
    assert nc.DEFAULTS == {k: doc[k] for k in nc.DEFAULTS} and {k for k in doc if k.startswith("ntt.")} == set(nc.DEFAULTS)
    hdr = open(os.path.join(root, "include", "summa_gpu.h")).read()
    for name, (lo, hi) in nc.RANGES.items():
        m = re.search(r'^ \*   "%s" +(0 \| )?(\d+)\.\.(\d+), default' % re.escape(name), hdr, flags=re.M)
        assert m and (int(m[2]), int(m[3])) == (lo, hi) and bool(m[1]) == (name == "ntt.big_tile_log"), name


def _configs(ranges=nc.RANGES):
    """the configurations of the grid: every parameter at each of its boundary points (lowest, one step inside, default, one
    step inside, highest) with the others at their defaults, and the parameters that meet in one decision crossed at lowest /
    default / highest: the plan cuts with the tile and the threads of either shape under each kernel choice (the LDS of a
    launch is a function of all of them), and the four parameters that choose the throughput shape with each other"""
    def ends(name):
        lo, hi = ranges[name]
        return sorted({lo, nc.DEFAULTS[name], hi} | ({0} if name == "ntt.big_tile_log" else set()))
    names = [n for n in nc.DEFAULTS if n != "ntt.coset_scale_pass"]     # (that one decides what a caller passes, not a launch)
    out = [{}] + [{n: v} for n in names for v in nc.boundary_points(n, ranges)]
    cuts = list(itertools.product(ends("ntt.max_single_log"), ends("ntt.max_multi_log")))
    for (ms, mm), r4 in itertools.product(cuts, ends("ntt.radix4")):
        base = {"ntt.max_single_log": ms, "ntt.max_multi_log": mm, "ntt.radix4": r4}
        for tile, thr in itertools.product(ends("ntt.tile_log"), ends("ntt.threads")):
            out.append(dict(base, **{"ntt.tile_log": tile, "ntt.threads": thr, "ntt.big_tile_log": 0}))
        for tile, thr in itertools.product(ends("ntt.big_tile_log"), ends("ntt.big_threads")):
            out.append(dict(base, **{"ntt.big_tile_log": tile, "ntt.big_threads": thr, "ntt.batch_min": 1}))
    for btile, bmin, blog, r4 in itertools.product((0, 10), nc.boundary_points("ntt.batch_min"), nc.boundary_points("ntt.big_log"),
                                                   ends("ntt.radix4")):
        out.append({"ntt.big_tile_log": btile, "ntt.batch_min": bmin, "ntt.big_log": blog, "ntt.radix4": r4})
    return out


def _jobs(log_ns=range(1, 29)):
    """log_n 1 .. 28 x in_len in {n, n/2, n/8, n/64} x nbatch in {0, 1, 3, 4, 32}; what rides on the passes rotates with them"""
    jobs = []
    for log_n in log_ns:
        for i, shift in enumerate((0, 1, 3, 6)):
            for j, nbatch in enumerate((0, 1, 3, 4, 32)):
                jobs.append((log_n, (1 << log_n) >> shift, nbatch) + FLAGS[(log_n + i + 2 * j) % len(FLAGS)])
    return jobs


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ntt") / "ntt_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "circuits_halo2_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "ntt_plan_check.cpp"), "-o", exe])

    def run(cases):
        text = "".join(f"{log_n} {in_len} {nbatch} {sc} {pre} {post} {tab} {nc.check_args(params)}\n"
                       for params, (log_n, in_len, nbatch, sc, pre, post, tab) in cases)
        got = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split("\n")[:-1]
        assert len(got) == len(cases)
        return got
    return run


def _restated(params, job, **kw):
    log_n, in_len, nbatch, sc, pre, post, tab = job
    return nc.plan(params, log_n, in_len, nbatch, bool(sc), bool(pre), bool(post), bool(tab), **kw)


def test_restated_rules_are_the_engines_own_and_every_launch_fits(plan_check):
    """tests/cpp/ntt_plan_check.cpp runs the engine's planning (csrc/ntt_plan.h, no HIP) on every job of the grid; ntt_cases.plan
    must say the same, field by field: the GPU tests name the variant a case exercises on the strength of the restatement.  And
    every job of the grid -- every value the parameter table accepts, at its boundary points -- is a chain of launches the kernels
    can take: dynamic LDS <= 160 KiB, threads <= 1024 (512 for the radix-4 kernel), no pass of length 1, lengths that multiply to
    n.  The C++ rules are the reference: a difference is fixed in ntt_cases.py."""
    cases = list(itertools.product(_configs(), _jobs()))
    assert len(cases) > 100000
    got = plan_check(cases)
    biggest = 0
    for line, (params, job) in zip(got, cases):
        p = _restated(params, job)
        want = nc.plan_line(p)
        if line != want:
            diff = [(a, b) for a, b in zip(line.split(" "), want.split(" ")) if a != b]
            raise AssertionError(f"{params} {job}: engine / restatement {diff or (line, want)}")
        assert not nc.limits_broken(p, job[0]), (params, job, nc.limits_broken(p, job[0]))
        biggest = max(biggest, max(s["lds"] for s in p["passes"]))
    assert biggest == nc.lds_bytes(9, 3) == 157024      # the budget is used: a 2^12-element tile beside a pass of 2^9 points


def test_the_rules_before_the_fix_exceeded_the_lds():
    """the defect this file was written around, from the formula alone: with the ranges the table took before (both plan cuts up
    to 12) and no narrowing of the tile, launches ask for more than 160 KiB -- the listed ones, and on the grid only launches of
    these three kinds; under the present rules the same jobs fit, or the value is no longer accepted"""
    old = lambda params, log_n, **kw: nc.plan(params, log_n, fit_lds=False, **kw)
    worst = lambda p: max(s["lds"] for s in p["passes"])
    assert worst(old({"ntt.max_single_log": 12}, 12)) == 221536
    assert worst(old({"ntt.max_multi_log": 12}, 23)) == 221536 and worst(old({"ntt.max_multi_log": 12}, 24)) == 221536
    assert worst(old({"ntt.max_multi_log": 10, "ntt.tile_log": 12}, 19)) == 166240
    # (from 2^ntt.big_log points on the throughput shape's tile is the one that counts)
    for tiles in ({"ntt.tile_log": 12, "ntt.big_tile_log": 0}, {"ntt.big_tile_log": 12}):
        assert worst(old(dict(tiles, **{"ntt.max_multi_log": 10}), 20)) == 166240
        assert worst(old(dict(tiles, **{"ntt.max_multi_log": 11}), 22)) == 184672
        assert worst(nc.plan(dict(tiles, **{"ntt.max_multi_log": 10}), 20)) == nc.lds_bytes(10, 1) == 92512
        assert worst(nc.plan(dict(tiles, **{"ntt.max_multi_log": 11}), 22)) == nc.lds_bytes(11, 0) == 110944
    over = set()
    for params, job in itertools.product(_configs(nc.PARENT_RANGES), _jobs()):
        for s in _restated(params, job, fit_lds=False)["passes"]:
            if s["lds"] > nc.LDS_BUDGET:
                over.add((s["log_r"], s["log_t"]))
    assert over == {(12, 0), (11, 1), (10, 2)}


# the default configuration's plans, recorded from the launch code before the rules moved into ntt_plan.h (csrc/ntt.hip, factor and
# launch_pass): per pass (kind, log_r, log_b, log_t, radix-4 kernel, threads, workgroups, dynamic LDS bytes)
RECORDED_DEFAULT_PLANS = {
    11: [("Y", 11, 0, 0, 0, 256, 1, 110944)],
    17: [("X", 8, 9, 1, 0, 256, 256, 23392), ("Y", 9, 8, 0, 0, 256, 256, 28000)],
    20: [("X", 6, 14, 4, 1, 256, 1024, 38368), ("Y", 7, 6, 3, 1, 256, 1024, 39520), ("Y", 7, 13, 3, 1, 256, 1024, 39520)],
    22: [("X", 7, 15, 3, 1, 256, 4096, 39520), ("Y", 7, 7, 3, 1, 256, 4096, 39520), ("Y", 8, 14, 2, 1, 256, 4096, 41824)],
}


@pytest.mark.parametrize("log_n", sorted(RECORDED_DEFAULT_PLANS))
def test_default_plans_are_the_recorded_ones(plan_check, log_n):
    """moving the rules changed no default plan or launch shape: the engine's rules give, for the default configuration, what the
    launch code gave before; a batch of 16 such transforms (log_n <= 18) takes the throughput shape"""
    line, = plan_check([({}, (log_n, 1 << log_n, 0, 0, 0, 0, 0))])
    p = nc.plan({}, log_n)
    assert line == nc.plan_line(p)
    got = [(s["kind"], s["log_r"], s["log_b"], s["log_t"], s["r4"], s["threads"], s["grid_x"], s["lds"]) for s in p["passes"]]
    assert got == RECORDED_DEFAULT_PLANS[log_n]
    if log_n == 17:
        b = nc.plan({}, log_n, nbatch=16)["passes"]
        assert [(s["log_t"], s["r4"], s["threads"], s["grid_x"], s["grid_y"]) for s in b] == [(2, 1, 256, 128, 16), (1, 1, 256, 128, 16)]


def test_gpu_cases_reach_every_variant():
    """the case list of tests/test_gpu_ntt_plans.py, run through the restatement, launches every variant of a pass at least once
    (a missing one is an error in the list); sizes stay small, with the one exception the list names"""
    cases = nc.gpu_cases()
    assert 100 <= len(cases) <= 170, len(cases)
    seen = set()
    for case in cases:
        assert case["k"] + case.get("ext", 0) <= 14 or case["k"] == nc.NARROWED_K, case["name"]
        if case.get("count", 0) > nc.BATCH_MAX or (case["op"] == "cosets" and case["count"] * nc.COSETS > nc.BATCH_MAX):
            seen.add("more than NTT_BATCH_MAX vectors")
        for t in nc.transforms_of(case):
            p = nc.plan(case["params"], **t)
            assert not nc.limits_broken(p, t["log_n"]), case["name"]
            seen.add(f"npass {p['npass']}")
            if t.get("scale"):
                seen.add("scale in the twiddle table" if p["scale_in_table"] else "scale as post3")
            cfg = nc.config(case["params"])
            for s in p["passes"]:
                r4 = "r4" if s["r4"] else "r2"
                seen.add(f"kind {s['kind']}")
                seen.add(f"{r4} skip {min(s['skip'], 3)}")
                seen.add(f"skip {min(s['skip'], 3)}")
                if s["kind"] == "X" and s["in_len"] < 1 << s["log_b"]:
                    seen.add("no whole row")
                if s["skip"] and s["skip"] == s["log_r"]:
                    seen.add("every stage skipped")
                left = s["log_r"] - s["skip"]
                if s["r4"]:
                    seen.add("r4 even" if left % 2 == 0 else "r4 odd")
                    if s["skip"] and left % 2:
                        seen.add("r4 odd after a skip")
                    if s["skip"] and left % 2 == 0:
                        seen.add("r4 even after a skip")
                elif s["want_r4"] and left == 1:
                    seen.add("r4 wanted, one stage left")
                seen.add("log_t 0" if s["log_t"] == 0 else "log_t > 0")
                if s["log_t_by_b"]:
                    seen.add("log_t limited by log_b")
                if s["log_t_by_lds"]:
                    seen.add("log_t limited by the LDS")
                work = s["E"] // (4 if s["r4"] else 2)
                if s["threads"] > s["E"] // 2:
                    seen.add("threads > E/2")
                if s["threads"] < s["E"] // 4:
                    seen.add("threads < E/4")
                if s["threads"] % 64:
                    seen.add("threads no multiple of 64")
                if s["threads"] < work and work % s["threads"]:
                    seen.add("sweeps with a ragged last round")
                if s["big_by_batch"] and not s["big_by_size"]:
                    seen.add("big by batch_min")
                if s["big_by_size"] and not s["big_by_batch"]:
                    seen.add("big by big_log")
                if cfg["big_tile_log"] == 0 and (s["grid_y"] >= cfg["batch_min"] or t["log_n"] >= cfg["big_log"]):
                    seen.add("big switched off")
                if s["fold29"]:
                    seen.add("fold29 with post3" if s["post3"] else "fold29 without post3")
                if s["post3"] and not s["fold29"]:
                    seen.add("post3 without fold29")
                if s["pre3"]:
                    seen.add("pre3")
                if s["pre_tab"]:
                    seen.add("pre_tab")
                if s["kind"] == "X" and s["sig"][1]:
                    seen.add("transposing store with sig_hi")
    want = {"npass 1", "npass 2", "npass 3", "kind X", "kind Y", "skip 0", "skip 1", "skip 2", "skip 3", "r2 skip 1", "r2 skip 2", "r2 skip 3",
            "r4 skip 1", "r4 skip 2", "r4 skip 3", "no whole row", "every stage skipped", "r4 even", "r4 odd", "r4 odd after a skip",
            "r4 even after a skip", "r4 wanted, one stage left", "log_t 0", "log_t > 0", "log_t limited by log_b", "log_t limited by the LDS",
            "threads > E/2", "threads < E/4", "threads no multiple of 64", "sweeps with a ragged last round", "big by batch_min",
            "big by big_log", "big switched off", "scale in the twiddle table", "scale as post3", "fold29 with post3",
            "fold29 without post3", "post3 without fold29", "pre3", "pre_tab", "transposing store with sig_hi",
            "more than NTT_BATCH_MAX vectors"}
    assert want <= seen, sorted(want - seen)
