"""CPU checks of tests/msm_cases.py, the builders behind the MSM GPU tests: the signed-digit recoding restated from
msm_digits / make_window_plan (csrc/msm_sort.cuh, csrc/msm_plan.h), the buckets with prescribed populations that test_gpu_msm_backends.py feeds
to the accumulation, the merge rounds and the reductions, and the expected points computed from dot products.  A case that
silently stopped producing L + 1 entries in its bucket fails here, without a GPU."""
import itertools
import os
import subprocess
from collections import Counter

import numpy as np
import pytest

import msm_cases as mc
from oracle import oracle as O

WIDTHS = (5, 6, 13, 16)
from msm_cases import EDGE_WIDTHS, POPULATIONS, edge_cases   # what test_gpu_msm_backends.py runs


def test_window_plan_and_recoding_round_trip():
    """the digits of a scalar, weighted by their windows' offsets, are the scalar; every digit is in its window's range;
    the vectorised recoding agrees with the scalar one"""
    rng = np.random.default_rng(5)
    for c in range(4, 17):
        width, off = mc.window_plan(c), mc.window_offsets(c)
        assert len(width) == (255 + c - 1) // c and sum(width) == 254 and width[-1] == c - 1 and max(width) == c
        vals = mc.signed_digit_specials(c) + [int.from_bytes(rng.bytes(32), "little") % mc.R for _ in range(40)] + [0, 1]
        for v in vals:
            d = mc.recode(v, c)
            assert sum(x << o for x, o in zip(d, off)) == v
            assert all(-(1 << (w - 1)) <= x < (1 << (w - 1)) for x, w in zip(d[:-1], width[:-1]))
            assert 0 <= d[-1] < 1 << width[-1]
        got = mc.digits_np(mc._ints(vals), c)
        assert got.shape == (len(width), len(vals))
        assert (got.T == np.array([mc.recode(v, c) for v in vals])).all()


@pytest.mark.parametrize("c", WIDTHS)
def test_place_puts_one_entry_where_it_says(c):
    """every spot the populations use, and the corners of the bucket range: exactly the intended entries and no others"""
    width = mc.window_plan(c)
    nbw, top = 1 << (c - 1), len(width) - 1
    spots = set(mc.population_spots(c, 2)) | {(0, nbw - 2, False), (0, nbw - 1, True), (1, 0, True), (top - 1, 0, True),
                                               (top, mc.max_top_digit(c) - 1, False)}
    for spot in spots:
        v, want = mc.place(c, *spot)
        assert 0 < v < mc.R
        assert mc.bucket_map([v], c) == want, spot
        assert want[spot] == 1 and sum(want.values()) == (2 if spot[2] else 1)
    with pytest.raises(AssertionError):
        mc.place(c, 0, nbw - 1, False)          # the last bucket takes the digit -2^(c-1) only
    with pytest.raises(AssertionError):
        mc.place(c, top, 0, True)               # the top window is unsigned


@pytest.mark.parametrize("c", WIDTHS)
@pytest.mark.parametrize("log_seg,fold,log_G,extra", POPULATIONS, ids=[f"seg{p[0]}-fold{p[1]}-G{p[2]}" for p in POPULATIONS])
def test_populations_are_what_they_say(c, log_seg, fold, log_G, extra):
    """the builder's scalars recode to exactly the intended (window, bucket, sign) -> count map, which holds every size of
    the list at least once; the counts the GPU test asserts (`tasks`, `max_bucket`) follow from it either way"""
    values, want = mc.populations(c, log_seg, fold, log_G, extra)
    assert mc.bucket_map(values, c) == want
    sizes = mc.population_sizes(log_seg, fold) + list(extra)
    L = 1 << log_seg
    assert {1, L - 1, L, L + 1, 2 * L, fold * L, fold * L + 1, L * L + 1} - {0} <= set(sizes)
    assert Counter(want.values()) & Counter(sizes) == Counter(sizes)     # every size is some bucket's exact population
    assert max(want.values()) == max(sizes)
    shuffled = mc.interleave(values, 7)
    assert sorted(shuffled) == sorted(values)
    canon = mc._ints(shuffled)
    for fixed in (False, True):
        cnt = mc.bucket_counts(canon, c, fixed)
        assert (cnt == mc.counts_from_map(want, c, fixed)).all()
        tasks, biggest = mc.tasks_and_max(cnt, log_seg)
        assert tasks == int(sum(-(-m // L) for m in mc.counts_from_map(want, c, fixed).ravel()))
        assert biggest >= max(sizes)
    # the spots: first, chunk boundary and last bucket of a window, and the top window
    G, nbw, top = 1 << log_G, 1 << (c - 1), len(mc.window_plan(c)) - 1
    used = {(w, b) for (w, b, _) in mc.population_spots(c, log_G)}
    assert {(0, 0), (0, G - 1), (0, G), (0, nbw - 1), (top, 0)} <= used and any(w == top and b > 0 for w, b in used)


@pytest.mark.parametrize("c", (5, 13))
def test_expected_points_match_the_oracle_msm(c):
    """the expected point of a prescribed-population case, <k, s> G from the dot product, is what the oracle's own MSM gives
    for the same scalars over bases s_i G (n <= 2^12)"""
    log_seg, fold, log_G, extra = POPULATIONS[0]
    values, _ = mc.populations(c, log_seg, fold, log_G, extra)
    values = mc.interleave(values, c)[:1 << 12]
    n = len(values)
    k = O.fr_to_mont(mc._ints(values))
    s = O.random_fr(0xC0 + c, n)
    bases = O.fixed_base_mul(s, O.ncpu())
    want = O.g1_mul(O.g1_generator(), O.fr_dot(k, s))
    assert want.any() and (want == O.best_multiexp(k, bases, O.ncpu())).all()


@pytest.mark.parametrize("c", EDGE_WIDTHS)
def test_group_law_edges_match_the_oracle_msm(c):
    """every group-law edge case of the GPU file: its expected point from the dot product equals the oracle's MSM over the
    same bases (identity points among them), and is not the identity; its buckets are what the case is named for"""
    G = O.g1_generator()
    for name, values, logs in edge_cases(c):
        n = len(values)
        assert n <= 1 << 12, name
        k = O.fr_to_mont(mc._ints(values))
        s = O.fr_to_mont(mc._ints(logs))
        bases = O.fixed_base_mul(s, O.ncpu())
        assert all((bases[64 * i:64 * i + 64] == 0).all() == (logs[i] == 0) for i in range(n))
        want = O.g1_mul(G, O.fr_dot(k, s))
        assert want.any(), name
        assert (want == O.best_multiexp(k, bases, O.ncpu())).all(), name
        m = mc.bucket_map(values, c)
        nbw = 1 << (c - 1)
        if name == "same_point":
            assert all(m[(0, b, b == nbw - 1)] == 1 for b in range(nbw))
        if name == "only_first":
            assert {b for (_, b, _) in m} == {0}
        if name == "only_last":
            assert {(w, b) for (w, b, _) in m} == {(0, nbw - 1), (1, 0)}
        if name == "one_window":
            assert {w for (w, _, _) in m} == {3}


def test_expected_backend_is_the_issue_table():
    """the restated decision rules at the places the table of defaults names: the headline MSM takes the scan path with 16
    level-0 workgroups per window (never msm_reduce_items<1>), a single commitment the folded 2-D path, and the forced roads"""
    e = mc.expected_backend(1 << 20, 1, False, 16, {}, 1)
    assert e["kernels"] == ["msm_accumulate", "msm_reduce_buckets<1>", "msm_reduce_items<4>", "msm_export_windows"]
    assert (e["log_G"], e["threads"], e["blocks"], e["T1"], e["quad"], e["red2d"]) == (3, 256, 16, 16, False, 0)
    e = mc.expected_backend(1 << 20, 1, False, 16, {}, 2)
    assert e["kernels"][1] == "msm_reduce_buckets_lean<1>" and e["log_G"] == 4
    e = mc.expected_backend(1 << 17, 1, True, 16, {}, 1, max_bucket=200)
    assert e["kernels"] == ["msm_accumulate", "msm_merge<4>", "msm_fold_buckets<4>", "msm_reduce2d_lines_folded<4>",
                            "msm_reduce2d_bits<4>", "msm_export_points"] and e["per_win"] == 16 and e["log_seg"] == 4
    e = mc.expected_backend(1 << 17, 7, True, 16, {}, 1)
    assert e["red2d"] == 0 and e["kernels"][1] == "msm_reduce_buckets<4>"      # 7 x 2^15 buckets: still quad-cooperative
    e = mc.expected_backend(1 << 12, 1, False, 16, {"msm.red2d": 0, "msm.quad": 0, "msm.red_threads": 64, "msm.log_red_chunk": 1}, 1)
    assert (e["blocks"], e["T1"]) == (256, 256) and "msm_reduce_items<1>" in e["kernels"]
    e = mc.expected_backend(1 << 12, 1, False, 16, {"msm.red2d": 0, "msm.quad": 2, "msm.log_red_chunk": 1}, 1)
    assert e["log_G"] == 3 and e["blocks"] == 64                         # raised by the loop: 2^14 chunks > 64 x 64
    e = mc.expected_backend(1 << 12, 1, False, 5, {"msm.red2d": 0, "msm.log_red_chunk": 8}, 1)
    assert e["log_G"] == 4 and e["blocks"] == 1 and e["T1"] is None      # clamped to c - 1
    e = mc.expected_backend(1 << 15, 1, False, 13, {"msm.red2d": 2, "msm.red2d_prefold": 0, "msm.quad": 0}, 1)
    assert e["kernels"][1:] == ["msm_reduce2d_lines<1>", "msm_reduce2d_bits<1>", "msm_reduce2d_combine", "msm_export_points"]
    assert mc.expected_backend(1 << 12, 1, True, 4, {"msm.red2d": 2}, 1)["red2d"] == 0
    # merge rounds: 700 entries in tasks of 4 are four rounds, three when the 2-D line sums take 8 partial sums per bucket
    assert mc.expected_backend(1 << 12, 1, False, 13, {"msm.red2d": 0, "msm.log_seg": 2}, 1, max_bucket=700)["merge_rounds"] == 4
    assert mc.expected_backend(1 << 12, 1, False, 13, {"msm.red2d": 2, "msm.log_seg": 2}, 1, max_bucket=700)["merge_rounds"] == 3
    for fold in (1, 8, 256):
        p = {"msm.red2d": 2, "msm.log_seg": 2, "msm.red2d_fold": fold}
        assert mc.expected_backend(1 << 12, 1, False, 13, p, 1, max_bucket=4 * fold)["merge_rounds"] == 0
        assert mc.expected_backend(1 << 12, 1, False, 13, p, 1, max_bucket=4 * fold + 1)["merge_rounds"] == 1
    # the grid rule: 128 threads x three waves per SIMD on 256 CUs, two when another job is in flight, tasks when waves = 8
    assert mc.accumulate_threads(1 << 20, 1, False, 16, {}, 1, 256) == 256 * 768
    assert mc.accumulate_threads(1 << 20, 1, False, 16, {}, 2, 256) == 256 * 512
    ub = 16 * (1 << 15) + (16 << 20 >> 7)
    assert mc.accumulate_threads(1 << 20, 1, False, 16, {"msm.acc_waves": 8, "msm.acc_threads": 64}, 1, 256) == (ub + 63) // 64 * 64


def test_backend_defaults_are_the_documented_ones():
    from param_doc import documented_defaults
    doc = documented_defaults()
    assert {f"msm.{k}": v for k, v in mc.BACKEND_DEFAULTS.items()} == {f"msm.{k}": doc[f"msm.{k}"] for k in mc.BACKEND_DEFAULTS}


# ----------------------------------------------------------------------------- the restated rules against the real ones
def _plan_param_sets():
    """the msm.* settings the GPU back-end tests run under (test_gpu_msm_backends.py: SCAN_PATHS, DEVICE_2D, HOST_2D, _GRID and
    the forced shapes of the scan reduction, the task length, the merge rounds and the fold), without the "msm." prefix"""
    scan = [{"red2d": 0, "quad": 0, "red_lean": 0}, {"red2d": 0, "quad": 2}, {"red2d": 0, "quad": 0, "red_lean": 2}]
    dev2d = [{"red2d": 2, "red2d_prefold": pf, "quad": q} for pf in (1, 0) for q in (0, 2)]
    host2d = [{"red2d": 1, "red2d_prefold": pf, "quad": q} for pf in (1, 0) for q in (0, 2)]
    sets = [{}] + scan + dev2d + host2d
    sets += [{"red2d": 0, "quad": 0, "red_threads": 64}, {"red2d": 0, "quad": 0, "red_threads": 64, "log_red_chunk": 1},
             {"red2d": 0, "log_red_chunk": 1}, {"red2d": 0, "log_red_chunk": 8}, {"red2d": 0, "quad": 2, "log_red_chunk": 1}]
    sets += [{"log_seg": 2}, {"log_seg": 2, "merge_quad_tasks": 0}, {"merge_quad_tasks": 0}]
    sets += [{"acc_threads": at, "acc_waves": w} for at in (64, 128, 256) for w in (1, 2, 3, 7, 8)]
    sets += [{"acc_waves_fixed": 2}, {"acc_waves_fixed": 3}]
    sets += [{"red2d": 2, "log_seg": 2, "red2d_fold": 1}, {"red2d": 2, "log_seg": 2, "red2d_fold": 8}, {"red2d_fold": 1}]
    return sets


def _fmt(v):
    return "-" if v is None else str(int(v))


def _restated(n, M, fixed, c, params, jobs, largest, tasks):
    """everything but the grid of one line of msm_plan_check, from the restatement in msm_cases.py; None: not a valid job"""
    p = {f"msm.{k}": v for k, v in params.items()}
    cc = c if fixed else mc.generic_window_bits(n, M > 1, {**p, **({"msm.window_bits": c} if c else {})})
    try:
        e = mc.expected_backend(n, M, fixed, cc, p, jobs, max_bucket=largest, tasks=tasks or None)
    except AssertionError:
        return None
    width = mc.window_plan(cc)
    W1, sets = len(width), (1 if fixed else len(width)) * M
    log_seg = params.get("log_seg") or mc.auto_log_seg(W1 * M * n, sets << (cc - 1))
    assert (e["c"], e["windows"], e["sets"], e["log_seg"]) == (cc, W1, sets, log_seg)
    return cc, (f"c={cc} windows={W1} widths={','.join(map(str, width))} sets={sets} log_seg={log_seg} quad={int(e['quad'])} "
                f"red2d={e['red2d']} fold={e['fold']} log_G={_fmt(e['log_G'])} threads={_fmt(e['threads'])} blocks={_fmt(e['blocks'])} "
                f"T1={_fmt(e['T1'])} merge_rounds={e['merge_rounds']} per_win={e['per_win']} kernels={','.join(e['kernels'])}")


def test_restated_rules_are_the_engines_own(tmp_path):
    """tests/cpp/msm_plan_check.cpp runs the engine's planning (csrc/msm_plan.h, no HIP) on every job of a grid; `expected_backend`,
    `accumulate_threads`, `auto_log_seg`, `generic_window_bits` and `window_plan` must say the same, field by field: the
    GPU tests name the kernel a case exercises on the strength of these restatements.  A job the engine rejects (more than
    2^21 buckets: generic jobs of 6, 7 or 9 MSMs at c = 16) must be one the restatement rejects, and the other way round; at
    least 95 % of the grid are valid jobs.  The C++ rules are the reference: a difference is fixed in msm_cases.py."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "msm_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(root, "circuits_halo2_amd", "csrc"),
                           os.path.join(root, "tests", "cpp", "msm_plan_check.cpp"), "-o", exe])
    shapes = [(n, M, fixed, c) for n in (1 << 10, 1 << 12, 1 << 15, 1 << 17, 1 << 20) for M in (1, 4, 6, 7, 9)
              for fixed in (False, True) for c in (0, 4, 5, 6, 10, 11, 12, 13, 16) if c or not fixed]
    cases = [(n, M, fixed, c, params, jobs, cus, largest, 0)
             for (n, M, fixed, c), params, jobs in itertools.product(shapes, _plan_param_sets(), (1, 2))
             for cus in (256, 64) for largest in (1, 33, 700, 70000)]
    # the job's exact task count, which msm.merge_quad_tasks is compared with (the grid above leaves it at the upper bound)
    cases += [(1 << 12, 1, False, 13, {"red2d": 0, "log_seg": 2, "merge_quad_tasks": mqt}, 1, 256, 700, tasks)
              for mqt in (0, 1000, 1001, 0x7fffffff) for tasks in (900, 1300, 4000)]
    text = "".join(f"{n} {M} {int(fixed)} {c} {jobs} {cus} {largest} {tasks} " + " ".join(f"{k}={v}" for k, v in params.items()) + "\n"
                   for n, M, fixed, c, params, jobs, cus, largest, tasks in cases)
    got = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split("\n")[:-1]
    assert len(got) == len(cases)
    backend, grid = {}, {}
    valid = 0
    for line, (n, M, fixed, c, params, jobs, cus, largest, tasks) in zip(got, cases):
        pk = tuple(params.items())
        key = (n, M, fixed, c, pk, jobs, largest, tasks)
        if key not in backend:
            backend[key] = _restated(n, M, fixed, c, params, jobs, largest, tasks)
        if backend[key] is None:
            assert line == "invalid", (key, line)
            continue
        cc, want = backend[key]
        gkey = (n, M, fixed, cc, pk, jobs, cus)
        if gkey not in grid:
            grid[gkey] = mc.accumulate_threads(n, M, fixed, cc, {f"msm.{k}": v for k, v in params.items()}, jobs, cus)
        want = f"{want} acc_threads={grid[gkey]}"
        if line != want:
            diff = [(a, b) for a, b in zip(line.split(" "), want.split(" ")) if a != b]
            raise AssertionError(f"n={n} M={M} fixed={fixed} c={c} {params} jobs={jobs} cus={cus} largest={largest} tasks={tasks}: "
                                 f"engine / restatement {diff or (line, want)}")
        valid += 1
    assert valid >= 0.95 * len(cases), (valid, len(cases))
