"""The NTT engine's host decisions restated in Python (csrc/ntt_plan.h: the pass factorisation, the geometry of every pass, the
stages a zero-padded first pass leaves out, the workgroup of every launch), and the list of (configuration, shape) cases that
tests/test_gpu_ntt_plans.py runs against the oracle.  tests/test_ntt_cases_cpu.py compares the restatement with the engine's
own rules (tests/cpp/ntt_plan_check.cpp) and asserts that the case list reaches every variant of a pass -- without a GPU.

Parameters carry their public names and values here ("ntt.radix4": 0 by size, 1 always, 2 never)."""
import functools

LDS_BUDGET = 160 * 1024
BATCH_MAX = 32
MAX_PASS_LOG = 11
BATCHED_MAX_LOG = 18          # several transforms of one size share their launches up to 2^18 points; above, one after the other
NO_LIMIT = 0x7FFFFFFF

DEFAULTS = {"ntt.max_single_log": 11, "ntt.max_multi_log": 9, "ntt.tile_log": 9, "ntt.threads": 256, "ntt.big_tile_log": 10,
            "ntt.big_threads": 512, "ntt.batch_min": 4, "ntt.big_log": 20, "ntt.radix4": 0, "ntt.coset_scale_pass": 0}
# (lowest, highest) accepted value; ntt.big_tile_log also takes 0
RANGES = {"ntt.max_single_log": (1, MAX_PASS_LOG), "ntt.max_multi_log": (4, MAX_PASS_LOG), "ntt.tile_log": (6, 12), "ntt.threads": (64, 1024),
          "ntt.big_tile_log": (6, 12), "ntt.big_threads": (64, 1024), "ntt.batch_min": (1, NO_LIMIT), "ntt.big_log": (1, NO_LIMIT),
          "ntt.radix4": (0, 2), "ntt.coset_scale_pass": (0, 1)}
PARENT_RANGES = dict(RANGES, **{"ntt.max_single_log": (1, 12), "ntt.max_multi_log": (4, 12)})   # what the table took before


def boundary_points(name, ranges=RANGES):
    """lowest, one step inside, default, one step inside, highest (and the 0 of ntt.big_tile_log)"""
    lo, hi = ranges[name]
    pts = {lo, min(lo + 1, hi), DEFAULTS[name], max(hi - 1, lo), hi}
    if name == "ntt.big_tile_log":
        pts.add(0)
    return sorted(pts)


def config(params):
    """public parameters -> the fields of NttConfig (radix4 counts the other way round there: 0 never, 1 by size, 2 always)"""
    p = dict(DEFAULTS)
    for name, value in params.items():
        assert name in DEFAULTS, name
        p[name] = value
    cfg = {k[4:]: v for k, v in p.items() if k != "ntt.coset_scale_pass"}
    cfg["radix4"] = {0: 1, 1: 2, 2: 0}[p["ntt.radix4"]]
    return cfg


def check_args(params):
    """the name=value words of one line of ntt_plan_check for these public parameters"""
    cfg, dflt = config(params), config({})
    return " ".join(f"{k}={v}" for k, v in cfg.items() if v != dflt[k])


def factor(max_single, max_multi, log_n):
    if log_n <= max_single:
        return 1, (log_n, 0, 0)
    if log_n <= 2 * max_multi:
        l1 = (log_n + 1) // 2
        return 2, (l1, log_n - l1, 0)
    l1 = (log_n + 2) // 3
    l2 = (log_n - l1 + 1) // 2
    return 3, (l1, l2, log_n - l1 - l2)


def pass_geoms(npass, l):
    """the passes in launch order: kind, log_r, log_b, sig_lo, sig_hi, fold29, tw_pass (-1: no inter-pass twiddle on the store)"""
    l1, l2, l3 = l
    if npass == 1:
        return [dict(kind="Y", log_r=l1, log_b=0, sig=(0, 0), fold29=0, tw_pass=-1)]
    if npass == 2:
        return [dict(kind="X", log_r=l2, log_b=l1, sig=(l1, 0), fold29=0, tw_pass=0),
                dict(kind="Y", log_r=l1, log_b=l2, sig=(0, 0), fold29=1, tw_pass=-1)]
    return [dict(kind="X", log_r=l3, log_b=l1 + l2, sig=(l1, l2), fold29=0, tw_pass=0),
            dict(kind="Y", log_r=l2, log_b=l3, sig=(0, 0), fold29=0, tw_pass=1),
            dict(kind="Y", log_r=l1, log_b=l2 + l3, sig=(0, 0), fold29=1, tw_pass=-1)]


def skippable_stages(kind, log_r, log_b, in_len, log_n):
    if kind != "X" or in_len == 0 or in_len & (in_len - 1) or in_len >= 1 << log_n:
        return 0
    rows = in_len >> log_b
    if rows == 0 or rows >= 1 << log_r:
        return 0
    return log_r - (rows - 1).bit_length()


def lds_bytes(log_r, log_t):
    return ((1 << (log_r + log_t)) + (1 << log_r) // 2 + 8) * 36 + 64


@functools.lru_cache(maxsize=None)
def pass_shape(tile_log, max_threads, want_r4, kind, log_r, log_b, log_n, in_len, fit_lds=True):
    """the workgroup of one launch, once the shape (tile_log, max_threads) that applies is known"""
    skip = skippable_stages(kind, log_r, log_b, in_len, log_n)
    log_e = max(min(tile_log, log_n), log_r)
    wanted = log_e - log_r
    log_t = min(wanted, log_b)
    by_b, before = log_t < wanted, log_t
    while fit_lds and log_t and lds_bytes(log_r, log_t) > LDS_BUDGET:
        log_t -= 1
    E = 1 << (log_r + log_t)
    r4 = 1 if want_r4 and log_r - skip >= 2 else 0
    threads = min(min(max_threads, 512 if r4 else 1024), max(64, E // (4 if r4 else 2)))
    return dict(skip=skip, log_t=log_t, log_t_by_b=by_b, log_t_by_lds=log_t < before, E=E, r4=r4, threads=threads, grid_x=1 << (log_n - log_r - log_t),
                lds=lds_bytes(log_r, log_t))


def plan(params, log_n, in_len=None, nbatch=0, scale=False, pre3=False, post3=False, pre_tab=False, fit_lds=True):
    """what the engine launches for one transform (nbatch = 0) or one batched launch chain of `nbatch` vectors"""
    cfg = config(params)
    n = 1 << log_n
    in_len = n if in_len is None else min(in_len, n)
    npass, l = factor(cfg["max_single_log"], cfg["max_multi_log"], log_n)
    in_table = bool(scale) and not post3 and npass > 1
    by_batch, by_size = nbatch >= cfg["batch_min"], log_n >= cfg["big_log"]
    big = (by_batch or by_size) and cfg["big_tile_log"] != 0
    tile_log, max_threads = (cfg["big_tile_log"], cfg["big_threads"]) if big else (cfg["tile_log"], cfg["threads"])
    want_r4 = cfg["radix4"] == 2 or (cfg["radix4"] == 1 and big)
    passes = []
    for i, g in enumerate(pass_geoms(npass, l)):
        first, last = i == 0, i == npass - 1
        s = pass_shape(tile_log, max_threads, want_r4, g["kind"], g["log_r"], g["log_b"], log_n, in_len if first else n, fit_lds)
        passes.append(dict(g, **s, big=big, big_by_batch=big and by_batch, big_by_size=big and by_size, want_r4=want_r4,
                           in_len=in_len if first else n, grid_y=nbatch or 1, pre3=bool(first and pre3), pre_tab=bool(first and pre_tab),
                           post3=bool(last and (post3 or (scale and not in_table)))))
    # batched: a call with several vectors of this size goes through the batched launches; scratch: an in-place call needs a scratch vector
    return dict(npass=npass, l=l, scale_in_table=in_table, batched=1 <= log_n <= BATCHED_MAX_LOG, scratch=npass > 1, passes=passes)


def plan_line(p):
    """the plan as tests/cpp/ntt_plan_check.cpp prints it"""
    out = (f"npass={p['npass']} l={p['l'][0]},{p['l'][1]},{p['l'][2]} scale_in_table={int(p['scale_in_table'])} batched={int(p['batched'])} "
           f"scratch={int(p['scratch'])}")
    for s in p["passes"]:
        out += (f" | kind={s['kind']} log_r={s['log_r']} log_b={s['log_b']} sig={s['sig'][0]},{s['sig'][1]} skip={s['skip']} big={int(s['big'])} "
                f"log_t={s['log_t']} E={s['E']} r4={s['r4']} threads={s['threads']} grid={s['grid_x']},{s['grid_y']} lds={s['lds']} "
                f"pre3={int(s['pre3'])} pre_tab={int(s['pre_tab'])} post3={int(s['post3'])} fold29={s['fold29']} tw_pass={s['tw_pass']}")
    return out


def limits_broken(p, log_n):
    """the limits every launch must keep; returns what a plan breaks (empty: nothing)"""
    bad = []
    if sum(p["l"]) != log_n or len([x for x in p["l"] if x]) != p["npass"]:
        bad.append("lengths")
    for s in p["passes"]:
        if s["lds"] > LDS_BUDGET:
            bad.append(f"lds {s['lds']}")
        if s["threads"] > (512 if s["r4"] else 1024):
            bad.append(f"threads {s['threads']}")
        if s["log_r"] < 1:
            bad.append("log_r")
    return bad


# ----------------------------------------------------------------------------- the cases of tests/test_gpu_ntt_plans.py
# An operation of the library as the plan sees it: (log_n of the transform, in_len, scale, pre3, post3, pre_tab) from the case's k;
# `count` vectors go through batched launches of at most BATCH_MAX.
def transforms_of(case):
    """the (plan arguments) of every launch chain a case runs: list of dicts for `plan`"""
    op, k, params = case["op"], case["k"], case["params"]
    d, count = case.get("ext", 0), case.get("count", 0)
    chunks = [min(BATCH_MAX, count - f) for f in range(0, count, BATCH_MAX)]
    if op in ("fft_dev", "fft_host", "fft_root"):
        return [dict(log_n=k)]
    if op in ("intt_dev", "l2c_dev"):
        return [dict(log_n=k, scale=True)]
    if op in ("batch", "batch_oop"):
        return [dict(log_n=k, nbatch=c, scale=case.get("divisor", False)) for c in chunks]
    if op == "c2e":
        return [dict(log_n=k + d, in_len=1 << k, pre3=True)]
    if op == "c2e_batch":
        return [dict(log_n=k + d, in_len=1 << k, pre3=True, nbatch=c) for c in chunks]
    if op == "e2c":            # the round trip: coeff_to_extended, then extended_to_coeff
        return [dict(log_n=k + d, in_len=1 << k, pre3=True), dict(log_n=k + d, post3=True)]
    if op == "cosets":         # `count` columns on COSETS cosets each
        blocks = count * COSETS
        chunks = [min(BATCH_MAX, blocks - f) for f in range(0, blocks, BATCH_MAX)]
        tab = not dict(DEFAULTS, **params)["ntt.coset_scale_pass"]
        return [dict(log_n=k, nbatch=c, pre_tab=tab) for c in chunks]
    raise AssertionError(op)


NARROWED_K = BATCHED_MAX_LOG + 1
COSETS, COSET_EXT = 5, 3       # EvaluationDomain(6, k): five cosets of an extended domain of 2^(k + 3) rows


def _p(**kw):
    return {"ntt." + k: v for k, v in kw.items()}


def _case(op, k, params, **kw):
    name = f"{op}-k{k}" + "".join(f"-{a}{b}" for a, b in kw.items()) + "".join(f"-{a[4:]}={b}" for a, b in params.items())
    return dict(name=name, op=op, k=k, params=params, **kw)


def gpu_cases():
    """some 160 (configuration, shape) cases, log_n <= 14: see tests/test_ntt_cases_cpu.py for what they must reach"""
    c = []
    # --- the plan cuts, under each kernel (radix4: 2 never, 1 always): 1, 2 and 3 passes at small sizes; odd and even pass lengths
    cuts = [_p(max_single_log=1, max_multi_log=4), _p(max_single_log=4, max_multi_log=4), _p(max_single_log=4, max_multi_log=6), {}]
    for r4 in (2, 1):
        for cut in cuts:
            for k in (1, 2, 5, 9, 12)[r4 == 1:]:
                c.append(_case("fft_dev", k, dict(cut, **{"ntt.radix4": r4})))
        c.append(_case("fft_dev", 14, dict(cuts[0], **{"ntt.radix4": r4})))
        c.append(_case("fft_dev", 13, dict(cuts[2], **{"ntt.radix4": r4})))
    # --- the longest single pass the table accepts (one step further it was 2^12 points in 221,536 bytes of LDS)
    for r4 in (2, 1):
        c.append(_case("fft_dev", 11, _p(max_single_log=MAX_PASS_LOG, radix4=r4)))
        c.append(_case("fft_dev", 11, _p(max_single_log=MAX_PASS_LOG, tile_log=12, threads=1024, radix4=r4)))
    c.append(_case("l2c_dev", 11, _p(max_single_log=MAX_PASS_LOG)))
    # ... and the one size above the others: a pass of 2^10 points under tile_log = 12 exists from 2^19 points on only; its
    # 2^12-element tile (166,240 bytes) does not fit the LDS and is narrowed
    c.append(_case("fft_dev", NARROWED_K, _p(max_multi_log=10, tile_log=12, threads=1024, big_tile_log=0)))
    # --- tile and thread shapes (big shape switched off): wide tiles, many / few / odd thread counts
    for tile in (6, 9, 12):
        for thr in (64, 192, 1024):
            for k, cut in ((12, {}), (10, _p(max_single_log=4, max_multi_log=6)))[:1 + (thr != 192)]:
                c.append(_case("fft_dev", k, dict(cut, **_p(tile_log=tile, threads=thr, big_tile_log=0))))
    c.append(_case("fft_dev", 14, _p(max_single_log=4, max_multi_log=10, tile_log=12, threads=1024, big_tile_log=0)))
    c.append(_case("fft_dev", 12, _p(tile_log=12, threads=100, big_tile_log=0, radix4=1)))
    c.append(_case("fft_dev", 9, _p(max_single_log=4, max_multi_log=4, tile_log=8, threads=100, big_tile_log=0, radix4=2)))
    # --- the throughput shape: chosen by the batch, by the size, switched off; its tile and threads
    for btile in (0, 6, 12):
        for bthr in (64, 320, 1024):
            c.append(_case("batch", 10, _p(max_single_log=4, max_multi_log=6, big_tile_log=btile, big_threads=bthr, batch_min=1), count=3))
            if bthr != 320:
                c.append(_case("fft_dev", 12, _p(max_single_log=4, max_multi_log=4, big_tile_log=btile, big_threads=bthr, big_log=8)))
    c.append(_case("batch", 9, _p(batch_min=4), count=3))                   # below batch_min: the small shape
    c.append(_case("batch", 9, _p(batch_min=4), count=5))
    c.append(_case("fft_dev", 8, _p(big_log=8, max_single_log=4)))
    c.append(_case("fft_dev", 7, _p(big_log=8, max_single_log=4)))
    c.append(_case("fft_dev", 9, _p(big_log=1, batch_min=1, max_single_log=1, max_multi_log=4)))
    # --- entry points: host pointer, inverse with divisor (scale on the store of one pass / in the twiddle table of several)
    for cut in (cuts[0], cuts[2], {}):
        c.append(_case("fft_host", 9, cut))
        c.append(_case("fft_root", 9, cut))
        c.append(_case("intt_dev", 10, cut))
        c.append(_case("l2c_dev", 9, cut))
    c.append(_case("intt_dev", 4, _p(max_single_log=4, max_multi_log=4)))
    # --- batches in place and out of place, 1, 3, 5 and 33 vectors
    for op in ("batch", "batch_oop"):
        for count in (1, 3, 5, 33):
            c.append(_case(op, 7, cuts[1], count=count, divisor=count != 3))
            if count in (3, 33):
                c.append(_case(op, 10, cuts[0], count=count, divisor=count == 3))
        c.append(_case(op, 11, {}, count=5, divisor=True))
        c.append(_case(op, 12, {}, count=5, divisor=True))
    # --- the zero-padded first pass: ext_k - k of 1, 2 and 3 under each plan and each kernel
    for ext in (1, 2, 3):
        for cut in (cuts[1], cuts[2], cuts[0], {}):
            for r4 in (2, 1) if cut in cuts[1:3] else (1 + (ext + (not cut)) % 2,):
                c.append(_case("c2e", 9 - ext if cut else 12 - ext, dict(cut, **{"ntt.radix4": r4}), ext=ext))
        c.append(_case("c2e", 3, cuts[1], ext=ext))                        # every stage skipped
        c.append(_case("c2e", 2, dict(cuts[1], **{"ntt.radix4": 1}), ext=ext))   # no whole row (ext = 3): the general zero-fill load
        c.append(_case("c2e_batch", 6, cuts[1], ext=ext, count=5))
        c.append(_case("c2e_batch", 7, dict(cuts[0], **{"ntt.radix4": 1}), ext=ext, count=3))
        c.append(_case("e2c", 7, cuts[2], ext=ext))
        c.append(_case("e2c", 6, dict(cuts[0], **{"ntt.radix4": 1}), ext=ext))
    c.append(_case("c2e_batch", 9, {}, ext=3, count=33))
    c.append(_case("e2c", 8, {}, ext=3))                                    # one pass: post3 without fold29
    c.append(_case("e2c", 9, {}, ext=3))
    # --- the cosets, shift on the load of the first pass (a table) or in a pass of its own
    for csp in (0, 1):
        for cut in (cuts[1], cuts[0], {}):
            c.append(_case("cosets", 8, dict(cut, **{"ntt.coset_scale_pass": csp}), count=2))
        c.append(_case("cosets", 10, _p(coset_scale_pass=csp, max_single_log=4, max_multi_log=6, radix4=1), count=7))
        c.append(_case("cosets", 12, _p(coset_scale_pass=csp), count=1))
    names = [x["name"] for x in c]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    return c
