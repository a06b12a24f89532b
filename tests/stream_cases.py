"""The stream-order table: one row per entry point of include/summa_gpu.h that takes a `void* stream` (no GPU, no HIP here).

The header promises that every `_dev` entry point is ordered on the stream it is given: work enqueued earlier on that stream is
seen by the call, work enqueued afterwards sees the call's results, with no host wait in between.  tests/test_gpu_stream_order.py
holds every row to that promise (a delayed producer in front of the call, a trailer behind it); tests/test_stream_cases_cpu.py
checks, without a GPU, that the table covers the header and that every row could fail.

A row builds a Case:
  ins        device input buffers: name -> (real words, decoy words of the same shape)
  host_ins   host buffers the entry reads before it returns (pageable memory: the header's promise for sg_mst_entries_dev and
             sg_mst_update_dev): name -> (real, decoy); the test overwrites them with the decoy as soon as the call is back
  outs       device output buffers: name -> bytes (pre-filled with 0x5A)
  inout      names of `ins` the call overwrites with a result (in-place transforms, the running numerator, a tree)
  opaque     device work buffers whose contents the header does not define: name -> bytes (never compared)
  call       call(b, h, ctx) issues the entry on torch's current stream: through the Python wrapper where the wrapper lets the
             caller own the output buffers (the wrappers pass ffi.current_stream_ptr()), through ffi.lib() where the wrapper
             allocates its outputs itself (a fresh allocation cannot be pre-filled) or where there is no wrapper; it returns the
             host result (bytes as a numpy array) of an entry that has one
  ref        ref(inputs) -> {output name or "host": expected words}, from oracle.oracle, oracle.pyref or the reference functions
             of the existing case modules only -- never from another library path
  aux        outputs that say only "done" (a status word, a problem word): compared, but equal for real and decoy by nature
  fixed      output name -> rows that the operation's definition makes independent of the inputs (z[0] = 1, the zero behind a
             quotient's last coefficient): equal for real and decoy by nature, still never 0x5A
  blocks     output name -> a number of equal blocks (a user's column of the witness): where the floor plan fixes most cells, every
             block must still hold a row in which real and decoy differ
  params     library parameters (sg_set_param) the call runs under, so that a small shape reaches the path in question
  setup      setup() -> ctx: resident state that is not a caller's buffer (an SRS handle, a program in device memory), made and
             complete before the first wait of a test; cleanup(ctx) gives it back after the last one

Shapes are the smallest that still take the path in question (n = 2^10 / k = 10, the extended domain of 2^12 rows; the batched
NTT once at 2^12 -- batched launches on the caller's stream -- and once at 2^19, the first size that runs on the two batch
streams, three vectors so that the halves of the lane's scratch are reused).  `cold`: the same row at a k that no other row
uses, so that plans, twiddles, domain constants and coset tables are made by that very call.
"""
import collections
import ctypes as C
import functools
import re

import numpy as np

FILL = 0x5A
K = 10
N = 1 << K
EXT = 2                       # extended domain of 2^(K + EXT) rows
K_COLD = 7                    # no row uses 2^7 or its extended domain 2^9
BATCH_LOGS = {"caller": 12, "batch streams": 19}      # sg_ntt_fr_batch*: batched on the caller's stream / on the batch streams
BATCH_COLD = {"caller": 14, "batch streams": 20}
BATCH_VECTORS = 3
MSM_JOB_LENGTHS = [N, N, N // 2, N, N // 2]
COMMIT_JOBS = 5
EXEMPT = {
    "sg_stream_wait": "a host wait and nothing else: it produces neither a device nor a host result",
    "sg_time_ntt_dev": "takes no stream (it times launches on the library's own) and returns a duration, not a result",
}

Row = collections.namedtuple("Row", "name entry via build caches per_stream")
ROWS = []


def row(name, entry, via, caches=None, per_stream=False):
    """register a row; caches: what the entry keeps between calls (the row is then also run cold, then warm on a second stream);
    per_stream: the entry's work space is the stream's (the row is then also run on two streams call by call)"""
    def deco(fn):
        ROWS.append(Row(name, entry, via, fn, caches, per_stream))
        return fn
    return deco


class Case:
    def __init__(self, call, ref, ins=None, outs=None, inout=(), aux=(), fixed=None, host_ins=None, opaque=None, setup=None,
                 cleanup=None, blocks=None, params=None, note=""):
        self.call, self.ref = call, ref
        self.ins, self.outs, self.inout, self.aux = dict(ins or {}), dict(outs or {}), tuple(inout), tuple(aux)
        self.fixed, self.host_ins, self.opaque = dict(fixed or {}), dict(host_ins or {}), dict(opaque or {})
        self.setup, self.cleanup = setup or (lambda: None), cleanup or (lambda ctx: None)
        self.blocks, self.params, self.note = dict(blocks or {}), dict(params or {}), note
        self._want = {}

    def inputs(self, which):
        i = 0 if which == "real" else 1
        d = {name: pair[i] for name, pair in self.ins.items()}
        d.update({name: pair[i] for name, pair in self.host_ins.items()})
        return d

    def want(self, which="real"):
        """the oracle's result for the real (or the decoy) inputs, computed once"""
        if which not in self._want:
            w = {k: np.ascontiguousarray(v, dtype=np.uint8).reshape(-1) for k, v in self.ref(self.inputs(which)).items()}
            for a in w.values():
                a.setflags(write=False)
            self._want[which] = w
        return self._want[which]

    def output_names(self):
        return list(self.outs) + list(self.inout)


def rows_of(words):
    """32-byte rows; a result that is no multiple of 32 bytes (a counter, a flag, a row count) is one row"""
    words = np.ascontiguousarray(words, dtype=np.uint8).reshape(-1)
    return words.reshape(-1, 32) if words.size % 32 == 0 and words.size else words.reshape(1, -1)


@functools.lru_cache(maxsize=None)
def built(name, seed=0, cold=False):
    """the case of a row, built once and shared (read only)"""
    from oracle import oracle as O
    return by_name(name).build(O, seed, cold)


def by_name(name):
    return next(r for r in ROWS if r.name == name)


def header_stream_entries(text):
    """names of the prototypes of a C header that have a `void* stream` parameter"""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = re.findall(r"\b(?:int|void)\s+(s[gpv]_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S)
    return [name for name, args in protos if re.search(r"void\s*\*\s*stream\b", args)]


MAX_FUSED = 64                      # csrc/msm_plan.h: MSMs in one fused job
LOG_FUSE_GENERIC, LOG_FUSE_FIXED = 25, 27       # include/summa_gpu.h, "msm.log_fuse_entries": the built-in sizes of each kind
COMMIT_PARAMS = {"msm.log_fuse_entries": 16}    # the commit rows' columns of 2^10: one (generic) or two (fixed-base) to a fused job


def max_fused(n, log_fuse=LOG_FUSE_GENERIC):
    """csrc/msm_plan.h, max_fused: how many same-length MSMs a generic fused job takes"""
    import msm_cases
    c = msm_cases.generic_window_bits(n, True)
    W = -(-255 // c)
    return max(1, min((1 << 21) // (W << (c - 1)), (1 << log_fuse) // max(1, W * n), MAX_FUSED))


def max_fused_fixed(table_n, n, log_fuse=LOG_FUSE_FIXED):
    """csrc/msm_plan.h, max_fused_fixed, over the window table sg_srs_precompute builds by default for table_n points"""
    import g1_cases
    c = g1_cases.default_window_bits(table_n)
    W = -(-255 // c)
    return max(1, min((1 << 21) >> (c - 1), (1 << log_fuse) // max(1, W * n), MAX_FUSED))


def fused_groups(lengths, limit=max_fused):
    """csrc/commit_plan.h, fused_groups: consecutive MSMs of equal length are one fused job, at most limit(length) of them"""
    groups, i = [], 0
    while i < len(lengths):
        g = 1
        while i + g < len(lengths) and lengths[i + g] == lengths[i] and g < limit(lengths[i]):
            g += 1
        groups.append((i, g))
        i += g
    return groups


def row_groups(name):
    """the fused jobs a batch row runs as: (lengths, fixed-base?, groups) under the row's parameters"""
    case = built(name)
    log_fuse = case.params.get("msm.log_fuse_entries", 0)
    if name == "msm_g1_batch":
        return MSM_JOB_LENGTHS, False, fused_groups(MSM_JOB_LENGTHS, lambda n: max_fused(n, log_fuse or LOG_FUSE_GENERIC))
    fixed = name in FIXED_BASE_ROWS
    limit = (lambda n: max_fused_fixed(N, n, log_fuse or LOG_FUSE_FIXED)) if fixed else (lambda n: max_fused(n, log_fuse or LOG_FUSE_GENERIC))
    return [N] * COMMIT_JOBS, fixed, fused_groups([N] * COMMIT_JOBS, limit)


BATCH_ROWS = ("msm_g1_batch", "commit_batch", "commit_batch_mixed")
FIXED_BASE_ROWS = ("commit_batch",)       # rows whose SRS has its window table (sg_srs_precompute): the prover's path


# ----------------------------------------------------------------------------- helpers of the rows
def _ffi():
    from circuits_halo2_amd import ffi
    return ffi, ffi.lib()


def _A():
    from circuits_halo2_amd import arithmetic
    return arithmetic


def _p(t):
    return C.c_void_p(t.data_ptr())


def _arr(ts):
    return (C.c_void_p * max(1, len(ts)))(*[t.data_ptr() for t in ts])


def _stream():
    return _ffi()[0].current_stream_ptr()


def _check(rc):
    _ffi()[0].check(rc)


def _hp(a):
    return a.ctypes.data_as(C.c_void_p)


def _pair(O, seed, n, tag=0):
    """(real, decoy): n random field elements each, from seeds no other buffer of the module shares.  The seeds differ in their
    high bits: oracle.random_fr replaces a rejected candidate i from the stream of seed ^ (i + 1), so two seeds that differ in
    their low bits only can share elements"""
    base = ((seed + 1) << 44) | (tag << 36) | 0x5eed
    return O.random_fr(base, n), O.random_fr(base | (1 << 60), n)


def _cols(O, seed, names, n):
    return {name: _pair(O, seed, n, 10 + i) for i, name in enumerate(names)}


def _word(O, seed, tag):
    """one random field element: a host argument (a point, a challenge), the same for real and decoy"""
    return O.random_fr(900001 * (seed + 1) + tag, 1)


def _fr(values):
    from oracle import pyref as P
    return np.frombuffer(P.frs_to_bytes(values), dtype=np.uint8).copy()


def _ints(words):
    raw = bytes(np.ascontiguousarray(words, dtype=np.uint8))
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


def _raw(values):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), dtype=np.uint8).copy()


def _cat(parts):
    return np.concatenate([np.ascontiguousarray(p, dtype=np.uint8).reshape(-1) for p in parts])


@functools.lru_cache(maxsize=None)
def _bases(seed, n):
    """n points s_i G, s_i random: bases of an MSM (any points of the group serve)"""
    from oracle import oracle as O
    b = O.fixed_base_mul(O.random_fr(777000 + (seed << 24), n), O.ncpu() if n > 4096 else 1)
    b.setflags(write=False)
    return b


def _kk(cold):
    return K_COLD if cold else K


# ============================================================================= MSM and commitments
def _msm_case(O, seed, timed):
    def call(b, h, ctx):
        from circuits_halo2_amd import arithmetic as A
        out = A.best_multiexp(b["scalars"], b["bases"], timings=timed)
        return out[0] if timed else out
    ins = {"scalars": _pair(O, seed, N), "bases": (_bases(2 * seed, N), _bases(2 * seed + 1, N))}
    return Case(call, lambda i: {"host": O.best_multiexp(i["scalars"], i["bases"])}, ins=ins)


@row("msm_g1", "sg_msm_g1_dev", "arithmetic.best_multiexp", caches="the MSM engines' work space")
def _(O, seed, cold):
    return _msm_case(O, seed, False)


@row("msm_g1_timed", "sg_msm_g1_dev_timed", "arithmetic.best_multiexp(timings=True)")
def _(O, seed, cold):
    return _msm_case(O, seed, True)


@row("msm_g1_batch", "sg_msm_g1_batch_dev", "arithmetic.best_multiexp_batch", caches="the MSM engines' work space")
def _(O, seed, cold):
    ins = {}
    for j, n in enumerate(MSM_JOB_LENGTHS):
        ins[f"scalars{j}"] = _pair(O, seed, n, 20 + j)
        ins[f"bases{j}"] = (_bases(10 + 2 * j, N)[:64 * n], _bases(11 + 2 * j, N)[:64 * n])

    def call(b, h, ctx):
        from circuits_halo2_amd import arithmetic as A
        return _cat(A.best_multiexp_batch([(b[f"scalars{j}"], b[f"bases{j}"]) for j in range(len(MSM_JOB_LENGTHS))]))
    ref = lambda i: {"host": _cat([O.best_multiexp(i[f"scalars{j}"], np.ascontiguousarray(i[f"bases{j}"])) for j in range(len(MSM_JOB_LENGTHS))])}
    return Case(call, ref, ins=ins)


def _srs(k=K, precompute=None):
    """a resident SRS of 2^k points per basis (any points serve: a commitment is an MSM against them)"""
    from circuits_halo2_amd.params import ParamsKZG
    p = ParamsKZG(k, _bases(40, 1 << k), _bases(41, 1 << k))
    p.handle()
    if precompute is not None:
        p.precompute(precompute)
    return p


def _srs_fixed():
    """the same with the window table of g: commitments against it take the fixed-base path"""
    return _srs(K, 0)


def _commit_ref(O, names, bases):
    g = {0: _bases(40, N), 1: _bases(41, N)}
    return lambda i: {"host": _cat([O.best_multiexp(i[name], g[b]) for name, b in zip(names, bases)])}


def _commit_one(O, seed, timed):
    def call(b, h, ctx):
        ffi, L = _ffi()
        out = np.zeros(64, dtype=np.uint8)
        if timed:
            tm = ffi.MsmTimings()
            _check(L.sg_commit_dev_timed(C.c_uint64(ctx.handle()), C.c_int(1), _p(b["scalars"]), C.c_size_t(N), _stream(), _hp(out), C.byref(tm)))
            return out
        return ctx.commit_lagrange(b["scalars"])
    return Case(call, _commit_ref(O, ["scalars"], [1]), ins={"scalars": _pair(O, seed, N)}, setup=_srs, cleanup=lambda p: p.free())


@row("commit", "sg_commit_dev", "ParamsKZG.commit_lagrange", caches="the MSM engines' work space")
def _(O, seed, cold):
    return _commit_one(O, seed, False)


@row("commit_timed", "sg_commit_dev_timed", "ffi.lib()")
def _(O, seed, cold):
    return _commit_one(O, seed, True)


@row("commit_batch", "sg_commit_batch_dev", "ParamsKZG.commit_batch", caches="the MSM engines' work space")
def _(O, seed, cold):
    names = [f"poly{j}" for j in range(COMMIT_JOBS)]
    call = lambda b, h, ctx: ctx.commit_batch([b[n] for n in names]).reshape(-1)
    return Case(call, _commit_ref(O, names, [0] * COMMIT_JOBS), ins=_cols(O, seed, names, N), setup=_srs_fixed, cleanup=lambda p: p.free(),
                params=COMMIT_PARAMS,
                note="the entry takes one length for all its columns; five columns of 2^10 over g's window table, two to a fused job under "
                     "msm.log_fuse_entries = 16: three jobs, both engines, the finish of a third group")


MIXED_BASES = [0, 1, 1, 0, 1]


def mixed_case(O, seed):
    names = [f"poly{j}" for j in range(COMMIT_JOBS)]
    call = lambda b, h, ctx: ctx.commit_batch_mixed([b[n] for n in names], MIXED_BASES).reshape(-1)
    return Case(call, _commit_ref(O, names, MIXED_BASES), ins=_cols(O, seed, names, N), setup=_srs, cleanup=lambda p: p.free(), params=COMMIT_PARAMS,
                note="no window tables: the generic fused path, one column to a job under msm.log_fuse_entries = 16, five jobs")


@row("commit_batch_mixed", "sg_commit_batch_mixed_dev", "ParamsKZG.commit_batch_mixed", caches="the MSM engines' work space")
def _(O, seed, cold):
    return mixed_case(O, seed)


@row("srs_upload", "sg_srs_upload_dev", "ParamsKZG.from_device")
def _(O, seed, cold):
    """the entry returns a handle once its copies are complete; what it holds is read back through commitments of host scalars
    (sg_commit: a host-pointer call that waits) and compared with the oracle's MSM of the same scalars over the real bases"""
    s = O.random_fr(4242 + seed, N)

    def call(b, h, ctx):
        from circuits_halo2_amd.params import ParamsKZG
        p = ParamsKZG.from_device(K, b["g"], b["g_lagrange"])
        ctx.append(p)
        return _cat([p._commit(0, s), p._commit(1, s)])
    ins = {"g": (_bases(50 + 2 * seed, N), _bases(51 + 2 * seed, N)), "g_lagrange": (_bases(60 + 2 * seed, N), _bases(61 + 2 * seed, N))}
    ref = lambda i: {"host": _cat([O.best_multiexp(s, np.ascontiguousarray(i["g"])), O.best_multiexp(s, np.ascontiguousarray(i["g_lagrange"]))])}

    def cleanup(ctx):
        ffi, L = _ffi()
        for p in ctx:
            _check(L.sg_srs_free(C.c_uint64(p._handle)))
    return Case(call, ref, ins=ins, setup=list, cleanup=cleanup)


@row("srs_copy", "sg_srs_copy_dev", "ffi.lib()")
def _(O, seed, cold):
    """no caller's buffer goes in (the bases are resident): the row holds the outputs to the stream's order"""
    def call(b, h, ctx):
        _check(_ffi()[1].sg_srs_copy_dev(C.c_uint64(ctx.handle()), _p(b["g"]), _p(b["g_lagrange"]), _stream()))
    return Case(call, lambda i: {"g": _bases(40, N), "g_lagrange": _bases(41, N)}, outs={"g": 64 * N, "g_lagrange": 64 * N}, setup=_srs,
                cleanup=lambda p: p.free())


# ============================================================================= transforms
@row("ntt", "sg_ntt_fr_dev", "arithmetic.best_fft", caches="NTT plan, twiddles, scratch slot", per_stream=True)
def _(O, seed, cold):
    k = _kk(cold)
    call = lambda b, h, ctx: _A().best_fft(b["a"], O.omega(k), k)
    return Case(call, lambda i: {"a": O.best_fft(i["a"], O.omega(k), k)}, ins={"a": _pair(O, seed, 1 << k)}, inout=["a"])


@row("intt", "sg_intt_fr_dev", "ffi.lib()", caches="NTT plan, twiddles, scratch slot")
def _(O, seed, cold):
    k = _kk(cold)
    w, d = O.omega_inv(k), O.n_inv(k)
    call = lambda b, h, ctx: _check(_ffi()[1].sg_intt_fr_dev(_p(b["a"]), _hp(w), _hp(d), C.c_uint32(k), _stream()))
    return Case(call, lambda i: {"a": O.ifft(i["a"], w, d, k)}, ins={"a": _pair(O, seed, 1 << k)}, inout=["a"])


def _domain(k):
    from circuits_halo2_amd.domain import EvaluationDomain
    dom = EvaluationDomain((1 << EXT) + 1, k)
    assert dom.extended_k == k + EXT
    return dom


@row("lagrange_to_coeff", "sg_lagrange_to_coeff_dev", "EvaluationDomain.lagrange_to_coeff", caches="domain constants, NTT plan, twiddles")
def _(O, seed, cold):
    k = _kk(cold)
    call = lambda b, h, ctx: _domain(k).lagrange_to_coeff(b["a"])
    return Case(call, lambda i: {"a": O.lagrange_to_coeff(i["a"], k)}, ins={"a": _pair(O, seed, 1 << k)}, inout=["a"])


def _batch(O, seed, cold, where, oop):
    log_n = (BATCH_COLD if cold else BATCH_LOGS)[where]
    names = [f"a{j}" for j in range(BATCH_VECTORS)]
    w, th = O.omega(log_n), O.ncpu()
    ins = {name: _pair(O, seed, 1 << log_n, 30 + j) for j, name in enumerate(names)}
    if oop:
        def call(b, h, ctx):
            _check(_ffi()[1].sg_ntt_fr_batch_oop_dev(_arr([b[n] for n in names]), _arr([b["out_" + n] for n in names]), C.c_size_t(len(names)),
                                                     _hp(w), None, C.c_uint32(log_n), _stream()))
        return Case(call, lambda i: {"out_" + n: O.best_fft(i[n], w, log_n, th) for n in names}, ins=ins,
                    outs={"out_" + n: 32 << log_n for n in names})
    call = lambda b, h, ctx: _A().best_fft_batch([b[n] for n in names], w, log_n)
    return Case(call, lambda i: {n: O.best_fft(i[n], w, log_n, th) for n in names}, ins=ins, inout=names)


@row("ntt_batch_on_the_callers_stream", "sg_ntt_fr_batch_dev", "arithmetic.best_fft_batch", caches="batched NTT plan, twiddles, scratch slot 3",
     per_stream=True)
def _(O, seed, cold):
    return _batch(O, seed, cold, "caller", False)


@row("ntt_batch_on_the_batch_streams", "sg_ntt_fr_batch_dev", "arithmetic.best_fft_batch", caches="NTT plan, twiddles, the lane's scratch")
def _(O, seed, cold):
    return _batch(O, seed, cold, "batch streams", False)


@row("ntt_batch_oop_on_the_callers_stream", "sg_ntt_fr_batch_oop_dev", "ffi.lib()", caches="batched NTT plan, twiddles", per_stream=True)
def _(O, seed, cold):
    return _batch(O, seed, cold, "caller", True)


@row("ntt_batch_oop_on_the_batch_streams", "sg_ntt_fr_batch_oop_dev", "ffi.lib()", caches="NTT plan, twiddles, the lane's scratch")
def _(O, seed, cold):
    return _batch(O, seed, cold, "batch streams", True)


@row("coeff_to_extended", "sg_coeff_to_extended_dev", "ffi.lib()", caches="domain constants, NTT plan, twiddles")
def _(O, seed, cold):
    k = _kk(cold)
    call = lambda b, h, ctx: _check(_ffi()[1].sg_coeff_to_extended_dev(_p(b["c"]), C.c_uint32(k), C.c_uint32(k + EXT), _p(b["out"]), _stream()))
    return Case(call, lambda i: {"out": O.coeff_to_extended(i["c"], k, k + EXT)}, ins={"c": _pair(O, seed, 1 << k)}, outs={"out": 32 << (k + EXT)})


@row("coeff_to_extended_batch", "sg_coeff_to_extended_batch_dev", "ffi.lib()", caches="domain constants, batched NTT plan, twiddles")
def _(O, seed, cold):
    k = _kk(cold)
    names = ["c0", "c1", "c2"]

    def call(b, h, ctx):
        _check(_ffi()[1].sg_coeff_to_extended_batch_dev(_arr([b[n] for n in names]), _arr([b["out_" + n] for n in names]), C.c_size_t(3), C.c_uint32(k),
                                                        C.c_uint32(k + EXT), _stream()))
    return Case(call, lambda i: {"out_" + n: O.coeff_to_extended(i[n], k, k + EXT) for n in names}, ins=_cols(O, seed, names, 1 << k),
                outs={"out_" + n: 32 << (k + EXT) for n in names})


@row("extended_to_coeff", "sg_extended_to_coeff_dev", "EvaluationDomain.extended_to_coeff", caches="domain constants, NTT plan, twiddles")
def _(O, seed, cold):
    k = _kk(cold)
    call = lambda b, h, ctx: _domain(k).extended_to_coeff(b["a"])
    return Case(call, lambda i: {"a": O.extended_to_coeff(i["a"], k, k + EXT)}, ins={"a": _pair(O, seed, 1 << (k + EXT))}, inout=["a"])


@row("divide_by_vanishing_poly", "sg_divide_by_vanishing_poly_dev", "EvaluationDomain.divide_by_vanishing_poly", caches="domain constants, t_evals")
def _(O, seed, cold):
    k = _kk(cold)
    call = lambda b, h, ctx: _domain(k).divide_by_vanishing_poly(b["a"])
    return Case(call, lambda i: {"a": O.divide_by_vanishing_poly(i["a"], k, k + EXT)}, ins={"a": _pair(O, seed, 1 << (k + EXT))}, inout=["a"])


N_COSETS = 3


@row("coeff_to_cosets_batch", "sg_coeff_to_cosets_batch_dev", "ffi.lib()", caches="domain constants, coset tables, batched NTT plan")
def _(O, seed, cold):
    import coset_cases as cc
    k = _kk(cold)
    names = ["c0", "c1"]

    def call(b, h, ctx):
        _check(_ffi()[1].sg_coeff_to_cosets_batch_dev(_arr([b[n] for n in names]), _arr([b["out_" + n] for n in names]), C.c_size_t(2), C.c_uint32(k),
                                                      C.c_uint32(k + EXT), C.c_uint32(N_COSETS), _stream()))
    ref = lambda i: {"out_" + n: cc.gather(O.coeff_to_extended(i[n], k, k + EXT), k, EXT, N_COSETS) for n in names}
    return Case(call, ref, ins=_cols(O, seed, names, 1 << k), outs={"out_" + n: (32 * N_COSETS) << k for n in names})


@row("cosets_to_pieces", "sg_cosets_to_pieces_dev", "ffi.lib()", caches="domain constants, coset tables, batched NTT plan")
def _(O, seed, cold):
    import coset_cases as cc
    k = _kk(cold)
    names = [f"piece{t}" for t in range(N_COSETS)]

    def call(b, h, ctx):
        _check(_ffi()[1].sg_cosets_to_pieces_dev(_p(b["values"]), _arr([b[n] for n in names]), C.c_uint32(k), C.c_uint32(k + EXT), C.c_uint32(N_COSETS),
                                                 _stream()))
    ref = lambda i: dict(zip(names, cc.ref_cosets_to_pieces(i["values"], k, EXT, N_COSETS)))
    return Case(call, ref, ins={"values": _pair(O, seed, N_COSETS << k)}, outs={n: 32 << k for n in names},
                note="the values are destroyed: what the call leaves in them is not defined and not compared")


# ============================================================================= G1 set-up operations
@row("g1_fixed_base_mul", "sg_g1_fixed_base_mul_dev", "ffi.lib()")
def _(O, seed, cold):
    call = lambda b, h, ctx: _check(_ffi()[1].sg_g1_fixed_base_mul_dev(_p(b["s"]), C.c_size_t(N), _p(b["out"]), _stream()))
    return Case(call, lambda i: {"out": O.fixed_base_mul(i["s"])}, ins={"s": _pair(O, seed, N)}, outs={"out": 64 * N})


@row("kzg_setup", "sg_kzg_setup_dev", "ffi.lib()", caches="domain constants")
def _(O, seed, cold):
    """tau is a host argument: no caller's buffer goes in, the row holds the outputs to the stream's order"""
    import g1_cases as gc
    k = _kk(cold)
    tau = _word(O, seed, 1)
    call = lambda b, h, ctx: _check(_ffi()[1].sg_kzg_setup_dev(C.c_uint32(k), _hp(tau), _p(b["g"]), _p(b["g_lagrange"]), _stream()))

    def ref(i):
        t = _ints(O.fr_from_mont(tau))[0]
        return {"g": O.fixed_base_mul(O.fr_powers(tau, 1 << k)), "g_lagrange": O.fixed_base_mul(gc.mont(gc.lagrange_at(t, k)))}
    return Case(call, ref, outs={"g": 64 << k, "g_lagrange": 64 << k})


@row("g1_fft", "sg_g1_fft_dev", "ffi.lib()")
def _(O, seed, cold):
    k = 8          # g1_cases.FFT_LOGS' largest: two blocks of 128 butterflies
    w = O.omega(k)
    s = _pair(O, seed, 1 << k)
    call = lambda b, h, ctx: _check(_ffi()[1].sg_g1_fft_dev(_p(b["in"]), _p(b["out"]), _hp(w), None, C.c_uint32(k), _stream()))
    pts = tuple(O.fixed_base_mul(x) for x in s)
    want = {bytes(p): O.fixed_base_mul(O.best_fft(x, w, k)) for p, x in zip(pts, s)}
    return Case(call, lambda i: {"out": want[bytes(i["in"])]}, ins={"in": pts}, outs={"out": 64 << k},
                note="in[i] = s_i G, so out = (best_fft of s) G by the oracle")


# ============================================================================= element-wise and scan helpers
@row("fr_to_montgomery", "sg_fr_to_montgomery_dev", "ffi.lib()")
def _(O, seed, cold):
    call = lambda b, h, ctx: _check(_ffi()[1].sg_fr_to_montgomery_dev(_p(b["in"]), _p(b["out"]), C.c_size_t(N), _stream()))
    ins = {"in": tuple(O.fr_from_mont(a) for a in _pair(O, seed, N))}
    return Case(call, lambda i: {"out": O.fr_to_mont(i["in"])}, ins=ins, outs={"out": 32 * N})


@row("fr_from_montgomery", "sg_fr_from_montgomery_dev", "ffi.lib()")
def _(O, seed, cold):
    call = lambda b, h, ctx: _check(_ffi()[1].sg_fr_from_montgomery_dev(_p(b["in"]), _p(b["out"]), C.c_size_t(N), _stream()))
    return Case(call, lambda i: {"out": O.fr_from_mont(i["in"])}, ins={"in": _pair(O, seed, N)}, outs={"out": 32 * N})


def _permute_case(O, seed, kind, entry, rows=N):
    """sg_lookup_permute*: the columns go in as Montgomery words; A' and S' come back as Montgomery words"""
    import lookup_permute_cases as lp
    cases = []
    for which in (0, 1):
        rng = np.random.default_rng(1000 * seed + 11 + which)
        if kind == "range":             # a range table of 8-bit values: even ones for real, odd ones for the decoy
            pool = [2 * v + which for v in range(128)]
        else:                           # full-width values, each column's own
            pool = [int.from_bytes(rng.bytes(32), "little") % lp.R for _ in range(300)]
        table = [pool[i % len(pool)] for i in range(rows)]
        rng.shuffle(table)
        inp = [table[j] for j in rng.integers(0, rows, rows)]
        cases.append((lp.to_limbs(inp), lp.to_limbs(table), tuple(lp.to_limbs(c) for c in lp.expected(inp, table))))
    mont = lambda limbs: O.fr_to_mont(np.ascontiguousarray(limbs).view(np.uint8).reshape(-1).copy())
    ins = {"input": tuple(mont(c[0]) for c in cases), "table": tuple(mont(c[1]) for c in cases)}
    want = {bytes(mont(c[0])): {"permuted_input": mont(c[2][0]), "permuted_table": mont(c[2][1])} for c in cases}
    is_async = "async" in entry

    def call(b, h, ctx):
        fn = getattr(_ffi()[1], entry)
        args = [_p(b["input"]), _p(b["table"]), C.c_size_t(rows), _p(b["permuted_input"]), _p(b["permuted_table"])]
        _check(fn(*args, _p(b["status"]), _stream()) if is_async else fn(*args, _stream()))

    def ref(i):
        w = dict(want[bytes(i["input"])])
        if is_async:
            w["status"] = np.zeros(4, dtype=np.uint8)
        return w
    outs = {"permuted_input": 32 * rows, "permuted_table": 32 * rows}
    if is_async:
        outs["status"] = 4
    return Case(call, ref, ins=ins, outs=outs, aux=["status"] if is_async else [],
                note="expected: lookup_permute_cases.expected (Python integers) as Montgomery words")


@row("lookup_permute_small", "sg_lookup_permute_small_dev", "ffi.lib()", caches="lookup work space", per_stream=True)
def _(O, seed, cold):
    return _permute_case(O, seed, "range", "sg_lookup_permute_small_dev")


@row("lookup_permute_small_async", "sg_lookup_permute_small_async_dev", "ffi.lib()", caches="lookup work space", per_stream=True)
def _(O, seed, cold):
    return _permute_case(O, seed, "range", "sg_lookup_permute_small_async_dev")


@row("lookup_permute", "sg_lookup_permute_dev", "ffi.lib()", caches="lookup work space", per_stream=True)
def _(O, seed, cold):
    return _permute_case(O, seed, "wide", "sg_lookup_permute_dev")


@row("lookup_permute_async", "sg_lookup_permute_async_dev", "ffi.lib()", caches="lookup work space", per_stream=True)
def _(O, seed, cold):
    return _permute_case(O, seed, "wide", "sg_lookup_permute_async_dev")


def _random_key(seed):
    return np.frombuffer(bytes((seed * 31 + 7 * i + 1) % 256 for i in range(32)), dtype=np.uint8).copy()


@row("fr_random", "sg_fr_random_dev", "ffi.lib()")
def _(O, seed, cold):
    """the key is a host argument: no caller's buffer goes in, the row holds the output to the stream's order"""
    from oracle import pyref as P
    key, n = _random_key(seed), 300
    call = lambda b, h, ctx: _check(_ffi()[1].sg_fr_random_dev(_hp(key), C.c_uint64(9), _p(b["out"]), C.c_size_t(n), _stream()))
    return Case(call, lambda i: {"out": _raw(P.chacha_field_elements(bytes(key), 9, n))}, outs={"out": 32 * n},
                note="300 elements: two blocks of 256 threads; the reference is Python's ChaCha20, a few hundred blocks of it")


@row("fr_random_batch", "sg_fr_random_batch_dev", "ffi.lib()")
def _(O, seed, cold):
    from oracle import pyref as P
    key, ns = _random_key(seed + 100), [257, 40]

    def call(b, h, ctx):
        _check(_ffi()[1].sg_fr_random_batch_dev(_hp(key), C.c_uint64(5), _arr([b["out0"], b["out1"]]), (C.c_size_t * 2)(*ns), C.c_uint32(2), _stream()))
    return Case(call, lambda i: {f"out{d}": _raw(P.chacha_field_elements(bytes(key), 5 + d, n)) for d, n in enumerate(ns)},
                outs={f"out{d}": 32 * n for d, n in enumerate(ns)})


@row("fr_eval_poly", "sg_fr_eval_poly_dev", "arithmetic.eval_polynomial")
def _(O, seed, cold):
    x = _word(O, seed, 2)
    call = lambda b, h, ctx: _A().eval_polynomial(b["poly"], x)
    return Case(call, lambda i: {"host": O.fr_eval_poly(i["poly"], x)}, ins={"poly": _pair(O, seed, N)})


@row("fr_eval_poly_batch", "sg_fr_eval_poly_batch_dev", "arithmetic.eval_polynomial_batch")
def _(O, seed, cold):
    names = ["p0", "p1", "p2"]
    pts = O.random_fr(31337 + seed, 3)
    call = lambda b, h, ctx: _A().eval_polynomial_batch([b[n] for n in names], pts).reshape(-1)
    ref = lambda i: {"host": _cat([O.fr_eval_poly(i[n], pts[32 * j:32 * j + 32].copy()) for j, n in enumerate(names)])}
    return Case(call, ref, ins=_cols(O, seed, names, N))


@row("fr_batch_invert", "sg_fr_batch_invert_dev", "arithmetic.batch_invert")
def _(O, seed, cold):
    call = lambda b, h, ctx: _A().batch_invert(b["a"])
    return Case(call, lambda i: {"a": O.fr_batch_invert(i["a"])}, ins={"a": _pair(O, seed, N)}, inout=["a"])


@row("fr_prefix_product", "sg_fr_prefix_product_dev", "ffi.lib()", caches="scratch slots")
def _(O, seed, cold):
    call = lambda b, h, ctx: _check(_ffi()[1].sg_fr_prefix_product_dev(_p(b["a"]), C.c_size_t(N), _p(b["out"]), _stream()))
    return Case(call, lambda i: {"out": O.fr_prefix_product(i["a"])}, ins={"a": _pair(O, seed, N)}, outs={"out": 32 * (N + 1)}, fixed={"out": [0]})


@row("permutation_product", "sg_permutation_product_dev", "ffi.lib()", caches="domain constants, local twiddles, scratch slots")
def _(O, seed, cold):
    beta, gamma, z0, one = _word(O, seed, 3), _word(O, seed, 4), _word(O, seed, 5), _fr([1])
    names = ["v0", "v1", "s0", "s1"]

    def call(b, h, ctx):
        _check(_ffi()[1].sg_permutation_product_dev(_arr([b["v0"], b["v1"]]), _arr([b["s0"], b["s1"]]), C.c_uint32(2), _hp(beta), _hp(gamma), _hp(one),
                                                    C.c_uint32(K), _hp(z0), _p(b["z"]), _stream()))
    ref = lambda i: {"z": O.permutation_product([i["v0"], i["v1"]], [i["s0"], i["s1"]], beta, gamma, one, K, z0)}
    return Case(call, ref, ins=_cols(O, seed, names, N), outs={"z": 32 * N}, fixed={"z": [0]})


LOOKUP_COLS = ["input", "table", "permuted_input", "permuted_table"]


@row("lookup_product", "sg_lookup_product_dev", "ffi.lib()", caches="scratch slots")
def _(O, seed, cold):
    beta, gamma = _word(O, seed, 6), _word(O, seed, 7)

    def call(b, h, ctx):
        _check(_ffi()[1].sg_lookup_product_dev(*[_p(b[n]) for n in LOOKUP_COLS], _hp(beta), _hp(gamma), C.c_size_t(N), _p(b["z"]), _stream()))
    ref = lambda i: {"z": O.lookup_product(*[i[n] for n in LOOKUP_COLS], beta, gamma)}
    return Case(call, ref, ins=_cols(O, seed, LOOKUP_COLS, N), outs={"z": 32 * N}, fixed={"z": [0]})


GRAND_CHUNKS = [2, 1]
GRAND_USABLE = N - 6


def _grand(O, seed, closing):
    from oracle import pyref as P
    beta, gamma = _word(O, seed, 8), _word(O, seed, 9)
    vals, sigs = [f"v{c}" for c in range(3)], [f"s{c}" for c in range(3)]
    names = vals + sigs + LOOKUP_COLS
    zs = ["z0", "z1", "z_lookup"]

    def call(b, h, ctx):
        L = _ffi()[1]
        head = [_arr([b[n] for n in vals]), _arr([b[n] for n in sigs]), (C.c_uint32 * 2)(*GRAND_CHUNKS), C.c_uint32(2), _arr([b[n] for n in LOOKUP_COLS]),
                C.c_uint32(1), _hp(beta), _hp(gamma), C.c_uint32(K), C.c_size_t(GRAND_USABLE), _arr([b[n] for n in zs])]
        _check(L.sg_grand_products_closing_dev(*head, _p(b["closing"]), _stream()) if closing else L.sg_grand_products_dev(*head, _stream()))

    def ref(i):
        at = lambda z: z[32 * GRAND_USABLE:32 * GRAND_USABLE + 32].copy()
        z0 = O.permutation_product([i["v0"], i["v1"]], [i["s0"], i["s1"]], beta, gamma, _fr([1]), K)
        z1 = O.permutation_product([i["v2"]], [i["s2"]], beta, gamma, _fr([pow(P.DELTA, 2, P.R)]), K, at(z0))
        zl = O.lookup_product(*[i[n] for n in LOOKUP_COLS], beta, gamma)
        w = {"z0": z0, "z1": z1, "z_lookup": zl}
        if closing:
            w["closing"] = _cat([at(z0), at(z1), at(zl)])
        return w
    outs = {n: 32 * N for n in zs}
    if closing:
        outs["closing"] = 96
    return Case(call, ref, ins=_cols(O, seed, names, N), outs=outs, fixed={"z0": [0], "z_lookup": [0]},
                note="the oracle's products chained by hand: chunk 1 starts from chunk 0's value at the last usable row")


@row("grand_products", "sg_grand_products_dev", "ffi.lib()", caches="domain constants, local twiddles, scratch slots")
def _(O, seed, cold):
    return _grand(O, seed, False)


@row("grand_products_closing", "sg_grand_products_closing_dev", "ffi.lib()", caches="domain constants, local twiddles, scratch slots")
def _(O, seed, cold):
    return _grand(O, seed, True)


@row("fr_mul", "sg_fr_mul_dev", "ffi.lib()")
def _(O, seed, cold):
    call = lambda b, h, ctx: _check(_ffi()[1].sg_fr_mul_dev(_p(b["a"]), _p(b["b"]), C.c_size_t(N), _p(b["out"]), _stream()))
    return Case(call, lambda i: {"out": O.fr_mul_n(i["a"], i["b"])}, ins=_cols(O, seed, ["a", "b"], N), outs={"out": 32 * N})


def _kate_want(O, a, b):
    q, rem = O.fr_kate_division(a, b)
    return np.concatenate([q, np.zeros(32, dtype=np.uint8)]), rem


@row("fr_kate_division", "sg_fr_kate_division_dev", "ffi.lib()", caches="scratch slots")
def _(O, seed, cold):
    pt = _word(O, seed, 10)

    def call(b, h, ctx):
        rem = np.zeros(32, dtype=np.uint8)
        _check(_ffi()[1].sg_fr_kate_division_dev(_p(b["a"]), C.c_size_t(N), _hp(pt), _p(b["q"]), _hp(rem), _stream()))
        return rem
    ref = lambda i: dict(zip(("q", "host"), _kate_want(O, i["a"], pt)))
    return Case(call, ref, ins={"a": _pair(O, seed, N)}, outs={"q": 32 * N}, fixed={"q": [N - 1]})


@row("fr_kate_division_batch", "sg_fr_kate_division_batch_dev", "ffi.lib()", caches="the ring of power tables", per_stream=True)
def _(O, seed, cold):
    """`points` is read before the call returns (the header): the test overwrites it as soon as the call is back"""
    names = ["a0", "a1", "a2"]
    pts = O.random_fr(5151 + seed, 3)

    def call(b, h, ctx):
        _check(_ffi()[1].sg_fr_kate_division_batch_dev(_arr([b[n] for n in names]), C.c_size_t(N), _hp(h["points"]), C.c_uint32(3),
                                                       _arr([b["q_" + n] for n in names]), _stream()))
    ref = lambda i: {"q_" + n: _kate_want(O, i[n], i["points"][32 * j:32 * j + 32].copy())[0] for j, n in enumerate(names)}
    return Case(call, ref, ins=_cols(O, seed, names, N), host_ins={"points": (pts, O.random_fr(6161 + seed, 3))},
                outs={"q_" + n: 32 * N for n in names}, fixed={"q_" + n: [N - 1] for n in names})


@row("fr_kate_division_rem", "sg_fr_kate_division_rem_dev", "ffi.lib()", caches="scratch slots")
def _(O, seed, cold):
    pt = _word(O, seed, 11)
    call = lambda b, h, ctx: _check(_ffi()[1].sg_fr_kate_division_rem_dev(_p(b["a"]), C.c_size_t(N), _hp(pt), _p(b["q"]), _p(b["rem"]), _stream()))
    ref = lambda i: dict(zip(("q", "rem"), _kate_want(O, i["a"], pt)))
    return Case(call, ref, ins={"a": _pair(O, seed, N)}, outs={"q": 32 * N, "rem": 32}, fixed={"q": [N - 1]})


def _noncanonical_cols(O, seed, counts):
    """two columns of canonical words with counts[which] words at or above r planted (poly_cases.NONCANONICAL)"""
    import poly_cases as pc
    out = {}
    for j, name in enumerate(("c0", "c1")):
        pair = [a.copy() for a in _pair(O, seed, N, 40 + j)]
        for which, a in enumerate(pair):
            for t in range(counts[which] if j == 0 else 1):
                r = (37 * t + 5 * which + j) % N
                a[32 * r:32 * r + 32] = _raw([pc.NONCANONICAL[t % 3]])
        out[name] = tuple(pair)
    return out


def _count(i):
    from oracle import pyref as P
    return sum(v >= P.R for name in ("c0", "c1") for v in _ints(i[name]))


@row("fr_count_noncanonical", "sg_fr_count_noncanonical_dev", "ffi.lib()", caches="scratch slots")
def _(O, seed, cold):
    def call(b, h, ctx):
        _check(_ffi()[1].sg_fr_count_noncanonical_dev(_arr([b["c0"], b["c1"]]), C.c_uint32(2), C.c_size_t(N), _p(b["count"]), _stream()))
    ref = lambda i: {"count": np.array([_count(i)], dtype=np.uint32).view(np.uint8)}
    return Case(call, ref, ins=_noncanonical_cols(O, seed, (5 + seed, 12 + seed)), outs={"count": 4}, note="expected: the words at or above r, counted as integers")


@row("fr_flag_noncanonical", "sg_fr_flag_noncanonical_dev", "ffi.lib()")
def _(O, seed, cold):
    """the real columns hold words at or above r (the flag becomes 1), the decoy's are canonical (the flag is left alone)"""
    def call(b, h, ctx):
        _check(_ffi()[1].sg_fr_flag_noncanonical_dev(_arr([b["c0"], b["c1"]]), C.c_uint32(2), C.c_size_t(N), _p(b["flag"]), _stream()))
    cols = _noncanonical_cols(O, seed, (5, 0))
    cols["c1"] = (cols["c1"][0], _pair(O, seed, N, 41)[1])
    ref = lambda i: {"flag": np.array([1], dtype=np.uint32).view(np.uint8) if _count(i) else np.full(4, FILL, dtype=np.uint8)}
    return Case(call, ref, ins=cols, outs={"flag": 4})


def _lincomb_want(O, i, names, coeffs, low):
    out = O.fr_lincomb([i[n] for n in names], coeffs)
    for r in range(low.size // 32):
        out[32 * r:32 * r + 32] = O.fr_add(out[32 * r:32 * r + 32].copy(), low[32 * r:32 * r + 32].copy())
    return out


@row("fr_lincomb", "sg_fr_lincomb_dev", "ffi.lib()")
def _(O, seed, cold):
    names, co = ["p0", "p1", "p2"], O.random_fr(7171 + seed, 3)
    call = lambda b, h, ctx: _check(_ffi()[1].sg_fr_lincomb_dev(_arr([b[n] for n in names]), _hp(co), C.c_uint32(3), C.c_size_t(N), _p(b["out"]), _stream()))
    return Case(call, lambda i: {"out": O.fr_lincomb([i[n] for n in names], co)}, ins=_cols(O, seed, names, N), outs={"out": 32 * N})


@row("fr_lincomb_low", "sg_fr_lincomb_low_dev", "ffi.lib()")
def _(O, seed, cold):
    names, co, low = ["p0", "p1"], O.random_fr(7272 + seed, 2), O.random_fr(7373 + seed, 3)

    def call(b, h, ctx):
        _check(_ffi()[1].sg_fr_lincomb_low_dev(_arr([b[n] for n in names]), _hp(co), C.c_uint32(2), C.c_size_t(N), _hp(low), C.c_uint32(3), _p(b["out"]),
                                               _stream()))
    return Case(call, lambda i: {"out": _lincomb_want(O, i, names, co, low)}, ins=_cols(O, seed, names, N), outs={"out": 32 * N})


@row("fr_lincomb_sets", "sg_fr_lincomb_sets_dev", "arithmetic.fr_lincomb_sets", caches="the blob ring", per_stream=True)
def _(O, seed, cold):
    sets = [(["p0", "p1", "p2"], O.random_fr(7474 + seed, 3), O.random_fr(7575 + seed, 2)), (["p3", "p1"], O.random_fr(7676 + seed, 2), O.random_fr(7777 + seed, 4))]
    names = ["p0", "p1", "p2", "p3"]

    def call(b, h, ctx):
        from circuits_halo2_amd import arithmetic as A
        A.fr_lincomb_sets([([b[n] for n in ns], co, low) for ns, co, low in sets], N, [b["out0"], b["out1"]])
    ref = lambda i: {f"out{s}": _lincomb_want(O, i, ns, co, low) for s, (ns, co, low) in enumerate(sets)}
    return Case(call, ref, ins=_cols(O, seed, names, N), outs={"out0": 32 * N, "out1": 32 * N})


# ============================================================================= the quotient's numerator
PERM_COLS, CHUNK_LEN, LAST_ROT = 3, 2, 6
SELECTORS = ["l0", "l_last", "l_active"]


def _perm_names():
    return ["values", "z0", "z1"] + [f"col{c}" for c in range(PERM_COLS)] + [f"sigma{c}" for c in range(PERM_COLS)] + SELECTORS


def _perm_ref(O, i, ch):
    return O.quotient_permutation(i["values"], [i["z0"], i["z1"]], [i[f"col{c}"] for c in range(PERM_COLS)], [i[f"sigma{c}"] for c in range(PERM_COLS)],
                                  CHUNK_LEN, i["l0"], i["l_last"], i["l_active"], *ch, K, K + EXT, LAST_ROT)


def _gathered(O, seed, names):
    """columns drawn on the extended domain (the oracle's layout); the device gets the coset-major gather of the first N_COSETS
    cosets of the same words: a rotation moves inside a residue class, so the other classes never mix with them"""
    import coset_cases as cc
    ext = _cols(O, seed, names, N << EXT)
    dev = {n: tuple(cc.gather(a, K, EXT, N_COSETS) for a in pair) for n, pair in ext.items()}
    back = {bytes(dev[names[0]][w]): {n: ext[n][w] for n in names} for w in (0, 1)}
    return dev, lambda i: back[bytes(i[names[0]])]


@row("quotient_permutation", "sg_quotient_permutation_dev", "arithmetic.quotient_permutation", caches="domain constants, local twiddles")
def _(O, seed, cold):
    ch = [_word(O, seed, 12 + j) for j in range(3)]

    def call(b, h, ctx):
        from circuits_halo2_amd import arithmetic as A
        A.quotient_permutation(b["values"], [b["z0"], b["z1"]], [b[f"col{c}"] for c in range(PERM_COLS)], [b[f"sigma{c}"] for c in range(PERM_COLS)],
                               CHUNK_LEN, b["l0"], b["l_last"], b["l_active"], *ch, K, K + EXT, LAST_ROT)
    return Case(call, lambda i: {"values": _perm_ref(O, i, ch)}, ins=_cols(O, seed, _perm_names(), N << EXT), inout=["values"])


@row("quotient_permutation_cosets", "sg_quotient_permutation_cosets_dev", "arithmetic.quotient_permutation_cosets", caches="domain constants, local twiddles, coset tables")
def _(O, seed, cold):
    import coset_cases as cc
    ch = [_word(O, seed, 15 + j) for j in range(3)]
    dev, ext_of = _gathered(O, seed, _perm_names())

    def call(b, h, ctx):
        from circuits_halo2_amd import arithmetic as A
        A.quotient_permutation_cosets(b["values"], [b["z0"], b["z1"]], [b[f"col{c}"] for c in range(PERM_COLS)], [b[f"sigma{c}"] for c in range(PERM_COLS)],
                                      CHUNK_LEN, b["l0"], b["l_last"], b["l_active"], *ch, K, K + EXT, N_COSETS, LAST_ROT)
    return Case(call, lambda i: {"values": cc.gather(_perm_ref(O, ext_of(i), ch), K, EXT, N_COSETS)}, ins=dev, inout=["values"])


LOOKUP_ARGS = ["values", "z", "permuted_input", "permuted_table", "input", "table"] + SELECTORS


def _lookup_ref(O, i, ch):
    return O.quotient_lookup(*[i[n] for n in LOOKUP_ARGS], *ch, K, K + EXT)


@row("quotient_lookup", "sg_quotient_lookup_dev", "arithmetic.quotient_lookup")
def _(O, seed, cold):
    ch = [_word(O, seed, 18 + j) for j in range(3)]
    call = lambda b, h, ctx: _A().quotient_lookup(*[b[n] for n in LOOKUP_ARGS], *ch, K, K + EXT)
    return Case(call, lambda i: {"values": _lookup_ref(O, i, ch)}, ins=_cols(O, seed, LOOKUP_ARGS, N << EXT), inout=["values"])


@row("quotient_lookup_cosets", "sg_quotient_lookup_cosets_dev", "arithmetic.quotient_lookup_cosets")
def _(O, seed, cold):
    import coset_cases as cc
    ch = [_word(O, seed, 21 + j) for j in range(3)]
    dev, ext_of = _gathered(O, seed, LOOKUP_ARGS)
    call = lambda b, h, ctx: _A().quotient_lookup_cosets(*[b[n] for n in LOOKUP_ARGS], *ch, K, N_COSETS)
    return Case(call, lambda i: {"values": cc.gather(_lookup_ref(O, ext_of(i), ch), K, EXT, N_COSETS)}, ins=dev, inout=["values"])


GATES_CASE = "random_folded_seed502_calc40"


def _gates(O, seed, cosets):
    """a folded random program of gates_cases' device corpus (3 fixed, 4 advice, 1 instance column, 2 challenges); the columns
    and the previous values differ between real and decoy, the program's constants and the challenges are host arguments"""
    import gates_cases as gc
    case = gc.device_case(O, GATES_CASE)
    rows = (cosets << K) if cosets else (N << EXT)
    inp = [gc.make_inputs(O, case, "random", rows, seed=50 + 2 * seed + w) for w in (0, 1)]
    groups = [("fixed", case.n_fixed), ("advice", case.n_advice), ("instance", case.n_instance)]
    ins = {"previous": (inp[0]["previous"], inp[1]["previous"])}
    for grp, cnt in groups:
        for c in range(cnt):
            ins[f"{grp}{c}"] = (inp[0][grp][c], inp[1][grp][c])
    host = {n: inp[0][n] for n in ("constants", "challenges", "beta", "gamma", "theta", "y")}

    def call(b, h, ctx):
        from circuits_halo2_amd import arithmetic as A
        cols = [[b[f"{grp}{c}"] for c in range(cnt)] for grp, cnt in groups]
        args = (b["previous"], gc.GraphWithConstants(case, host["constants"]), *cols, host["challenges"], host["beta"], host["gamma"], host["theta"], host["y"])
        A.quotient_gates_cosets(*args, K, cosets) if cosets else A.quotient_gates(*args, K, K + EXT)

    def ref(i):
        full = dict(host, previous=i["previous"], **{grp: [i[f"{grp}{c}"] for c in range(cnt)] for grp, cnt in groups})
        return {"previous": gc.expected_rows(O, case, full, K, K + EXT, cosets)}
    return Case(call, ref, ins=ins, inout=["previous"])


@row("quotient_gates", "sg_quotient_gates_dev", "arithmetic.quotient_gates")
def _(O, seed, cold):
    return _gates(O, seed, 0)


@row("quotient_gates_cosets", "sg_quotient_gates_cosets_dev", "arithmetic.quotient_gates_cosets")
def _(O, seed, cold):
    return _gates(O, seed, N_COSETS)


NUM_EXT, NUM_COSETS, NUM_NC = 3, 5, 2        # the reference circuit's quotient: 2^(k + 3) extended rows, five cosets


@row("quotient_numerator_cosets", "sg_quotient_numerator_cosets_dev", "arithmetic.quotient_numerator_cosets", caches="the lowered programs")
def _(O, seed, cold):
    """halo2's evaluate_h on the extended domain by the oracle -- gates (previous value zero), permutation, lookup -- gathered to
    coset-major, as tests/test_gpu_round5_oracle.py states it; the reference circuit's programs with two currencies"""
    import coset_cases as cc
    from circuits_halo2_amd import mst_inclusion as M
    from oracle import pyref as P
    counts = [("fixed", M.NUM_FIXED), ("advice", M.NUM_ADVICE), ("inst", 1), ("z", 2), ("sigma", 6), ("sel", 3), ("look", 3)]
    names = [f"{g}{c}" for g, cnt in counts for c in range(cnt)]
    ek = K + NUM_EXT
    ext = _cols(O, seed, names, 1 << ek)
    dev = {n: tuple(cc.gather(a, K, NUM_EXT, NUM_COSETS) for a in pair) for n, pair in ext.items()}
    back = {bytes(dev[names[0]][w]): {n: ext[n][w] for n in names} for w in (0, 1)}
    beta, gamma, theta = (_word(O, seed, 24 + j) for j in range(3))
    y_int = _ints(_word(O, seed, 27))[0] % P.R
    y, chal = _fr([y_int]), np.ascontiguousarray(M.gate_challenges(y_int, NUM_NC))
    grp = lambda d, g: [d[f"{g}{c}"] for c in range(dict(counts)[g])]
    perm = lambda d: [d["fixed2"], d["advice0"], d["advice1"], d["fixed3"], d["advice2"], d["inst0"]]       # mst_inclusion.PERMUTATION_COLUMNS

    def call(b, h, ctx):
        from circuits_halo2_amd import arithmetic as A
        A.quotient_numerator_cosets(b["values"], M.gate_graph(NUM_NC), M.lookup_input_graph(), grp(b, "fixed"), grp(b, "advice"), grp(b, "inst"), chal,
                                    grp(b, "z"), perm(b), grp(b, "sigma"), 4, *grp(b, "sel"), *grp(b, "look"), b["fixed4"], beta, gamma, theta, y, K, ek,
                                    NUM_COSETS, LAST_ROT)

    def ref(i):
        e = back[bytes(i[names[0]])]
        zeros, none = np.zeros(32 << ek, dtype=np.uint8), np.zeros(0, dtype=np.uint8)
        cols = (grp(e, "fixed"), grp(e, "advice"), grp(e, "inst"))
        v = O.quotient_gates(zeros, M.gate_graph(NUM_NC).as_dict(), *cols, chal, beta, gamma, theta, y, K, ek)
        v = O.quotient_permutation(v, grp(e, "z"), perm(e), grp(e, "sigma"), 4, *grp(e, "sel"), beta, gamma, y, K, ek, LAST_ROT)
        a = O.quotient_gates(zeros, M.lookup_input_graph().as_dict(), *cols, none, beta, gamma, theta, y, K, ek)
        lz, pin, ptab = grp(e, "look")
        v = O.quotient_lookup(v, lz, pin, ptab, a, e["fixed4"], *grp(e, "sel"), beta, gamma, y, K, ek)
        return {"values": cc.gather(v, K, NUM_EXT, NUM_COSETS)}
    return Case(call, ref, ins=dev, outs={"values": (32 * NUM_COSETS) << K})


# ============================================================================= the Merkle sum tree and the witness
MST_NC = 2


@row("mst_leaves", "sg_mst_leaves_dev", "ffi.lib()")
def _(O, seed, cold):
    def call(b, h, ctx):
        _check(_ffi()[1].sg_mst_leaves_dev(_p(b["usernames"]), _p(b["balances"]), C.c_size_t(N), C.c_uint32(MST_NC), _p(b["hashes"]), _stream()))
    ins = {"usernames": _pair(O, seed, N, 1), "balances": _pair(O, seed, N * MST_NC, 2)}
    return Case(call, lambda i: {"hashes": O.mst_leaves(i["usernames"], i["balances"], MST_NC)}, ins=ins, outs={"hashes": 32 * N})


@row("mst_level", "sg_mst_level_dev", "ffi.lib()")
def _(O, seed, cold):
    def call(b, h, ctx):
        _check(_ffi()[1].sg_mst_level_dev(_p(b["child_hashes"]), _p(b["child_balances"]), C.c_size_t(N), C.c_uint32(MST_NC), _p(b["hashes"]),
                                          _p(b["balances"]), _stream()))
    ins = {"child_hashes": _pair(O, seed, 2 * N, 1), "child_balances": _pair(O, seed, 2 * N * MST_NC, 2)}
    ref = lambda i: dict(zip(("hashes", "balances"), O.mst_level(i["child_hashes"], i["child_balances"], MST_NC)))
    return Case(call, ref, ins=ins, outs={"hashes": 32 * N, "balances": 32 * N * MST_NC})


@row("mst_build", "sg_mst_build_dev", "ffi.lib()")
def _(O, seed, cold):
    import witness_cases as wc

    def call(b, h, ctx):
        _check(_ffi()[1].sg_mst_build_dev(_p(b["usernames"]), _p(b["balances"]), C.c_uint32(K), C.c_uint32(MST_NC), _p(b["node_hashes"]),
                                          _p(b["node_balances"]), _stream()))
    ins = {"usernames": _pair(O, seed, N, 1), "balances": _pair(O, seed, N * MST_NC, 2)}
    ref = lambda i: dict(zip(("node_hashes", "node_balances"), wc.expected_tree(O, i["usernames"], i["balances"], K, MST_NC)[:2]))
    return Case(call, ref, ins=ins, outs={"node_hashes": 32 * (2 * N - 1), "node_balances": 32 * (2 * N - 1) * MST_NC})


def _entries(seed, which, n=N):
    """n entries with names and balances of fixed widths (so that real and decoy have one shape), all different"""
    tag = "ab"[which]
    return [(f"user{tag}{seed % 10}{i:05d}", [10 ** 11 + (7919 * i + 13 * c + 1000 * which + seed) % 10 ** 11 for c in range(MST_NC)]) for i in range(n)]


def _entry_words(entries):
    from oracle import pyref as P
    e = [P.mst_entry(name, bal) for name, bal in entries]
    return _fr([u for u, _ in e]), _fr([b for _, bal in e for b in bal])


@row("mst_entries", "sg_mst_entries_dev", "ffi.lib()", caches="scratch slots")
def _(O, seed, cold):
    """HOST inputs in pageable memory: they have been read when the call returns, so the test overwrites them with the decoy's
    as soon as the call is back"""
    from circuits_halo2_amd.merkle_sum_tree import pack_entries
    packs = [pack_entries(_entries(seed, w), MST_NC) for w in (0, 1)]
    keys = ("name_bytes", "name_off", "digit_bytes", "digit_off")
    host = {k: tuple(np.ascontiguousarray(p[j]).copy() for p in packs) for j, k in enumerate(keys)}
    assert all(a.shape == b.shape for a, b in host.values())
    want = {bytes(packs[w][0]): dict(zip(("usernames", "balances"), _entry_words(_entries(seed, w)))) for w in (0, 1)}

    def call(b, h, ctx):
        _check(_ffi()[1].sg_mst_entries_dev(*[_hp(h[k]) for k in keys], C.c_size_t(N), C.c_size_t(N), C.c_uint32(MST_NC), _p(b["usernames"]),
                                            _p(b["balances"]), _stream()))
    return Case(call, lambda i: want[bytes(i["name_bytes"])], host_ins=host, outs={"usernames": 32 * N, "balances": 32 * N * MST_NC},
                note="expected: pyref.mst_entry (keccak256 of the name mod r, the balances mod r) as Montgomery words")


def _csv_text(seed, which, merged=False):
    body = "".join(f"{name},{bal[0]},{bal[1]}\n" for name, bal in _entries(seed, which))
    if merged:                                              # every second line end becomes a letter: half the rows, the same bytes
        lines = body.split("\n")[:-1]
        body = "".join(l + ("x" if j % 2 == 0 else "\n") for j, l in enumerate(lines))
    head = "username,balance_ETH_ETH,balance_USDT_ETH\n"
    return np.frombuffer((head + body).encode(), dtype=np.uint8).copy(), len(head)


CSV_TILE = 4096          # include/summa_gpu.h, sg_mst_csv_geometry: the bytes a workgroup scans


def _csv_tiles(nbytes):
    """bytes of the scan's tile scratch"""
    return 4 * (-(-nbytes // CSV_TILE) + 2)


@row("mst_csv_scan", "sg_mst_csv_scan_dev", "ffi.lib()")
def _(O, seed, cold):
    """the host result is the row count and the flags; the decoy is the same text with every second line end replaced by a
    letter: half the rows in the same number of bytes.  The tile scratch's contents are the library's own"""
    real, off = _csv_text(seed, 0)
    decoy, _ = _csv_text(seed, 0, merged=True)
    assert real.size == decoy.size

    def call(b, h, ctx):
        n_rows, flags = C.c_uint64(0), C.c_uint32(0)
        _check(_ffi()[1].sg_mst_csv_scan_dev(_p(b["text"]), real.size, off, _p(b["tiles"]), C.byref(n_rows), C.byref(flags), _stream()))
        return np.frombuffer(n_rows.value.to_bytes(8, "little") + flags.value.to_bytes(4, "little"), dtype=np.uint8).copy()

    def ref(i):
        lines = bytes(i["text"][off:]).split(b"\n")
        assert lines[-1] == b""
        return {"host": np.frombuffer((len(lines) - 1).to_bytes(8, "little") + bytes(4), dtype=np.uint8).copy()}
    return Case(call, ref, ins={"text": (real, decoy)}, opaque={"tiles": _csv_tiles(real.size - off)},
                note="expected: the lines of the body, counted in Python; no flag")


@row("mst_csv_entries", "sg_mst_csv_entries_dev", "ffi.lib()")
def _(O, seed, cold):
    """real and decoy are two files of one layout (names and balances of fixed widths) with other names and other balances; the
    tile scratch is what a scan of that layout leaves (made in the set-up, complete before the test's first wait)"""
    texts = [_csv_text(seed, w) for w in (0, 1)]
    off = texts[0][1]
    size = texts[0][0].size
    assert texts[1][0].size == size
    want = {bytes(t): dict(zip(("usernames", "balances"), _entry_words(_entries(seed, w)))) for w, (t, _) in enumerate(texts)}

    def setup():
        import torch
        ffi, L = _ffi()
        d_text = torch.from_numpy(texts[0][0]).cuda()
        tiles = torch.zeros(_csv_tiles(size - off), dtype=torch.uint8, device="cuda")
        n_rows, flags = C.c_uint64(0), C.c_uint32(0)
        _check(L.sg_mst_csv_scan_dev(_p(d_text), size, off, _p(tiles), C.byref(n_rows), C.byref(flags), None))
        torch.cuda.synchronize()
        assert (n_rows.value, flags.value) == (N, 0)
        return tiles

    def call(b, h, ctx):
        problem = C.c_uint64(1 << 40)
        _check(_ffi()[1].sg_mst_csv_entries_dev(_p(b["text"]), size, off, _p(ctx), ord(","), MST_NC, N, N, _p(b["spans"]), _p(b["usernames"]),
                                                _p(b["balances"]), C.byref(problem), _stream()))
        return np.frombuffer(problem.value.to_bytes(8, "little"), dtype=np.uint8).copy()

    def ref(i):
        return dict(want[bytes(i["text"])], host=np.zeros(8, dtype=np.uint8))
    return Case(call, ref, ins={"text": (texts[0][0], texts[1][0])}, outs={"usernames": 32 * N, "balances": 32 * N * MST_NC}, aux=["host"],
                opaque={"spans": 8 * (N + 2 + 2 * N * (1 + MST_NC))}, setup=setup)


UPDATED = [0, 5, N - 1]


@row("mst_update", "sg_mst_update_dev", "ffi.lib()", caches="scratch slots")
def _(O, seed, cold):
    """the tree (four device arrays) is the device input and output; the new balances are HOST inputs in pageable memory, read
    when the call returns.  Expected: the oracle's tree over the changed leaves"""
    import witness_cases as wc
    from circuits_halo2_amd.merkle_sum_tree import pack_balances
    users = _pair(O, seed, N, 1)
    bals = _pair(O, seed, N * MST_NC, 2)
    trees = [wc.expected_tree(O, u, b, K, MST_NC)[:2] for u, b in zip(users, bals)]
    new = [[10 ** 12 + 1000 * w + 10 * j + c + seed for j in range(len(UPDATED)) for c in range(MST_NC)] for w in (0, 1)]
    packs = [pack_balances(f) for f in new]
    host = {"digit_bytes": tuple(np.ascontiguousarray(p[0]).copy() for p in packs), "digit_off": tuple(np.ascontiguousarray(p[1]).copy() for p in packs)}
    idx = np.array(UPDATED, dtype=np.uint32)
    ins = {"usernames": users, "leaf_balances": bals, "node_hashes": tuple(t[0] for t in trees), "node_balances": tuple(t[1] for t in trees)}

    def call(b, h, ctx):
        _check(_ffi()[1].sg_mst_update_dev(_hp(idx), _hp(h["digit_bytes"]), _hp(h["digit_off"]), len(UPDATED), K, MST_NC, _p(b["usernames"]),
                                           _p(b["leaf_balances"]), _p(b["node_hashes"]), _p(b["node_balances"]), _stream()))

    def ref(i):
        leaf = np.array(i["leaf_balances"])
        fresh = _fr([int(bytes(i["digit_bytes"][int(a):int(b)])) for a, b in zip(i["digit_off"], i["digit_off"][1:])])
        for j, at in enumerate(UPDATED):
            leaf[32 * MST_NC * at:32 * MST_NC * (at + 1)] = fresh[32 * MST_NC * j:32 * MST_NC * (j + 1)]
        h, b = wc.expected_tree(O, i["usernames"], leaf, K, MST_NC)[:2]
        return {"leaf_balances": leaf, "node_hashes": h, "node_balances": b}
    return Case(call, ref, ins=ins, host_ins=host, inout=["leaf_balances", "node_hashes", "node_balances"])


WITNESS_SHAPE = (2, 2, 8)          # levels, currencies, bytes of a range check: a configuration of witness_cases.WITNESS_CONFIGS


@row("mst_inclusion_witness", "sg_mst_inclusion_witness_dev", "ffi.lib()")
def _(O, seed, cold):
    """real: witness_cases' tree with every balance in range, decoy: its tree with balances out of range (the same usernames).
    Expected: witness_cases.reference_columns.  The floor plan fixes most cells of the three columns (zeros, path bits, sponge
    constants, running sums of balances both trees share), so the two results differ in a part of the rows only: at least one
    row in every user's every column"""
    import witness_cases as wc
    cfg = wc.config(*WITNESS_SHAPE)
    rows = 1 << cfg.k
    idx = wc.witness_users(cfg.levels)
    kinds = wc.TREE_KINDS
    trees = [wc.witness_tree(cfg.levels, cfg.nc, kind, cfg.n_bytes) for kind in kinds]

    def words(t):
        return (wc.mont(t.users), wc.mont([h for level in t.node_hash for h in level]), wc.mont([b for level in t.node_bal for node in level for b in node]))
    w = [words(t) for t in trees]
    ins = {name: (w[0][j], w[1][j]) for j, name in enumerate(("usernames", "node_hashes", "node_balances"))}
    kind_of = {bytes(w[j][2]): kinds[j] for j in (0, 1)}

    def setup():
        import torch
        return (torch.from_numpy(wc.program(cfg).view(np.int32).copy()).cuda(), torch.tensor(idx, dtype=torch.int32, device="cuda"))

    def call(b, h, ctx):
        _check(_ffi()[1].sg_mst_inclusion_witness_dev(_p(ctx[0]), C.c_uint32(cfg.n_items), C.c_uint32(cfg.n_absorbs), _p(b["usernames"]), _p(b["node_hashes"]),
                                                      _p(b["node_balances"]), C.c_uint32(cfg.levels), C.c_uint32(cfg.nc), _p(ctx[1]), C.c_uint32(len(idx)),
                                                      _p(b["advice"]), C.c_uint64(rows), _stream()))

    def ref(i):
        kind = kind_of[bytes(i["node_balances"])]
        return {"advice": _cat([wc.mont(col) for u in idx for col in wc.reference_columns(cfg, kind, u)])}
    return Case(call, ref, ins=ins, outs={"advice": 32 * len(idx) * 3 * rows}, setup=setup, blocks={"advice": 3 * len(idx)})
