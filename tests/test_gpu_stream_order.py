"""Every device entry point of include/summa_gpu.h held to its stream-order contract: the work a caller enqueued earlier on the
stream is seen by the call, the work it enqueues afterwards sees the call's results, and no host wait is needed in between.

Every row of tests/stream_cases.py runs this sequence on a fresh stream S, with no host wait between steps 2 and 5:
  1. the DECOY in the input buffers, 0x5A in the outputs, torch.cuda.synchronize()
  2. on S: a delay kernel (torch.cuda._sleep), then device-to-device copies of the REAL inputs into the input buffers -- the
     producer in flight
  3. on S: the entry point
  4. on S: the outputs copied into separate consumer tensors, then the input buffers overwritten with the decoy -- the trailer
  5. torch.cuda.synchronize()
and then the consumer tensors (and the host result of an entry that returns one) must equal, bit for bit, what the oracle gives
for the real inputs.  A call that missed the producer shows the decoy's result; a call whose output had not joined S shows 0x5A;
a call still reading its inputs after it returned shows the decoy's result through the trailer.  Host buffers that the header
says are read before the call returns are overwritten with the decoy's as soon as it is back.

The delay is measured, not guessed: torch.cuda._sleep is calibrated against events once, every row is run once undelayed between
two events (producer copies, call and trailer), and the delay is ten times the slowest row, at least 20 ms and at most 200 ms.
Measured on an MI355X, twice: 2 396 354 and 2 398 157 cycles of _sleep per millisecond; slowest row g1_fft (eight butterfly stages
over 256 points, a set-up operation) at 18.3 and 18.5 ms undelayed; delay 182.6 and 185.4 ms (437 634 456 and 444 686 659 cycles).
The figures of a run are in the control's assertion message and in the line the module prints.
The control shows that the delay holds a stream back: without an edge to S, a stream on another hardware queue reads the buffer
before S's producer has written it."""
import ctypes as C
import threading

import numpy as np
import pytest

import stream_cases as sc

pytestmark = pytest.mark.gpu

ALL = [r.name for r in sc.ROWS]
CACHED = [r.name for r in sc.ROWS if r.caches]
PER_STREAM = [r.name for r in sc.ROWS if r.per_stream]
MIN_DELAY_MS, MAX_DELAY_MS, MARGIN = 20.0, 200.0, 10.0


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from circuits_halo2_amd import ffi
    ffi.check(ffi.lib().sg_init(0))
    return ffi


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


class Run:
    """one case's buffers on the device: the input buffers hold the decoy, the outputs 0x5A (step 1, before the caller's wait)"""

    def __init__(self, case, ctx=None, set_params=True):
        import torch
        self.case = case
        self.set_params = set_params
        self.own_ctx = ctx is None
        self.ctx = case.setup() if ctx is None else ctx
        self.real = {n: _dev(p[0]) for n, p in case.ins.items()}
        self.decoy = {n: _dev(p[1]) for n, p in case.ins.items()}
        self.buf = {n: t.clone() for n, t in self.decoy.items()}
        for n, size in list(case.outs.items()) + list(case.opaque.items()):
            self.buf[n] = torch.full((size,), sc.FILL, dtype=torch.uint8, device="cuda")
        self.consumer = {n: torch.zeros_like(self.buf[n]) for n in case.output_names()}
        self.host = {n: p[0].copy() for n, p in case.host_ins.items()}
        self.result = None

    def issue(self, stream, cycles):
        """steps 2 to 4 on `stream`; nothing here waits for the device (an entry that returns a value to the host does)"""
        import torch
        case = self.case
        with torch.cuda.stream(stream):
            if cycles:
                torch.cuda._sleep(cycles)
            for n in case.ins:
                self.buf[n].copy_(self.real[n], non_blocking=True)
            for n, p in case.host_ins.items():
                self.host[n][...] = p[0]
            from circuits_halo2_amd import ffi
            with ffi.params(case.params if self.set_params else {}):      # (library parameters, per lane: the lanes are idle here)
                self.result = case.call(self.buf, self.host, self.ctx)
            for n, p in case.host_ins.items():
                self.host[n][...] = p[1]                      # read before the call returned, says the header
            for n in case.output_names():
                self.consumer[n].copy_(self.buf[n], non_blocking=True)
            for n in case.ins:
                self.buf[n].copy_(self.decoy[n], non_blocking=True)

    def check(self, what):
        """after the caller's wait: every consumer tensor and the host result against the oracle, bit for bit"""
        want, decoy = self.case.want("real"), self.case.want("decoy")
        got = {n: t.cpu().numpy() for n, t in self.consumer.items()}
        if "host" in want:
            assert self.result is not None, what
            got["host"] = np.ascontiguousarray(self.result, dtype=np.uint8).reshape(-1)
        assert set(got) == set(want), what
        for n in sorted(want):
            if np.array_equal(got[n], want[n]):
                continue
            g, w, d = sc.rows_of(got[n]), sc.rows_of(want[n]), sc.rows_of(decoy[n])
            assert g.shape == w.shape, f"{what}: {n} has {got[n].size} bytes, expected {want[n].size}"
            bad = (g != w).any(axis=1)
            as_decoy = int(((g == d).all(axis=1) & bad).sum())
            stale = int(((g == sc.FILL).all(axis=1) & bad).sum())
            raise AssertionError(f"{what}: {n}: {int(bad.sum())} of {bad.size} rows differ from the oracle's result for the real inputs, first at row "
                                 f"{int(np.argmax(bad))}; {as_decoy} of them are the decoy's result (the call missed the producer, or read its inputs "
                                 f"after it returned), {stale} are 0x5A (the output had not joined the stream)")

    def close(self):
        if self.own_ctx:
            self.case.cleanup(self.ctx)


def _timed(stream, fn):
    """milliseconds between two events around fn() on `stream`"""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(stream)
    fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


@pytest.fixture(scope="module")
def delay(gpu):
    """{"cycles", "ms", "cycles_per_ms", "slowest": (row, ms)}: torch.cuda._sleep calibrated against events, every row timed once
    undelayed (producer copies, call, trailer; the first call of a row also builds what the library caches, so the figure errs
    high), the delay ten times the slowest row within 20 .. 200 ms"""
    import torch
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        torch.cuda._sleep(1_000_000)
    probe = 20_000_000

    def spin():
        with torch.cuda.stream(s):
            torch.cuda._sleep(probe)
    per_ms = probe / _timed(s, spin)
    slowest = ("", 0.0)
    for name in ALL:
        run = Run(sc.built(name))
        try:
            ms = min(_timed(s, lambda: run.issue(s, 0)) for _ in range(2))         # the second time without the cache fills
        finally:
            torch.cuda.synchronize()
            run.close()
        slowest = max(slowest, (name, ms), key=lambda x: x[1])
    ms = min(MAX_DELAY_MS, max(MIN_DELAY_MS, MARGIN * slowest[1]))
    d = {"cycles": int(ms * per_ms), "ms": ms, "cycles_per_ms": per_ms, "slowest": slowest}
    print(f"\nstream order: {_report(d)}")
    return d


def _report(d):
    return (f"slowest row {d['slowest'][0]} {d['slowest'][1]:.3f} ms undelayed, {d['cycles_per_ms']:.0f} _sleep cycles per ms, "
            f"delay {d['ms']:.1f} ms = {d['cycles']} cycles")


def _streams(n):
    import torch
    return [torch.cuda.Stream() for _ in range(n)]


def _run_all(runs_and_streams, cycles, what):
    """step 1's wait, every run issued on its stream with its own delayed producer, ONE wait, every result checked"""
    import torch
    try:
        torch.cuda.synchronize()
        for run, stream in runs_and_streams:
            run.issue(stream, cycles)
        torch.cuda.synchronize()
        for j, (run, _) in enumerate(runs_and_streams):
            run.check(f"{what}, call {j}" if len(runs_and_streams) > 1 else what)
    finally:
        torch.cuda.synchronize()
        for run, _ in runs_and_streams:
            run.close()


# ============================================================================= the control
PROBES = 5          # more streams than the runtime has hardware queues by default (four)


def test_the_delay_holds_a_stream_back(gpu, delay):
    """On S the delay and a copy real -> buffer; on PROBES further streams with NO edge to S a copy buffer -> probe each.  A probe
    that holds the decoy after the wait read the buffer (valid, allocated memory) before S's producer wrote it: one such probe
    shows that the delay holds a stream back.  The runtime puts all streams on a few hardware queues, and a probe stream that
    shares S's queue runs behind the delay and reads the real words (or some of them, beside S's copy); that says nothing
    about the delay, so several consecutive streams are probed and the two cases are told apart.  Between issuing the work
    and the look at S nothing else touches the device, and the probes are compared on the host after the wait"""
    import torch
    n = 1 << 15
    real_h, decoy_h = np.full(n, 0x11, dtype=np.uint8), np.full(n, 0xEE, dtype=np.uint8)
    real, decoy = _dev(real_h), _dev(decoy_h)
    buf = decoy.clone()
    probes = [torch.zeros_like(decoy) for _ in range(PROBES)]
    s, *others = _streams(1 + PROBES)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        torch.cuda._sleep(delay["cycles"])
        buf.copy_(real, non_blocking=True)
    for probe, other in zip(probes, others):
        with torch.cuda.stream(other):
            probe.copy_(buf, non_blocking=True)
    busy = not s.query()                    # straight after issuing: no kernel, no wait in between
    torch.cuda.synchronize()
    holds = [p.cpu().numpy() for p in probes]
    assert np.array_equal(buf.cpu().numpy(), real_h)
    early = [j for j, h in enumerate(holds) if np.array_equal(h, decoy_h)]
    behind = [j for j, h in enumerate(holds) if np.isin(h, (0x11, 0xEE)).all() and (h == 0x11).any()]
    figures = (f"probes that hold the decoy (they read before S's producer wrote): {early}; probes that hold real words (they ran behind the delay: "
               f"they share a hardware queue with S): {behind}; S busy when everything was issued: {busy}; {_report(delay)}")
    assert sorted(early + behind) == list(range(PROBES)), f"a probe holds neither the decoy nor the real words; {figures}"
    assert busy, f"the delay is too short: S had passed its producer by the time the probes were issued; {figures}"
    assert early, f"every probe stream ran behind S, as if all of them shared its hardware queue: the control cannot tell whether the delay holds; {figures}"
    assert MIN_DELAY_MS <= delay["ms"] <= MAX_DELAY_MS and (delay["ms"] >= MARGIN * delay["slowest"][1] or delay["ms"] == MAX_DELAY_MS), figures
    print(f"\nstream order control: {figures}")


# ============================================================================= every row behind a producer in flight
@pytest.mark.parametrize("name", ALL)
def test_call_is_ordered_on_its_stream(gpu, delay, name):
    """the row's sequence, twice: on two fresh streams made one after the other, with different real inputs.  The runtime
    multiplexes streams onto a few hardware queues (four by default), and two streams that share a queue run in the order of
    submission -- which would hide a missing edge between the caller's stream and a stream of the library's own.  An
    observation of this runtime, not a property any test pins: with the wait of sg_msm_g1_dev taken out by hand, a row on one
    stream stayed green in some runs, and the same row on two streams made one after the other turned red in every run, as
    if consecutive streams sat on different queues.  The second run costs a fraction of a second and can only add sensitivity"""
    for j, stream in enumerate(_streams(2)):
        _run_all([(Run(sc.built(name, j)), stream)], delay["cycles"], f"{name}, stream {j}")


def test_msm_on_an_idle_stream(gpu, delay):
    """the other side of sg_msm_g1_dev's `hipStreamQuery(stream)`: nothing in flight on S, so no edge is recorded -- the inputs
    are in place, the point is the oracle's, and the trailer still finds the call complete"""
    import torch
    run = Run(sc.built("msm_g1"))
    s = _streams(1)[0]
    for n in run.case.ins:
        run.buf[n].copy_(run.real[n])
    torch.cuda.synchronize()
    assert s.query()
    with torch.cuda.stream(s):
        run.result = run.case.call(run.buf, run.host, run.ctx)
        for n in run.case.ins:
            run.buf[n].copy_(run.decoy[n], non_blocking=True)
    torch.cuda.synchronize()
    run.check("msm_g1 on an idle stream")


def test_the_batch_rows_run_as_the_fused_jobs_the_table_claims(gpu, delay):
    """the launch log of the accumulations ("msm.acc_log") while each batch row runs once, undelayed: as many fused jobs as
    stream_cases.row_groups works out from the library's limits, of those sizes, fixed-base where the row's SRS has its table --
    at least three, so that both engines and the finish path of a third group run behind the producer in the rows above"""
    import torch
    for name in sc.BATCH_ROWS:
        lengths, fixed, groups = sc.row_groups(name)
        run = Run(sc.built(name))
        try:
            torch.cuda.synchronize()
            with gpu.params({"msm.acc_log": 1}):
                run.issue(_streams(1)[0], 0)
                torch.cuda.synchronize()
                log = gpu.msm_launch_log()
            run.check(name)
            got = sorted((r["M"], r["n"], r["fixed"]) for r in log)
            want = sorted((count, lengths[first], int(fixed)) for first, count in groups)
            assert got == want and len(got) >= 3, f"{name}: accumulation launches (M, n, fixed-base) {got}, expected {want}"
        finally:
            torch.cuda.synchronize()
            run.close()


# ============================================================================= cold and warm caches
@pytest.mark.parametrize("name", CACHED)
def test_first_call_of_a_shape_then_a_second_stream(gpu, delay, name):
    """what the entry caches (plans, twiddles, domain constants, coset tables, t_evals, work spaces, scratch slots) is made by
    the first call, on S behind its delayed producer; the second call of the shape is issued at once on S2 behind a delayed
    producer of its own and must not use a table S has not finished.  The lanes' plans and work spaces are given back first
    (sg_collect_retired) and the sizes are ones no other test of the module uses"""
    gpu.check(gpu.lib().sg_collect_retired())
    s, s2 = _streams(2)
    _run_all([(Run(sc.built(name, 2, True)), s), (Run(sc.built(name, 3, True)), s2)], delay["cycles"], f"{name} cold, then warm")


# ============================================================================= two streams, call by call
@pytest.mark.parametrize("name", PER_STREAM)
def test_two_streams_interleaved(gpu, delay, name):
    """the rows whose work space is the stream's: four different real inputs issued on S and S2 in turn, delayed producers on
    both, one wait -- each result is its own"""
    s, s2 = _streams(2)
    runs = [(Run(sc.built(name, seed)), (s, s2)[seed % 2]) for seed in range(4)]
    import torch
    try:
        torch.cuda.synchronize()
        for j, (run, stream) in enumerate(runs):
            run.issue(stream, delay["cycles"] if j < 2 else 0)      # one delay per stream: the later calls queue behind it
        torch.cuda.synchronize()
        for j, (run, _) in enumerate(runs):
            run.check(f"{name}, call {j} on stream {j % 2}")
    finally:
        torch.cuda.synchronize()
        for run, _ in runs:
            run.close()


# ============================================================================= the commit combiner
def test_combined_commitments_wait_for_each_members_producer(gpu, delay):
    """sg_commit_batch_mixed_dev between sg_commit_combine_begin and _end from two threads, each with its own stream and its own
    delayed producer: the fused job is ordered after each member's stream.  Both threads' points are the oracle's for the
    real scalars, and sg_commit_combine_stats shows that the two requests ran as one job -- otherwise nothing was fused and
    the case proves nothing"""
    import torch
    L = gpu.lib()

    def stats():
        a, b = C.c_uint64(0), C.c_uint64(0)
        gpu.check(L.sg_commit_combine_stats(C.byref(a), C.byref(b)))
        return a.value, b.value

    from oracle import oracle as O
    cases = [sc.mixed_case(O, 5 + t) for t in range(2)]
    srs = cases[0].setup()
    runs = [Run(c, ctx=srs, set_params=False) for c in cases]      # (set once below, not by two threads at a time)
    streams = _streams(2)
    errors, gate = [], threading.Barrier(2)

    def member(t):
        try:
            gpu.bind_thread()
            gpu.check(L.sg_commit_combine_begin())
            try:
                gate.wait(timeout=60)
                runs[t].issue(streams[t], delay["cycles"])
            finally:
                gpu.check(L.sg_commit_combine_end())
        except Exception as e:                                   # noqa: BLE001 -- reported below
            errors.append(e)

    try:
        # the two requests are pending together: the runner waits for the second member for up to 100 ms, and no longer than it takes to arrive
        with gpu.params({"commit.combine_wait_us": 100000, "commit.combine_target": 2, **cases[0].params}):
            torch.cuda.synchronize()
            j0, r0 = stats()
            threads = [threading.Thread(target=member, args=(t,)) for t in range(2)]
            for th in threads:
                th.start()
            for th in threads:
                th.join()
            torch.cuda.synchronize()
            j1, r1 = stats()
        assert not errors, errors
        for t, run in enumerate(runs):
            run.check(f"combined commitments, thread {t}")
        assert (r1 - r0, j1 - j0) == (2, 1), f"{r1 - r0} requests ran as {j1 - j0} jobs: nothing was fused, the case proves nothing"
    finally:
        torch.cuda.synchronize()
        cases[0].cleanup(srs)
