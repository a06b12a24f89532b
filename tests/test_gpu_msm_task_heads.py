"""GPU tests of the task head and the steady-state loop of msm_accumulate (csrc/msm_accumulate.cuh): the first point of a
task by xyzz29_from_affine, the first two by the affine + affine addition, every later point by the signed mixed addition
that updates the accumulator in place, and the whole task over again by the deciding additions wherever a lane met a point
at infinity, a doubling or a cancellation.

Narrow windows (msm.window_bits = 4) and short tasks (msm.log_seg = 1, 2, 3: tasks of 2, 4 and 8 entries) put 65 .. 600 points
into a handful of deep buckets, so that one small MSM holds tasks of every length from 1 to 8, merge rounds behind them, and
the group-law edge cases at chosen positions of a task.  Every expected point is the oracle's best_multiexp of the same
inputs."""
import numpy as np
import pytest

import msm_cases as mc

pytestmark = pytest.mark.gpu

N_MAX = 600
C = 4


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    import circuits_halo2_amd as sg
    from circuits_halo2_amd import ffi
    ffi.check(sg.lib().sg_init(0))
    return sg


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def points(O):
    """N_MAX points s_i * G in the memory format (host); cases take a prefix and edit it"""
    return O.fixed_base_mul(O.random_fr(0x7A5C, N_MAX), O.ncpu())


def from_digits(digits):
    """the scalar whose window digits (tests/msm_cases.window_plan(C): signed but for the top window) are `digits`"""
    width = mc.window_plan(C)
    assert len(digits) == len(width)
    v, at = 0, 0
    for d, w in zip(digits, width):
        assert -(1 << (w - 1)) < d < (1 << (w - 1))
        v += d << at
        at += w
    from oracle import pyref as P
    assert 0 < v < P.R
    return v


W = len(mc.window_plan(C))
MIXED = from_digits([(1, -2, 3, -1, 2, -3)[w % 6] for w in range(W - 1)] + [1])       # one deep bucket per window, both signs
ALL_NEG = from_digits([-3] * (W - 1) + [1])                                           # every signed digit negative
ALL_POS = from_digits([3] * (W - 1) + [1])                                            # the same buckets with the other sign


def scalars_of(kind, n):
    if kind == "equal":
        return [MIXED] * n
    if kind == "negative":
        return [ALL_NEG] * n
    if kind == "alternating":      # one bucket per window whose entries change sign from one to the next
        return [ALL_POS if i % 2 == 0 else ALL_NEG for i in range(n)]
    raise KeyError(kind)


def negated(point):
    """(x, -y) of a 64-byte affine point in the memory format (Montgomery form: -y is q - y there too)"""
    from oracle import pyref as P
    y = int.from_bytes(point[32:].tobytes(), "little")
    out = point.copy()
    out[32:] = np.frombuffer(((P.Q - y) % P.Q).to_bytes(32, "little"), dtype=np.uint8)
    return out


def edited(points, n, edit):
    """the first n points with the edge case `edit` written into them"""
    b = points[:64 * n].copy().reshape(n, 64)
    mid = n // 2 + 1
    if edit == "twice":            # the same point twice in a row: at the head of a task, and further in
        b[1] = b[0]
        b[mid] = b[mid - 1]
        b[n - 1] = b[n - 2]
    elif edit == "thrice":         # ... and three times: the doubled point meets the point again
        b[1] = b[0]
        b[2] = b[0]
        b[mid] = b[mid - 1]
        b[mid + 1] = b[mid - 1]
    elif edit == "negated":        # a point followed by its negative: the head and a later pair cancel
        b[1] = negated(b[0])
        b[mid] = negated(b[mid - 1])
        b[n - 1] = negated(b[n - 2])
    elif edit == "identity0":
        b[0] = 0
    elif edit == "identity1":
        b[1] = 0
    elif edit == "identity_mid":
        b[mid] = 0
    elif edit == "identities":     # index 0, index 1 and the middle at once, and the last point
        b[0] = 0
        b[1] = 0
        b[mid] = 0
        b[n - 1] = 0
    else:
        assert edit is None
    return b.reshape(-1)


# (n, scalars, edit of the bases): with equal scalars a bucket holds all n entries in tasks of L, the last one of n mod L
CASES = [(n, "equal", None) for n in (65, 66, 67, 68, 69, 597)]
CASES += [(67, "negative", None), (70, "alternating", None), (599, "alternating", None)]
CASES += [(66, "equal", "twice"), (69, "negative", "twice"), (71, "equal", "thrice"), (66, "equal", "negated"), (73, "alternating", "negated"),
          (65, "equal", "identity0"), (66, "equal", "identity1"), (67, "negative", "identity_mid"), (77, "alternating", "identities")]


@pytest.mark.parametrize("log_seg", (1, 2, 3))
@pytest.mark.parametrize("n,kind,edit", CASES, ids=[f"{n}-{k}-{e or 'plain'}" for n, k, e in CASES])
def test_task_heads_and_tails(gpu, O, points, n, kind, edit, log_seg):
    """tasks of 1 .. 8 entries with merge rounds behind them, odd and even lengths, both signs, and a doubling, a cancellation
    or a point at infinity at the head of a task and inside it"""
    from circuits_halo2_amd import ffi
    from circuits_halo2_amd.arithmetic import best_multiexp
    k_dev, k_host = mc._mont(mc._ints(scalars_of(kind, n)))
    bases = edited(points, n, edit)
    want = O.best_multiexp(k_host, bases, O.ncpu())
    with ffi.params({"msm.window_bits": C, "msm.log_seg": log_seg}):
        got = best_multiexp(k_dev, mc._dev(bases))
    assert (np.asarray(got) == want).all()


def test_uniform_scalars_on_the_default_plan(gpu, O):
    """2^12 uniform scalars, nothing forced: the shape of the smoke test with both task heads in it"""
    from circuits_halo2_amd.arithmetic import best_multiexp
    n = 1 << 12
    sc = O.random_fr(0x51, n)
    bases = O.fixed_base_mul(O.random_fr(0x52, n), O.ncpu())
    got = best_multiexp(mc._dev(sc), mc._dev(bases))
    assert (np.asarray(got) == O.best_multiexp(sc, bases, O.ncpu())).all()


def test_fixed_base_commitment_k8(gpu, O, points):
    """one commitment of 2^8 coefficients over the window table of a resident SRS: a fixed-base job through the same kernel"""
    n = 1 << 8
    bases = points[:64 * n].copy()
    sc = O.random_fr(0x53, n)
    p = gpu.ParamsKZG(8, bases, bases)
    try:
        p.precompute(0)
        got = p.commit(mc._dev(sc))
    finally:
        p.free()
    assert (np.asarray(got) == O.best_multiexp(sc, bases, O.ncpu())).all()
