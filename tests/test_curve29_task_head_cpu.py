"""The task-head and signed-addition forms of csrc/bn254_curve29.cuh (xyzz29_from_affine, xyzz29_mmadd, the three-argument
xyzz29_madd and the ordinary-case bodies behind them) compiled for the host and checked against Python integers: the group
law for points of the curve, the formulas themselves for coordinates at the top of the load bound (which need not lie on the
curve), and the invariants of the file header (X < 8p, Y < 4p, ZZ, ZZZ < 2p, normalised limbs) on every result.  The same
harness runs once more as a stand-alone program under AddressSanitizer and UBSan."""
import os
import random
import subprocess

import pytest

from conftest import ROOT
from oracle import pyref as P

SRC = os.path.join(ROOT, "tests", "checks", "limb_curve29_head_check.cpp")
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
Q = P.Q
R256, R261 = (1 << 256) % Q, (1 << 261) % Q
M29 = (1 << 29) - 1


def _words(x):
    return " ".join("%x" % ((x >> (32 * i)) & 0xFFFFFFFF) for i in range(8))


def _raw_point(x, y):
    """memory words of the coordinate pair (x, y), on the curve or not"""
    return _words(x * R256 % Q) + " " + _words(y * R256 % Q)


def _point(pt):
    return " ".join(["0"] * 16) if pt is None else _raw_point(*pt)


def _limbs(v):
    """exactly normalised limbs of an integer below 2^261"""
    return " ".join("%x" % (((v >> (29 * i)) & M29) if i < 8 else (v >> 232)) for i in range(9))


def _acc(pt, z, lift=(0, 0, 0, 0)):
    """36 limbs of an XYZZ form of pt with ZZ = z^2, ZZZ = z^3 in the 2^261 domain, each coordinate raised by lift[i] * p"""
    if pt is None:
        return " ".join(["0"] * 36)
    zz, zzz = z * z % Q, z * z * z % Q
    vals = [pt[0] * zz % Q, pt[1] * zzz % Q, zz, zzz]
    return " ".join(_limbs(v * R261 % Q + k * Q) for v, k in zip(vals, lift))


def _decode(line):
    """one output line -> (affine point or None, the four residues out of the 2^261 domain, the raw values)"""
    t = [int(x, 16) for x in line.split()]
    assert len(t) == 32 + 36, line
    res = [sum(t[8 * c + i] << (32 * i) for i in range(8)) * pow(R256, -1, Q) % Q for c in range(4)]
    raw = []
    for c in range(4):
        l = t[32 + 9 * c: 32 + 9 * c + 9]
        assert all(v < (1 << 29) + 4 for v in l[:8]), ("limbs not normalised", line)
        raw.append(sum(v << (29 * i) for i, v in enumerate(l)))
    X, Y, ZZ, ZZZ = res
    for v, r in zip(raw, res):
        assert v % Q == r * R261 % Q, ("canonical words and limbs disagree", line)
    pt = None if ZZ == 0 else (X * pow(ZZ, -1, Q) % Q, Y * pow(ZZZ, -1, Q) % Q)
    if pt is not None:   # the invariants of a stored / accumulated point
        assert raw[0] < 8 * Q and raw[1] < 4 * Q and raw[2] < 2 * Q and raw[3] < 2 * Q, ("lazy bounds exceeded", line)
        assert pow(ZZ, 3, Q) == ZZZ * ZZZ % Q, ("ZZ^3 != ZZZ^2", line)
    return pt, res, raw


def _mmadd_formula(a, b):
    """mmadd-2008-s on plain residues: (X3, Y3, ZZ3, ZZZ3)"""
    (x1, y1), (x2, y2) = a, b
    p, r = (x2 - x1) % Q, (y2 - y1) % Q
    pp = p * p % Q
    ppp = p * pp % Q
    q = x1 * pp % Q
    x3 = (r * r - ppp - 2 * q) % Q
    return [x3, (r * (q - x3) - y1 * ppp) % Q, pp, ppp]


def _signed(pt, neg):
    return P.g1_neg(pt) if neg and pt is not None else pt


def _cases():
    rnd = random.Random(29)
    pts = [P.g1_mul(P.G1_GEN, rnd.randrange(1, P.R)) for _ in range(12)]
    cmds, checks = [], []   # a check consumes its lines and asserts

    def point_is(want):
        def chk(lines):
            assert _decode(lines[0])[0] == want, (lines[0], want)
        return chk, 1

    def formula_is(want):
        def chk(lines):
            assert _decode(lines[0])[1] == want, (lines[0], want)
        return chk, 1

    def both_are(want):
        def chk(lines):
            got, old = _decode(lines[0]), _decode(lines[1])
            assert got[0] == want and old[0] == want, (lines, want)
            assert lines[0].split()[:32] == lines[1].split()[:32], ("signed and negate-then-add forms differ", lines)
        return chk, 2

    # ---- xyzz29_mmadd
    for i in range(6):   # random pairs under every combination of signs
        a, b, na, nb = pts[i], pts[i + 6], i & 1, (i >> 1) & 1
        cmds.append(f"mmadd {_point(a)} {na} {_point(b)} {nb}")
        checks.append(point_is(P.g1_add(_signed(a, na), _signed(b, nb))))
    for na in (0, 1):    # a = b (doubling) and a = -b (identity), reached with and without negations
        a = pts[3]
        cmds.append(f"mmadd {_point(a)} {na} {_point(a)} {na}")
        checks.append(point_is(P.g1_add(_signed(a, na), _signed(a, na))))
        cmds.append(f"mmadd {_point(a)} {na} {_point(a)} {1 - na}")
        checks.append(point_is(None))
        cmds.append(f"mmadd {_point(a)} {na} {_point(P.g1_neg(a))} {na}")
        checks.append(point_is(None))
    for a, b in ((None, pts[1]), (pts[2], None), (None, None)):   # either or both at infinity
        for nb in (0, 1):
            cmds.append(f"mmadd {_point(a)} 0 {_point(b)} {nb}")
            checks.append(point_is(P.g1_add(a, _signed(b, nb))))
    # coordinates at the top of the load bound: memory words p - 1, p - 2 (and small ones against them)
    top = [(Q - 1) * pow(R256, -1, Q) % Q, (Q - 2) * pow(R256, -1, Q) % Q, pow(R256, -1, Q), 0]
    for x1, y1, x2, y2 in ((0, 0, 1, 1), (1, 1, 0, 0), (0, 1, 2, 0), (2, 0, 0, 1), (3, 2, 0, 0), (0, 0, 3, 2), (1, 0, 0, 3)):
        a, b = (top[x1], top[y1]), (top[x2], top[y2])
        for na, nb in ((0, 0), (1, 0), (0, 1), (1, 1)):
            sa, sb = (a[0], (-a[1]) % Q if na else a[1]), (b[0], (-b[1]) % Q if nb else b[1])
            if sa[0] == sb[0]:
                continue
            cmds.append(f"mmadd {_raw_point(*a)} {na} {_raw_point(*b)} {nb}")
            checks.append(formula_is(_mmadd_formula(sa, sb)))
    # ---- xyzz29_from_affine, with and without sign
    for pt in (pts[0], pts[7], None):
        for n in (0, 1):
            cmds.append(f"from {_point(pt)} {n}")
            checks.append(point_is(_signed(pt, n)))
    for x, y in ((0, 0), (1, 1), (0, 3), (3, 1)):
        for n in (0, 1):
            cmds.append(f"from {_raw_point(top[x], top[y])} {n}")
            checks.append(formula_is([top[x], (-top[y]) % Q if n else top[y], 1, 1]))
    # ---- the signed mixed addition against "negate, then xyzz29_madd"
    lifts = ((0, 0, 0, 0), (7, 3, 1, 1), (6, 2, 0, 1), (1, 3, 1, 0))   # up to the top of X < 8p, Y < 4p, ZZ, ZZZ < 2p
    for i in range(8):
        a, q, z = pts[i], pts[(i + 5) % 12], rnd.randrange(1, Q)
        for n in (0, 1):
            cmds.append(f"madd {_acc(a, z, lifts[i % 4])} {_point(q)} {n}")
            checks.append(both_are(P.g1_add(a, _signed(q, n))))
    for lift in lifts:   # accumulator = +-q: doubling and cancellation after the sign is applied
        q, z = pts[9], rnd.randrange(1, Q)
        for acc_neg in (0, 1):
            for n in (0, 1):
                cmds.append(f"madd {_acc(_signed(q, acc_neg), z, lift)} {_point(q)} {n}")
                checks.append(both_are(P.g1_add(_signed(q, acc_neg), _signed(q, n))))
    for n in (0, 1):     # identity accumulator, identity point
        cmds.append(f"madd {_acc(None, 1)} {_point(pts[4])} {n}")
        checks.append(both_are(_signed(pts[4], n)))
        cmds.append(f"madd {_acc(pts[4], 5, lifts[1])} {_point(None)} {n}")
        checks.append(both_are(pts[4]))
    return cmds, checks


@pytest.fixture(scope="module")
def cases():
    return _cases()


@pytest.mark.parametrize("flags", [["-O2"], SAN], ids=["plain", "asan_ubsan"])
def test_task_head_forms_vs_bigints(cases, flags, tmp_path):
    cmds, checks = cases
    exe = str(tmp_path / "limb_curve29_head_check")
    subprocess.check_call(["g++"] + flags + ["-std=c++17", "-o", exe, SRC])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], input="\n".join(cmds) + "\n", capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.strip().split("\n")
    assert len(lines) == sum(n for _, n in checks), (len(lines), len(cmds))
    at = 0
    for (chk, n), cmd in zip(checks, cmds):
        try:
            chk(lines[at: at + n])
        except AssertionError as e:
            raise AssertionError(f"{cmd.split()[0]} case {checks.index((chk, n))}: {e}") from None
        at += n
