"""CPU-only checks of the batch verifier: the multipliers and the bisection of csrc/verify_batch_plan.h (no HIP: built with plain
g++ as tests/cpp/verify_batch_check.cpp and compared with restatements in Python), and the ABI of include/summa_verifier.h and of
sg_msm_g1_many_* -- exported, declared in the bindings, plain C, bad arguments refused, and no fallback without a GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import verify_batch_cases as VC

SG_ERR_INVALID, SG_ERR_NO_DEVICE = -1, -2


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("verify_batch") / "verify_batch_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "circuits_halo2_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "verify_batch_check.cpp"), "-o", exe])

    def run(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")[:-1]
        assert len(out) == len(lines)
        return out
    return run


# ------------------------------------------------------------------ multipliers
def _mult_line(digest, proofs, insts, entropy):
    hx = lambda b: bytes(b).hex() if len(b) else "-"
    parts = ["mult", int(digest).to_bytes(32, "big").hex(), hx(entropy) if entropy is not None else "-"]
    for p, inst in zip(proofs, insts):
        parts += [hx(p), hx(VC.instance_words(inst))]
    return " ".join(parts)


def test_multipliers_equal_the_python_restatement(plan_check):
    """seed and r_i for the three golden proofs, with and without entropy, against keccak256_python; every r_i is below 2^128 and
    not 0; two proofs swapped, another entropy or another key change EVERY r_i (they hang on the whole batch)"""
    _, vk = VC.reference_key()
    golden = VC.golden_proofs()
    proofs, insts = [p for p, _ in golden], [i for _, i in golden]
    entropy = bytes(range(1, 33))
    swapped = ([proofs[1], proofs[0], proofs[2]], [insts[1], insts[0], insts[2]])
    cases = [(vk.transcript_repr, proofs, insts, None), (vk.transcript_repr, proofs, insts, entropy),
             (vk.transcript_repr, *swapped, None), (vk.transcript_repr, *swapped, entropy),
             (vk.transcript_repr + 1, proofs, insts, None), (vk.transcript_repr, proofs[:1], insts[:1], None),
             (vk.transcript_repr, [b"", proofs[0][:-1]], [[], insts[0][:3]], None)]
    out = plan_check([_mult_line(*c) for c in cases])
    rs = []
    for case, line in zip(cases, out):
        seed, want = VC.multipliers(*case)
        got = line.split()
        assert got[0] == seed.hex()
        r = [int.from_bytes(bytes.fromhex(h), "little") for h in got[1:]]
        assert r == want and len(r) == len(case[1])
        assert all(0 < v < 1 << 128 for v in r)
        rs.append(r)
    plain, with_entropy, swapped_plain, swapped_entropy, other_key = rs[:5]
    for a, b in ((plain, with_entropy), (plain, swapped_plain), (with_entropy, swapped_entropy), (plain, other_key)):
        assert all(x != y for x, y in zip(a, b))


# ------------------------------------------------------------------ bisection
def _bad_sets(n):
    sets = [set(), {0}, {n - 1}, {n // 2 - 1, n // 2} if n >= 2 else {0}, set(range(n))]
    return [s for i, s in enumerate(sets) if s not in sets[:i]]


@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 1000])
def test_bisection_finds_exactly_the_bad_proofs(plan_check, n):
    """verdicts = the bad set; one check for a batch without a bad proof, at most 1 + 2 |bad| ceil(log2 n) otherwise; never more
    than two ranges in one call (the halves of a rejected range); proofs the host part rejected (empty jobs) stay rejected and cost
    nothing"""
    ids = lambda s: ",".join(str(i) for i in sorted(s)) or "-"
    cases = [(set(), bad) for bad in _bad_sets(n)]
    if n >= 3:
        dead = {0, n // 2, n - 1}
        cases += [(dead, set()), (dead, {1}), (dead, set(range(n))), (set(range(n)), set())]
    out = plan_check([f"bisect honest {n} {ids(dead)} {ids(bad)}" for dead, bad in cases])
    for (dead, bad), line in zip(cases, out):
        verdicts, checks, calls, most = line.split()
        want = "".join("0" if (i in bad or i in dead) else "1" for i in range(n))
        assert verdicts == want, (n, dead, bad)
        live_bad = len(bad - dead)
        if len(dead) == n:
            assert int(checks) == 0 and int(calls) == 0
            continue
        assert int(checks) <= VC.pairing_bound(n, live_bad), (n, dead, bad, checks)
        if not live_bad:
            assert int(checks) == 1 and int(calls) == 1
        assert int(calls) <= int(checks) and int(most) <= 2


@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 1000])
def test_bisection_ends_when_accepts_lies(plan_check, n):
    """the whole batch rejected, every other range accepted: no loop -- every proof is accepted by its own check at the latest
    (for n = 1 the whole batch IS the proof's own check, and it said no)"""
    verdicts, checks, calls, _ = plan_check([f"bisect liar {n} - -"])[0].split()
    assert verdicts == ("0" if n == 1 else "1" * n)
    assert int(checks) <= VC.pairing_bound(n, 1) and int(calls) <= int(checks)


# ------------------------------------------------------------------ ABI
def _declared(header, prefix):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(" + prefix + r"[a-z0-9_]+)\s*\(", hdr)))


def test_new_symbols_are_exported_declared_and_plain_c():
    from circuits_halo2_amd import ffi
    L = C.CDLL(ffi.library_path())
    many = ["sg_msm_g1_many_begin", "sg_msm_g1_many_sums", "sg_msm_g1_many_end"]
    assert set(many) <= set(ffi.EXPORTS) and set(many) <= set(_declared("summa_gpu.h", "sg_"))
    assert _declared("summa_verifier.h", "sv_") == sorted(ffi.VERIFIER_EXPORTS) == ["sv_last_error", "sv_verify_batch"]
    for name in many + ffi.VERIFIER_EXPORTS:
        assert hasattr(L, name), name
    assert ffi.verifier_lib().sv_last_error() == b""
    rust = open(os.path.join(ROOT, "integration", "halo2_gpu_shim", "src", "lib.rs")).read()
    for name in many + ffi.VERIFIER_EXPORTS:
        assert re.search(r"pub fn " + name + r"\s*\(", rust), name
    if shutil.which("gcc"):
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c",
                               os.path.join(ROOT, "include", "summa_verifier.h")])


def _u32(values):
    return np.array(values, dtype=np.uint32)


def test_many_rejects_bad_arguments():
    """what needs no device to refuse: null pointers, a `first` that decreases, a job above 64 points, more than 2^14 jobs, more
    than 8 ranges, a range that ends before it starts"""
    from circuits_halo2_amd import ffi
    L = ffi.lib()
    sc, bs = np.zeros(32 * 130, dtype=np.uint8), np.zeros(64 * 130, dtype=np.uint8)
    h = C.c_uint64(0)
    begin = lambda first, jobs, s=sc, b=bs, hp=C.byref(h): L.sg_msm_g1_many_begin(ffi.ptr(s) if s is not None else None,
                                                                                  ffi.ptr(b) if b is not None else None,
                                                                                  ffi.ptr(_u32(first)) if first is not None else None, C.c_uint32(jobs), hp)
    assert begin(None, 1) == SG_ERR_INVALID
    assert begin([0, 1], 1, hp=None) == SG_ERR_INVALID
    assert begin([0, 1], 1, s=None) == SG_ERR_INVALID and begin([0, 1], 1, b=None) == SG_ERR_INVALID
    assert begin([0, 5, 4], 2) == SG_ERR_INVALID
    assert begin([0, 65], 1) == SG_ERR_INVALID and begin([0, 64, 129], 2) == SG_ERR_INVALID
    assert b"64 points" in L.sg_last_error()
    assert begin([0] * ((1 << 14) + 2), (1 << 14) + 1) == SG_ERR_INVALID
    out = np.zeros(64 * 9, dtype=np.uint8)
    sums = lambda ranges, count: L.sg_msm_g1_many_sums(C.c_uint64(12345), ffi.ptr(_u32(ranges)), C.c_uint32(count), ffi.ptr(out))
    assert sums([0, 0] * 9, 9) == SG_ERR_INVALID
    assert sums([2, 1], 1) == SG_ERR_INVALID
    assert L.sg_msm_g1_many_sums(C.c_uint64(12345), None, C.c_uint32(1), ffi.ptr(out)) == SG_ERR_INVALID
    assert L.sg_msm_g1_many_sums(C.c_uint64(12345), ffi.ptr(_u32([0, 0])), C.c_uint32(1), None) == SG_ERR_INVALID


def _batch_args(n, flavour=0):
    from circuits_halo2_amd import ffi, verifier as V
    params, vk = VC.reference_key()
    digest, fixed, perm, g2, s_g2 = V._native_key(params, vk)
    proofs, insts = VC.cycled(n)
    raws = [np.frombuffer(p, dtype=np.uint8).copy() for p in proofs]
    words = [np.frombuffer(VC.instance_words(i), dtype=np.uint8).copy() for i in insts]
    keep = (digest, fixed, perm, g2, s_g2, raws, words)
    args = [C.c_uint32(vk.k), C.c_uint32(vk.n_currencies), ffi.ptr(digest), ffi.ptr(fixed), ffi.ptr(perm), ffi.ptr(g2), ffi.ptr(s_g2),
            (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in raws]), (C.c_size_t * max(n, 1))(*[len(p) for p in proofs]),
            (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in words]), (C.c_uint32 * max(n, 1))(*[len(i) for i in insts]),
            C.c_uint32(n), C.c_int(flavour), None]
    return keep, args


def test_verify_batch_rejects_bad_arguments():
    """no proofs: SG_OK and nothing written; more than 8192, a null pointer, an unknown transcript, k out of range: SG_ERR_INVALID"""
    from circuits_halo2_amd import ffi
    L = ffi.verifier_lib()
    accepted = np.full(4, 7, dtype=np.uint8)
    pairings = C.c_uint32(99)
    keep, args = _batch_args(3)
    call = lambda a: L.sv_verify_batch(*a, ffi.ptr(accepted), C.byref(pairings))
    zero = list(args)
    zero[11] = C.c_uint32(0)
    assert call(zero) == 0 and (accepted == 7).all() and pairings.value == 99
    for pos, value in ((11, C.c_uint32(8193)), (12, C.c_int(2)), (0, C.c_uint32(3)), (0, C.c_uint32(26)), (1, C.c_uint32(0)), (2, None),
                       (7, None), (8, None), (9, None), (10, None)):
        bad = list(args)
        bad[pos] = value
        assert call(bad) == SG_ERR_INVALID, pos
        assert L.sv_last_error().startswith(b"sv_verify_batch: ")
    assert L.sv_verify_batch(*args, None, C.byref(pairings)) == SG_ERR_INVALID
    assert (accepted == 7).all()
    del keep


def test_no_gpu_means_no_device_and_no_fallback():
    """without a GPU every call that would need one fails with SG_ERR_NO_DEVICE: nothing is computed on the host instead"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from circuits_halo2_amd import arithmetic as A, ffi, verifier as V
    L = ffi.verifier_lib()
    assert L.sg_device_count() == 0
    sc, bs = np.zeros(32 * 3, dtype=np.uint8), np.zeros(64 * 3, dtype=np.uint8)
    h = C.c_uint64(0)
    assert L.sg_msm_g1_many_begin(ffi.ptr(sc), ffi.ptr(bs), ffi.ptr(_u32([0, 1, 3])), C.c_uint32(2), C.byref(h)) == SG_ERR_NO_DEVICE
    assert L.sg_msm_g1_many_begin(ffi.ptr(sc), ffi.ptr(bs), ffi.ptr(_u32([0])), C.c_uint32(0), C.byref(h)) == SG_ERR_NO_DEVICE
    out = np.zeros(64, dtype=np.uint8)
    assert L.sg_msm_g1_many_sums(C.c_uint64(1), ffi.ptr(_u32([0, 0])), C.c_uint32(1), ffi.ptr(out)) == SG_ERR_NO_DEVICE
    assert L.sg_msm_g1_many_end(C.c_uint64(1)) == SG_ERR_NO_DEVICE
    with pytest.raises(ffi.SummaGpuError) as e:
        A.MultiexpMany([(sc, bs)])
    assert e.value.code == SG_ERR_NO_DEVICE
    accepted = np.full(3, 7, dtype=np.uint8)
    keep, args = _batch_args(3)
    assert L.sv_verify_batch(*args, ffi.ptr(accepted), None) == SG_ERR_NO_DEVICE
    assert not accepted.any() and b"no HIP device" in L.sv_last_error()
    params, vk = VC.reference_key()
    proofs, insts = VC.cycled(3)
    with pytest.raises(ffi.SummaGpuError) as e:
        V.verify_batch(params, vk, proofs, insts)
    assert e.value.code == SG_ERR_NO_DEVICE
    # a batch whose every proof the host part rejects still has to reach the device: the verdict never comes from a shortcut
    with pytest.raises(ffi.SummaGpuError):
        V.verify_batch(params, vk, [p[:-1] for p in proofs], insts)
    assert V.verify_batch(params, vk, [], []) == []
    del keep
