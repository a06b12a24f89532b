"""The host side of `DeviceMerkleSumTree.from_entries`, without a GPU: `pack_entries` (the four buffers of sg_mst_entries_dev),
what sg_mst_entries_dev refuses -- it validates before it touches the device, so every refusal is an SG_ERR_INVALID on any
machine --, and the arithmetic the kernels compile (csrc/keccak_f1600.h, csrc/mst_entries.h) built by the host compiler
into tests/cpp/mst_entries_check.cpp, under address / undefined sanitizers, against the oracle: pyref.keccak256,
oracle.fr_to_mont of Python integers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

from circuits_halo2_amd import ffi
from circuits_halo2_amd.merkle_sum_tree import pack_entries
from oracle import oracle as O
from oracle import pyref as P

R = P.R
SG_ERR_INVALID = -1
LENGTHS = [0, 1, 135, 136, 137, 271, 272, 273]          # around one and two blocks of the rate, 136


def mont(v: int) -> bytes:
    return O.fr_to_mont(np.frombuffer((v % R).to_bytes(32, "little"), dtype=np.uint8).copy()).tobytes()


# ============================================================================= pack_entries
def test_pack_entries_offsets_and_bytes():
    entries = [("", [0, 1 << 64]), ("dxGaEAii", [11888, 41163]), ("zoë€𝄞", [7, 0]), ("a", [10, 999])]
    name_bytes, name_off, digit_bytes, digit_off = pack_entries(entries, 2)
    assert name_off.dtype == np.uint64 and digit_off.dtype == np.uint64
    assert name_bytes.dtype == np.uint8 and digit_bytes.dtype == np.uint8
    utf8 = "zoë€𝄞".encode()
    assert len(utf8) == 2 + 2 + 3 + 4                       # one, two, three and four bytes per character
    assert name_off.tolist() == [0, 0, 8, 8 + len(utf8), 9 + len(utf8)]
    assert name_bytes.tobytes() == b"dxGaEAii" + utf8 + b"a"
    fields = [b"0", b"18446744073709551616", b"11888", b"41163", b"7", b"0", b"10", b"999"]
    assert digit_bytes.tobytes() == b"".join(fields)
    assert digit_off.tolist() == [0] + list(np.cumsum([len(f) for f in fields]))
    for i, (name, bal) in enumerate(entries):               # read back the way the kernels do
        assert name_bytes[int(name_off[i]):int(name_off[i + 1])].tobytes().decode() == name
        for c, b in enumerate(bal):
            j = 2 * i + c
            assert int(digit_bytes[int(digit_off[j]):int(digit_off[j + 1])].tobytes()) == b


def test_pack_entries_one_currency_and_only_empty_names():
    name_bytes, name_off, digit_bytes, digit_off = pack_entries([("", [5]), ("", [60])], 1)
    assert name_bytes.size == 0 and name_off.tolist() == [0, 0, 0]
    assert digit_bytes.tobytes() == b"560" and digit_off.tolist() == [0, 1, 3]


def test_pack_entries_errors():
    with pytest.raises(ValueError, match="^Invalid balance$"):
        pack_entries([("a", [1, 2]), ("b", [3, -1])], 2)
    with pytest.raises(ValueError, match="^entry with a wrong number of balances$"):
        pack_entries([("a", [1, 2]), ("b", [3])], 2)
    with pytest.raises(ValueError, match="^entry with a wrong number of balances$"):
        pack_entries([("a", [1, 2])], 3)


# ============================================================================= sg_mst_entries_dev: refusals
class Call:
    """the arguments of a good call for 3 entries of 2 currencies (6 fields); tests change one thing.  The output pointers
    are not memory: a call that is refused never gets as far as using them."""

    def __init__(self, names=(b"ab", b"", b"xyz"), fields=(b"1", b"22", b"333", b"4", b"55", b"0"), nc=2):
        self.n, self.nc, self.rows = len(names), nc, 4
        self.names, self.fields = list(names), list(fields)
        self.name_off = self.digit_off = None
        self.null = None

    def buffers(self):
        def packed(parts):
            data = np.frombuffer(b"".join(parts) + b"\0", dtype=np.uint8).copy()      # (never empty)
            off = np.zeros(len(parts) + 1, dtype=np.uint64)
            off[1:] = np.cumsum([len(p) for p in parts])
            return data, off
        nb, no = packed(self.names)
        db, do = packed(self.fields)
        return [nb, no if self.name_off is None else np.array(self.name_off, dtype=np.uint64),
                db, do if self.digit_off is None else np.array(self.digit_off, dtype=np.uint64)]

    def run(self):
        keep = self.buffers()
        args = [ffi.ptr(a) for a in keep] + [C.c_void_p(0x1000), C.c_void_p(0x2000)]
        if self.null is not None:
            args[self.null] = None
        L = ffi.lib()
        rc = L.sg_mst_entries_dev(args[0], args[1], args[2], args[3], C.c_size_t(self.n), C.c_size_t(self.rows), C.c_uint32(self.nc),
                                  args[4], args[5], None)
        return rc, L.sg_last_error().decode()


@pytest.mark.parametrize("which", range(6))
def test_refuses_each_null_pointer(which):
    c = Call()
    c.null = which
    rc, msg = c.run()
    assert rc == SG_ERR_INVALID and "null" in msg


def test_refuses_bad_sizes():
    for change in ({"n": 0}, {"rows": 2}, {"rows": 1 << 32}, {"nc": 0}, {"nc": 65}):
        c = Call()
        for k, v in change.items():
            setattr(c, k, v)
        rc, msg = c.run()
        assert rc == SG_ERR_INVALID and "bad size" in msg, change


def test_refuses_bad_offsets():
    c = Call()
    c.name_off = [1, 2, 2, 5]
    rc, msg = c.run()
    assert rc == SG_ERR_INVALID and "name_off[0]" in msg
    c = Call()
    c.name_off = [0, 2, 1, 5]
    rc, msg = c.run()
    assert rc == SG_ERR_INVALID and "name_off decreases at entry 1" in msg
    c = Call()
    c.digit_off = [1, 1, 3, 6, 7, 9, 10]
    rc, msg = c.run()
    assert rc == SG_ERR_INVALID and "digit_off[0]" in msg
    c = Call()
    c.digit_off = [0, 1, 3, 6, 5, 9, 10]
    rc, msg = c.run()
    assert rc == SG_ERR_INVALID and "digit_off decreases at field 3" in msg


BAD_FIELDS = ["", "12a", "-1", " 1", "1 ", "+1", "1.0", "１"]     # the last one is U+FF11, a full-width digit one


@pytest.mark.parametrize("bad", BAD_FIELDS)
@pytest.mark.parametrize("at", [0, 3, 5])
def test_refuses_a_bad_balance_field_and_names_it(bad, at):
    c = Call()
    c.fields[at] = bad.encode()
    rc, msg = c.run()
    assert rc == SG_ERR_INVALID and f"balance field {at} " in msg, msg
    assert ("is empty" in msg) == (bad == "")


def test_names_the_lowest_bad_field():
    c = Call()
    c.fields[4], c.fields[2] = b"x", b""
    rc, msg = c.run()
    assert rc == SG_ERR_INVALID and "balance field 2 is empty" in msg


# ============================================================================= the kernels' arithmetic on the host
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("mst_entries") / "mst_entries_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "circuits_halo2_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "mst_entries_check.cpp"), "-o", out])
    return out


def ask(exe, commands):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], input="\n".join(commands) + "\n", capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    return [ln.split() for ln in r.stdout.splitlines()]


def test_keccak256_of_the_block_edge_lengths(exe):
    msgs = [bytes((7 * j + n) & 0xff for j in range(n)) for n in LENGTHS]
    out = ask(exe, [f"k {n}" for n in LENGTHS])
    assert len(out) == 2 * len(LENGTHS)
    for i, m in enumerate(msgs):
        want = P.keccak256(m)
        assert out[2 * i] == ["digest", want.hex()], f"length {len(m)}"
        assert out[2 * i + 1] == ["username", mont(int.from_bytes(want, "big")).hex(), "fr_same=1"], f"length {len(m)}"


def test_keccak256_of_names(exe):
    names = ["", "dxGaEAii", "zoë€𝄞", "user0", "user40", "x" * 1000]
    out = ask(exe, ["m " + (n.encode().hex() or "-") for n in names])
    for i, n in enumerate(names):
        assert out[2 * i] == ["digest", P.keccak256(n.encode()).hex()], n[:20]
        assert out[2 * i + 1] == ["username", mont(P.mst_entry(n, [])[0]).hex(), "fr_same=1"], n[:20]


def test_big_endian_reduction_in_every_band(exe):
    """32 bytes as a big-endian integer: the ends of each of the six bands [q r, (q + 1) r) below 2^256"""
    values = [0, 1, (1 << 256) - 1]
    for q in range(6):
        values += [q * R, q * R + 1, min((q + 1) * R, 1 << 256) - 1]
    assert {v // R for v in values} == set(range(6))
    out = ask(exe, ["b " + v.to_bytes(32, "big").hex() for v in values])
    for v, got in zip(values, out):
        assert got == ["reduced", mont(v).hex(), "fr_same=1"], hex(v)


def test_decimal_strings(exe):
    values = [0, 7, (1 << 64) - 1, 1 << 64, R - 1, R, R + 1, 1 << 256, 10 ** 100, int("9" * 300)]
    texts = [str(v) for v in values] + ["00012", "0" * 40 + str(R + 5)]
    out = ask(exe, ["d " + t for t in texts])
    for t, got in zip(texts, out):
        assert got == ["decimal", mont(int(t)).hex()], t[:40]
