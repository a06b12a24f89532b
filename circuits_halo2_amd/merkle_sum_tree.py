"""Host mirror of `zk_prover/src/merkle_sum_tree` (mst.rs:74-134, entry.rs:15-27,
utils/csv_parser.rs, utils/operation_helpers.rs:10-12) with the hashing on the GPU
(C ABI: sg_mst_leaves_dev / sg_mst_level_dev / sg_mst_build_dev).

Host logic kept here: CSV parsing, keccak256(username) -> field element, decimal balances ->
field elements, zero-entry padding to 2^depth, Merkle-proof extraction (tree.rs:85-137).
DeviceMerkleSumTree.from_entries leaves only the CSV parsing here: names and decimal balances
become field elements on the device (sg_mst_entries_dev) and the tree stays in HBM; DeviceMerkleSumTree.from_csv leaves the
header line here and reads the rest of the file on the device too (sg_mst_csv_scan_dev / sg_mst_csv_entries_dev), unless the
file is outside the device reader's subset of CSV text; DeviceMerkleSumTree.from_csv_sorted does the same and sorts the names
there as well (ss_mst_csv_entries_sorted_dev), and such a tree finds a user by name on the device (ss_mst_find_names);
DeviceMerkleSumTree.from_csv(name_index=True) sorts the names beside leaves that stay in file order (ss_mst_csv_name_index_dev,
ss_mst_find_leaves), and `duplicate_names` reports the usernames that occur more than once (ss_mst_duplicate_names_dev);
DeviceMerkleSumTree.update_leaf /
update_leaves / update_leaves_at change balances there in place (sg_mst_update_dev).
"""
from __future__ import annotations

import csv
import ctypes as C

import numpy as np

from . import ffi
from .utils import R_MODULUS

_KECCAK_RC = [0x0000000000000001, 0x0000000000008082, 0x800000000000808A, 0x8000000080008000, 0x000000000000808B,
              0x0000000080000001, 0x8000000080008081, 0x8000000000008009, 0x000000000000008A, 0x0000000000000088,
              0x0000000080008009, 0x000000008000000A, 0x000000008000808B, 0x800000000000008B, 0x8000000000008089,
              0x8000000000008003, 0x8000000000008002, 0x8000000000000080, 0x000000000000800A, 0x800000008000000A,
              0x8000000080008081, 0x8000000000008080, 0x0000000080000001, 0x8000000080008008]
_KECCAK_ROT = [0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14]
_M64 = (1 << 64) - 1


def keccak256(data: bytes) -> bytes:
    """Keccak-256 as Ethereum uses it (`ethers::utils::keccak256`, entry.rs:21): the library's host routine
    (sg_keccak256; the EVM transcript hashes a few KiB per proof)"""
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    out = np.zeros(32, dtype=np.uint8)
    ffi.check(ffi.lib().sg_keccak256(ffi.ptr(buf) if buf.size else None, C.c_size_t(buf.size), ffi.ptr(out)))
    return out.tobytes()


def keccak256_python(data: bytes) -> bytes:
    """the same with Python integers (lanes indexed x + 5y): the independent twin the library routine is checked against"""
    rate = 136
    msg = bytearray(data) + b"\x01"
    msg += bytes(-len(msg) % rate)
    msg[-1] |= 0x80
    st = [0] * 25
    for off in range(0, len(msg), rate):
        for i in range(rate // 8):
            st[i] ^= int.from_bytes(msg[off + 8 * i:off + 8 * i + 8], "little")
        for rc in _KECCAK_RC:
            c = [st[x] ^ st[x + 5] ^ st[x + 10] ^ st[x + 15] ^ st[x + 20] for x in range(5)]
            for x in range(5):
                d = c[(x + 4) % 5] ^ (((c[(x + 1) % 5] << 1) | (c[(x + 1) % 5] >> 63)) & _M64)
                for y in range(0, 25, 5):
                    st[x + y] ^= d
            b = [0] * 25
            for x in range(5):
                for y in range(5):
                    v, r = st[x + 5 * y], _KECCAK_ROT[x + 5 * y]
                    b[y + 5 * ((2 * x + 3 * y) % 5)] = ((v << r) | (v >> (64 - r))) & _M64 if r else v
            for y in range(0, 25, 5):
                for x in range(5):
                    st[x + y] = b[x + y] ^ ((~b[(x + 1) % 5 + y]) & b[(x + 2) % 5 + y])
            st[0] ^= rc
    return b"".join(v.to_bytes(8, "little") for v in st[:4])


def _to_fr_bytes(v: int) -> bytes:
    return ((v % R_MODULUS) << 256).__mod__(R_MODULUS).to_bytes(32, "little")


def big_intify_username(username: str) -> int:
    """utils/operation_helpers.rs:5-8: keccak256 of the username bytes as a big-endian integer"""
    return int.from_bytes(keccak256(username.encode()), "big")


def big_uint_to_fp(big_uint: int) -> bytes:
    """utils/operation_helpers.rs:10-12 (`Fp::from_str_vartime` of the decimal string): the integer reduced modulo r, in
    halo2curves' memory form (32 bytes, Montgomery, little-endian) -- what every `_dev` entry point takes"""
    if big_uint < 0:
        raise ValueError("Invalid balance")
    return _to_fr_bytes(big_uint)


_R_INV = pow(1 << 256, -1, R_MODULUS)


def _mont_to_int(row) -> int:
    """32 bytes in memory form (Montgomery, little-endian) -> the integer they stand for"""
    return int.from_bytes(bytes(row), "little") * _R_INV % R_MODULUS


def fp_to_big_uint(f) -> int:
    """utils/operation_helpers.rs:15-17: the canonical integer of a field element given in memory form"""
    if int.from_bytes(bytes(f), "little") >= R_MODULUS:
        raise ValueError("not a field element")
    return _mont_to_int(f)


def _level_first(depth: int, level: int) -> int:
    """the first node of `level` in the level-major node arrays of a tree of 2^depth leaves (the leaves, the 2^(depth - 1)
    parents, .., the root): mst_level_first of csrc/mst_update_plan.h"""
    return (2 << depth) - (2 << (depth - level))


def _check_balance_rows(rows, n_currencies: int, wrong_count: str):
    """what every front end asks of `rows`, a list of balance rows, in this order: n_currencies balances in each (else
    ValueError(wrong_count)), none negative"""
    if set(map(len, rows)) - {n_currencies}:
        raise ValueError(wrong_count)
    if rows and n_currencies and min(map(min, rows)) < 0:
        raise ValueError("Invalid balance")


def parse_csv_to_entries(path: str, n_currencies: int):
    """utils/csv_parser.rs: header `username,balance_<name>_<chain>,...`; one balance per
    currency column; raises if the column count differs from n_currencies (the reference's
    `try_into().unwrap()` panics there)."""
    with open(path, newline="") as f:
        first = f.readline()
    delim = ";" if ";" in first else ","
    with open(path, newline="") as f:
        rows = list(csv.reader(f, delimiter=delim))
    header, body = rows[0], rows[1:]
    if len(header) - 1 != n_currencies:
        raise ValueError(f"csv has {len(header) - 1} balance columns, N_CURRENCIES = {n_currencies}")
    cryptocurrencies = []
    for h in header[1:]:            # csv_parser.rs:17-31: `balance_<name>_<chain>`, anything else is an error
        parts = h.split("_")
        if len(parts) != 3 or parts[0] != "balance":
            raise ValueError(f"Invalid header: {h}")
        cryptocurrencies.append((parts[1], parts[2]))
    if header[0] != "username":
        raise ValueError("Username not found")
    def balance(text: str) -> int:
        # BigUint::parse_bytes(.., 10): decimal digits only -- no sign, blanks or underscores (csv_parser.rs:45-50)
        if not text or not text.isascii() or not text.isdigit():
            raise ValueError("Invalid balance")
        return int(text)
    entries = [(r[0], [balance(x) for x in r[1:1 + n_currencies]]) for r in body if r]
    return entries, cryptocurrencies


def _hash_batch(kind: str, *arrays, n: int, nc: int):
    """one device call over n nodes: kind 'leaf' (usernames, balances) -> hashes; 'middle' (child hashes, child
    balances of 2n children) -> (hashes, balances)"""
    import torch
    L = ffi.lib()
    dev = [torch.from_numpy(np.array(a, dtype=np.uint8, copy=True)).cuda() for a in arrays]
    h = torch.empty(32 * n, dtype=torch.uint8, device="cuda")
    if kind == "leaf":
        ffi.check(L.sg_mst_leaves_dev(ffi.dev_ptr(dev[0]), ffi.dev_ptr(dev[1]), C.c_size_t(n), C.c_uint32(nc), ffi.dev_ptr(h),
                                      ffi.current_stream_ptr()))
        return h.cpu().numpy()
    b = torch.empty(32 * n * nc, dtype=torch.uint8, device="cuda")
    ffi.check(L.sg_mst_level_dev(ffi.dev_ptr(dev[0]), ffi.dev_ptr(dev[1]), C.c_size_t(n), C.c_uint32(nc), ffi.dev_ptr(h),
                                 ffi.dev_ptr(b), ffi.current_stream_ptr()))
    return h.cpu().numpy(), b.cpu().numpy()


def _build_nodes(d_users, d_bals, depth: int, n_currencies: int):
    """sg_mst_build_dev on the current stream over 2^depth leaves on the device: the level-major node hashes and node
    balances, allocated here.  Nothing is waited for."""
    import torch
    nodes = (2 << depth) - 1
    d_h = torch.empty(32 * nodes, dtype=torch.uint8, device="cuda")
    d_b = torch.empty(32 * nodes * n_currencies, dtype=torch.uint8, device="cuda")
    ffi.check(ffi.lib().sg_mst_build_dev(ffi.dev_ptr(d_users), ffi.dev_ptr(d_bals), C.c_uint32(depth), C.c_uint32(n_currencies),
                                         ffi.dev_ptr(d_h), ffi.dev_ptr(d_b), ffi.current_stream_ptr()))
    return d_h, d_b


class DuplicateNames:
    """What `duplicate_names` found: the usernames that occur more than once in the snapshot.  The reference accepts such a file
    silently (mst.rs:103-134) and `index_of_username` finds the first row of a name only (mst.rs:207-223), so every later row
    of that name is *shadowed*: a leaf that no lookup, `update_leaf` or `prove_batch` by name can reach, whose balances still sit
    in the committed sums.
      n_repeated_names   names that occur more than once
      n_shadowed         shadowed leaves: the rows of those names but each one's first
      shadowed           numpy.uint32: the shadowed leaves ordered by the names' bytes and, within a name, by file row (with a
                         `cap`, the first `cap` of them)
      first              numpy.uint32: beside each listed leaf the one that a lookup of its name finds
      ok                 no name occurs twice"""

    def __init__(self, n_repeated_names, n_shadowed, shadowed, first):
        self.n_repeated_names, self.n_shadowed = int(n_repeated_names), int(n_shadowed)
        self.shadowed, self.first = np.asarray(shadowed, dtype=np.uint32), np.asarray(first, dtype=np.uint32)

    @property
    def ok(self) -> bool:
        return self.n_shadowed == 0

    def groups(self):
        """{first leaf: [its shadowed leaves]} of the listed leaves, in the list's order"""
        out = {}
        for leaf, head in zip(self.shadowed.tolist(), self.first.tolist()):
            out.setdefault(head, []).append(leaf)
        return out


class SnapshotDiff:
    """What `diff_csv` / `diff_entries` found: the next round's file B joined by username with the tree T as it was
    (include/summa_rounds.h has the rules).  A row of B is looked up as `index_of_username` looks a name up, so it finds the first
    leaf of its name; of several rows that find one leaf the first in file order owns it.  Balances compare as field elements: 007
    equals 7, and an integer >= r equals its residue.
      n_new, n_shadowed_rows, n_changed, n_same   the rows of B: not found in T; behind another row of the same name; the owner of a
                         leaf with a balance that differs; the owner of a leaf with none
      n_gone             named leaves of T that no row of B found
      n_unreachable      leaves of T behind another of the same name (`duplicate_names`): no row can own them, they are neither
                         changed nor gone
      changed            numpy.uint32: the changed leaves in increasing order, all of them
      new_rows, gone     numpy.uint32: the new rows of B and the gone leaves of T in increasing order (with a `cap`, the first `cap`)
      ok                 nobody changed, nobody is new, nobody is gone
      ingest, fallback_reason   "device" (both texts were joined in HBM, sr_mst_csv_diff_dev) or "host" (from `entries`), and why
      row_leaf(), row_state(), leaf_state(), owner()   the arrays as numpy (on the device way they stay in HBM until asked for): per
                         row its leaf or 0xFFFFFFFF and its state (ROW_*), per leaf of all 2^depth its state (LEAF_*) and owner row
      admitted           the range of leaves the NEW rows go to under `apply_diff(admit_new=True)`: the j-th new row becomes leaf
                         n_tree + j.  A round fits while admitted.stop <= 2^depth (`tree.free_leaves` >= n_new)
    A diff is of the tree as it was: `apply_diff` refuses it after another update.  A plain apply writes the changed balances alone:
    new users are not inserted and gone users are not zeroed unless `apply_diff` is asked to (`admit_new`, `zero_gone`), which
    settles the round in place.  A rebuild is still due when the new users no longer fit the padding (the depth has to grow), when
    the tree is sorted or holds no name index, and to drop the zeroed rows of gone users for good."""

    LEAF_PADDING, LEAF_SAME, LEAF_CHANGED, LEAF_GONE, LEAF_UNREACHABLE = 0, 1, 2, 3, 4
    ROW_SAME, ROW_CHANGED, ROW_NEW, ROW_SHADOWED = 1, 2, 3, 4
    ABSENT = 0xFFFFFFFF

    def __init__(self, counts, changed, new_rows, gone, arrays, ingest, fallback_reason=None, new_balances=None, dev=None):
        (self.n_new, self.n_shadowed_rows, self.n_changed, self.n_same, self.n_gone, self.n_unreachable) = (int(x) for x in counts)
        self.changed, self.new_rows, self.gone = (np.asarray(a, dtype=np.uint32) for a in (changed, new_rows, gone))
        self._arrays = arrays                  # {"row_leaf", "row_state", "leaf_state", "owner"}: numpy arrays or device tensors
        self.ingest, self.fallback_reason = ingest, fallback_reason
        self.new_balances = new_balances       # the host way: the owner row's balances for every changed leaf, in the list's order
        self._dev = dev                        # the device way: what sr_mst_apply_diff_dev takes
        self._tree, self._epoch, self._n_tree = None, None, None

    @property
    def ok(self) -> bool:
        return self.n_new == self.n_changed == self.n_gone == 0

    @property
    def admitted(self) -> range:
        return range(self._n_tree, self._n_tree + self.n_new)

    def summary(self):
        return {"new": self.n_new, "shadowed": self.n_shadowed_rows, "changed": self.n_changed, "same": self.n_same, "gone": self.n_gone,
                "unreachable": self.n_unreachable, "new_listed": len(self.new_rows), "gone_listed": len(self.gone)}

    def _array(self, key, dtype):
        a = self._arrays[key]
        return (a if isinstance(a, np.ndarray) else a.cpu().numpy()).view(dtype)

    def row_leaf(self) -> np.ndarray:
        return self._array("row_leaf", np.uint32)

    def row_state(self) -> np.ndarray:
        return self._array("row_state", np.uint8)

    def leaf_state(self) -> np.ndarray:
        return self._array("leaf_state", np.uint8)

    def owner(self) -> np.ndarray:
        return self._array("owner", np.uint32)


class CsvExport:
    """What `to_csv` wrote: `n_rows` rows and `size` bytes, the header line included; `ingest` says which way the text was made,
    "device" (sx_mst_csv_measure_dev / sx_mst_csv_write_dev over the tree's text and balances in HBM) or "host" (from `entries`),
    and `fallback_reason` why the host's."""

    def __init__(self, n_rows, size, ingest, fallback_reason=None):
        self.n_rows, self.size, self.ingest, self.fallback_reason = int(n_rows), int(size), ingest, fallback_reason

    def __repr__(self):
        return f"CsvExport(n_rows={self.n_rows}, size={self.size}, ingest={self.ingest!r}, fallback_reason={self.fallback_reason!r})"


def _csv_delimiter(delimiter) -> str:
    """one byte the reader takes as a delimiter (mst_diff_problem's rule): ASCII, no digit, quote, line end or NUL"""
    if not isinstance(delimiter, str) or len(delimiter) != 1 or not delimiter.isascii() or delimiter in '"\r\n\0' or delimiter.isdigit():
        raise ValueError("a delimiter the reader does not take")
    return delimiter


def _csv_header(cryptocurrencies, n_currencies: int, delimiter: str) -> str:
    """`username`, then for every (name, chain) the delimiter and balance_<name>_<chain>, then the line end"""
    crypto = [tuple(c) for c in cryptocurrencies or ()]
    if not crypto:
        raise ValueError("the tree has no cryptocurrency names and none are given")
    if len(crypto) != n_currencies or any(len(c) != 2 for c in crypto):
        raise ValueError("n_currencies (name, chain) pairs expected")
    return delimiter.join(["username"] + [f"balance_{name}_{chain}" for name, chain in crypto]) + "\n"


class _Tree:
    """What MerkleSumTree and DeviceMerkleSumTree share: everything that needs only `depth`, `n_currencies`, `entries` (None
    where a tree holds none), `is_sorted` and the class's `from_entries`."""

    def to_csv(self, path: str, cryptocurrencies=None, delimiter=None) -> CsvExport:
        """The snapshot CSV this tree commits to, from `entries` on the host, in the device reader's subset of CSV text: the header
        line `username,balance_<name>_<chain>,..` of `cryptocurrencies` (default: the tree's own), then one row per named entry in
        leaf order -- the name, then for each currency the delimiter (default ",") and the balance, then "\\n".  A balance is the
        canonical integer in [0, r) of the leaf's field element in decimal: 007 comes out as 7, an integer >= r as its residue.
        Padding entries (no name) are not written; duplicate names are written as they stand.  `from_csv` of the file has this
        tree's root, and `from_csv_sorted` that of a sorted tree -- unless a padding leaf was given non-zero balances by
        `update_leaves_at`: such a leaf has no name and is not written.
        ValueError: a tree without cryptocurrency names when none are given; a tree that holds no entries (built from field
        elements); a name with the delimiter, a quote, a line end, NUL or a non-ASCII byte in it, which would not read back as
        the same snapshot."""
        delim = _csv_delimiter("," if delimiter is None else delimiter)
        header = _csv_header(cryptocurrencies or self.cryptocurrencies, self.n_currencies, delim)
        if self.entries is None:
            raise ValueError("a tree built from field elements holds no entries")
        rows = []
        for name, bal in self.entries:
            if name is None:
                continue
            if not isinstance(name, str) or not name.isascii() or any(c in name for c in (delim, '"', "\r", "\n", "\0")):
                raise ValueError(f"username {name!r} would not read back: the delimiter, a quote, a line end, NUL or a non-ASCII byte")
            rows.append(delim.join([name] + [str(int(v) % R_MODULUS) for v in bal]))
        text = (header + "".join(row + "\n" for row in rows)).encode()
        with open(path, "wb") as f:
            f.write(text)
        return CsvExport(len(rows), len(text), "host")

    @classmethod
    def from_csv(cls, path: str, n_currencies: int, n_bytes: int = 8):
        entries, crypto = parse_csv_to_entries(path, n_currencies)
        t = cls.from_entries(entries, n_currencies, n_bytes)
        t.cryptocurrencies = crypto
        return t

    @classmethod
    def from_csv_sorted(cls, path: str, n_currencies: int, n_bytes: int = 8):
        """mst.rs:89-100: leaves sorted by the username byte values"""
        entries, crypto = parse_csv_to_entries(path, n_currencies)
        entries.sort(key=lambda e: e[0].encode())
        t = cls.from_entries(entries, n_currencies, n_bytes, is_sorted=True)
        t.cryptocurrencies = crypto
        return t

    @staticmethod
    def _entry_fields(name, bal):
        """(username field element, balance field elements) as Montgomery bytes; the zero entry is ("0", 0...)
        with username field element 0 (entry.rs:30-38).  A username may also be its field element, an int (the proofs of a
        tree without entries)."""
        u = name if isinstance(name, int) else 0 if name is None else big_intify_username(name)
        return _to_fr_bytes(u), b"".join(_to_fr_bytes(v) for v in bal)

    def get_entry(self, index: int):
        if self.entries is None:
            raise ValueError("a tree built from field elements holds no entries")
        return self.entries[index]

    def index_of_username(self, username: str) -> int:
        """mst.rs:207-223: linear scan, or binary search when the tree was built sorted"""
        if self.entries is None:
            raise KeyError("Username not found")
        if self.is_sorted:
            real = [e for e in self.entries if e[0] is not None]
            lo, hi = 0, len(real)
            key = username.encode()
            while lo < hi:
                mid = (lo + hi) // 2
                if real[mid][0].encode() < key:
                    lo = mid + 1
                else:
                    hi = mid
            if lo < len(real) and real[lo][0] == username:
                return lo
            raise KeyError("Username not found")
        for i, (name, _) in enumerate(self.entries):
            if name == username:
                return i
        raise KeyError("Username not found")

    def duplicate_names(self, cap=None) -> DuplicateNames:
        """The usernames that occur more than once, from `entries` on the host: the leaves in the stable order of their names'
        bytes, where a repeated name is a run and every leaf of a run but its first is shadowed.  cap: list at most that many
        shadowed leaves (None: all).  Zero entries (the padding) carry no name and are not counted."""
        if cap is not None and cap < 0:
            raise ValueError("cap below 0")
        if self.entries is None:
            raise ValueError("a tree built from field elements holds no entries")
        names = [(e[0].encode(), i) for i, e in enumerate(self.entries) if isinstance(e[0], str)]
        names.sort(key=lambda pair: pair[0])                  # stable: equal names keep the leaves' order
        shadowed, first, repeated = [], [], 0
        for at in range(1, len(names)):
            if names[at][0] != names[at - 1][0]:
                continue
            if not shadowed or shadowed[-1] != names[at - 1][1]:
                repeated += 1
                head = names[at - 1][1]
            shadowed.append(names[at][1])
            first.append(head)
        listed = len(shadowed) if cap is None else min(int(cap), len(shadowed))
        return DuplicateNames(repeated, len(shadowed), shadowed[:listed], first[:listed])

    _updates = 0              # how many times the balances changed: a diff is of the tree as it was

    def diff_entries(self, entries, cap=None) -> SnapshotDiff:
        """The next round's entries [(username, [balances])] against this tree, from `entries` on the host (SnapshotDiff has the
        rules).  cap: list at most that many new rows and gone leaves (None: all)."""
        if cap is not None and cap < 0:
            raise ValueError("cap below 0")
        if self.entries is None:
            raise ValueError("a tree built from field elements holds no entries")
        entries = list(entries)
        _check_balance_rows([bal for _, bal in entries], self.n_currencies, "wrong number of balances")
        D = SnapshotDiff
        first = {}
        for leaf, (name, _) in enumerate(self.entries):
            if isinstance(name, str):
                first.setdefault(name, leaf)
        leaves = 1 << self.depth
        row_leaf = np.array([first.get(name, D.ABSENT) for name, _ in entries], dtype=np.uint32)
        owner = np.full(leaves, D.ABSENT, dtype=np.uint32)
        for row in range(len(entries) - 1, -1, -1):           # the lowest row is written last
            if row_leaf[row] != D.ABSENT:
                owner[row_leaf[row]] = row
        row_state = np.full(len(entries), D.ROW_NEW, dtype=np.uint8)
        leaf_state = np.full(leaves, D.LEAF_PADDING, dtype=np.uint8)
        for row, leaf in enumerate(row_leaf.tolist()):
            if leaf == D.ABSENT:
                continue
            if owner[leaf] != row:
                row_state[row] = D.ROW_SHADOWED
                continue
            same = [v % R_MODULUS for v in entries[row][1]] == [v % R_MODULUS for v in self.entries[leaf][1]]
            row_state[row], leaf_state[leaf] = (D.ROW_SAME, D.LEAF_SAME) if same else (D.ROW_CHANGED, D.LEAF_CHANGED)
        n_named = 0
        for leaf, (name, _) in enumerate(self.entries):
            if isinstance(name, str):
                n_named += 1
                if first[name] != leaf:
                    leaf_state[leaf] = D.LEAF_UNREACHABLE
                elif owner[leaf] == D.ABSENT:
                    leaf_state[leaf] = D.LEAF_GONE
        changed, gone = np.flatnonzero(leaf_state == D.LEAF_CHANGED), np.flatnonzero(leaf_state == D.LEAF_GONE)
        new_rows = np.flatnonzero(row_state == D.ROW_NEW)
        counts = [new_rows.size, int((row_state == D.ROW_SHADOWED).sum()), changed.size, int((row_state == D.ROW_SAME).sum()), gone.size,
                  int((leaf_state == D.LEAF_UNREACHABLE).sum())]
        listed = None if cap is None else int(cap)
        diff = SnapshotDiff(counts, changed, new_rows[:listed], gone[:listed],
                            {"row_leaf": row_leaf, "row_state": row_state, "leaf_state": leaf_state, "owner": owner}, "host",
                            new_balances=[list(entries[owner[leaf]][1]) for leaf in changed.tolist()])
        diff._tree, diff._epoch, diff._n_tree = self, self._updates, n_named
        return diff

    @property
    def free_leaves(self) -> int:
        """2^depth less the named leaves: how many new users `apply_diff(admit_new=True)` can still admit before the depth has to
        grow"""
        if self.entries is None:
            raise ValueError("a tree built from field elements holds no entries")
        return sum(1 for name, _ in self.entries if name is None)

    def diff_csv(self, path: str, cap=None) -> SnapshotDiff:
        """`diff_entries` of the next round's CSV, parsed on the host"""
        entries, _ = parse_csv_to_entries(path, self.n_currencies)
        return self.diff_entries(entries, cap)

    def _name_of_leaf(self, index: int):
        return self.entries[index][0]

    def named_groups(self, dups: DuplicateNames, limit: int = 16):
        """[(username, [its leaves: the one a lookup finds, then the shadowed ones])] for the first `limit` repeated names of
        `dups`' list"""
        return [(self._name_of_leaf(head), [head] + leaves) for head, leaves in list(dups.groups().items())[:limit]]

    def _path(self, index: int):
        """tree.rs:85-137's walk from leaf `index` up to below the root: for every level (path bit, the sibling's number in
        its level)"""
        if not 0 <= index < (1 << self.depth):
            raise IndexError("Index out of bounds")
        return [((index >> level) & 1, (index >> level) ^ 1) for level in range(self.depth)]

    def verify_proof(self, proof) -> bool:
        """tree.rs:140-190: recompute the path from the entry and the sibling preimages (hashes on the device),
        compare the root hash and balances"""
        nc = self.n_currencies
        name, bal = proof["entry"]
        u, b = self._entry_fields(name, bal)
        bb = np.frombuffer(b, dtype=np.uint8)
        node_h, node_b = _hash_batch("leaf", np.frombuffer(u, dtype=np.uint8), bb, n=1, nc=nc), bb
        for level, bit in enumerate(proof["path_indices"]):
            if level == 0:
                pre = proof["sibling_leaf_node_hash_preimage"]
                sib_b = pre[32:]
                sib_h = _hash_batch("leaf", pre[:32], sib_b, n=1, nc=nc)
            else:
                pre = proof["sibling_middle_node_hash_preimages"][level - 1]
                sib_b = pre[:32 * nc]
                # a middle node is H(balances..., left.hash, right.hash): rebuild it from two pseudo-children whose
                # balances add up to the preimage's (left = the sums, right = zero)
                zeros = np.zeros(32 * nc, dtype=np.uint8)
                sib_h, chk_b = _hash_batch("middle", pre[32 * nc:], np.concatenate([sib_b, zeros]), n=1, nc=nc)
                if not (chk_b == sib_b).all():
                    return False
            pair_h = np.concatenate([sib_h, node_h]) if bit else np.concatenate([node_h, sib_h])
            pair_b = np.concatenate([sib_b, node_b]) if bit else np.concatenate([node_b, sib_b])
            node_h, node_b = _hash_batch("middle", pair_h, pair_b, n=1, nc=nc)
        rh, rb = proof["root"]
        return bool((node_h == rh).all() and (node_b == rb).all())


class MerkleSumTree(_Tree):
    """MerkleSumTree<N_CURRENCIES, N_BYTES> (mst.rs): `from_csv`, `from_csv_sorted`, `from_entries`, `from_params`, `root`,
    `leaves`, `entries`, `index_of_username`, `update_leaf`; Tree trait (tree.rs): `depth`, `nodes`, `cryptocurrencies`,
    `get_entry`, the two preimage getters, `generate_proof`, `verify_proof`; `Entry::compute_leaf / recompute_leaf` by index.  All Poseidon hashing runs on the device; nodes are kept level-major on the host."""

    def __init__(self, depth, n_currencies, entries, node_hashes, node_balances, is_sorted=False, cryptocurrencies=None):
        self.depth, self.n_currencies, self.entries = depth, n_currencies, entries
        self._h, self._b = node_hashes, node_balances  # level-major numpy buffers
        self.is_sorted = is_sorted
        self.cryptocurrencies = cryptocurrencies or []

    @classmethod
    def from_entries(cls, entries, n_currencies: int, n_bytes: int = 8, is_sorted: bool = False):
        import torch
        n = len(entries)
        if n == 0:
            raise ValueError("empty tree")
        # mst.rs:103-134 builds the tree from any BigUint balances: one that does not fit N_BYTES only fails later, in
        # the circuit's range check (circuits/tests.rs:268-299 builds its tree from entry_16_overflow.csv)
        _check_balance_rows([bal for _, bal in entries], n_currencies, "entry with a wrong number of balances")
        depth = max(0, (n - 1).bit_length())
        size = 1 << depth
        users = bytearray(32 * size)      # zero entries: username 0, balances 0 (entry.rs:30-38)
        bals = bytearray(32 * size * n_currencies)
        for i, (name, bal) in enumerate(entries):
            u, b = cls._entry_fields(name, bal)
            users[32 * i:32 * i + 32] = u
            bals[32 * i * n_currencies:32 * (i + 1) * n_currencies] = b
        d_users = torch.from_numpy(np.frombuffer(bytes(users), dtype=np.uint8).copy()).cuda()
        d_bals = torch.from_numpy(np.frombuffer(bytes(bals), dtype=np.uint8).copy()).cuda()
        d_h, d_b = _build_nodes(d_users, d_bals, depth, n_currencies)
        torch.cuda.synchronize()
        padded = list(entries) + [(None, [0] * n_currencies)] * (size - n)
        return cls(depth, n_currencies, padded, d_h.cpu().numpy(), d_b.cpu().numpy(), is_sorted)

    @classmethod
    def from_params(cls, root, nodes, depth: int, entries, cryptocurrencies, is_sorted: bool, n_currencies: int | None = None):
        """mst.rs:137-159: a tree from parts computed elsewhere -- `nodes[level][index]` = (hash, balances) in memory
        form, level 0 the leaves, `root` = (hash, balances).  The reference stores what it is given; here the shape is
        checked as well (2^(depth - level) nodes per level, the root equal to the top node), because the level-major
        buffers below have no room for a ragged tree."""
        if len(nodes) != depth + 1 or any(len(nodes[l]) != 1 << (depth - l) for l in range(depth + 1)):
            raise ValueError("nodes: expected 2^(depth - level) nodes on every level")
        nc = n_currencies if n_currencies is not None else len(bytes(nodes[0][0][1])) // 32
        hs = np.frombuffer(b"".join(bytes(h) for lvl in nodes for h, _ in lvl), dtype=np.uint8).copy()
        bs = np.frombuffer(b"".join(bytes(b) for lvl in nodes for _, b in lvl), dtype=np.uint8).copy()
        total = (2 << depth) - 1
        if hs.size != 32 * total or bs.size != 32 * nc * total:
            raise ValueError("nodes: every node is a 32-byte hash and n_currencies 32-byte balances")
        if bytes(root[0]) != bytes(nodes[depth][0][0]) or bytes(root[1]) != bytes(nodes[depth][0][1]):
            raise ValueError("root differs from the top node")
        size = 1 << depth
        padded = list(entries) + [(None, [0] * nc)] * (size - len(entries))
        return cls(depth, nc, padded, hs, bs, is_sorted, list(cryptocurrencies))

    def nodes(self):
        """tree.rs:15 `nodes()`: every level, leaves first, as lists of (hash, balances) views"""
        return [[self.node(level, i) for i in range(1 << (self.depth - level))] for level in range(self.depth + 1)]

    def compute_leaf(self, index: int):
        """entry.rs:40-47 `Entry::compute_leaf` of entry `index`: (hash, balances), hashed on the device"""
        return self.recompute_leaf(index, self.entries[index][1])

    def recompute_leaf(self, index: int, updated_balances):
        """entry.rs:50-58 `Entry::recompute_leaf`: the leaf this entry would have with other balances (nothing is stored)"""
        if len(updated_balances) != self.n_currencies:
            raise ValueError("wrong number of balances")
        u, b = self._entry_fields(self.entries[index][0], updated_balances)
        bb = np.frombuffer(b, dtype=np.uint8)
        return _hash_batch("leaf", np.frombuffer(u, dtype=np.uint8), bb, n=1, nc=self.n_currencies), bb.copy()

    def _level_offset(self, level: int) -> int:
        return _level_first(self.depth, level)

    def node(self, level: int, index: int):
        o = self._level_offset(level) + index
        nc = self.n_currencies
        return self._h[32 * o:32 * o + 32], self._b[32 * o * nc:32 * (o + 1) * nc]

    def _set_node(self, level: int, index: int, h, b):
        o = self._level_offset(level) + index
        nc = self.n_currencies
        self._h[32 * o:32 * o + 32] = h
        self._b[32 * o * nc:32 * (o + 1) * nc] = b

    def root(self):
        return self.node(self.depth, 0)

    def leaves(self):
        """(hashes, balances) of level 0"""
        size = 1 << self.depth
        return self._h[:32 * size], self._b[:32 * size * self.n_currencies]

    def update_leaf(self, username: str, new_balances):
        """mst.rs:169-204: new balances for one user, the leaf and its `depth` ancestors are re-hashed (device,
        one call per level); returns the new root (hash, balances)"""
        nc = self.n_currencies
        _check_balance_rows([new_balances], nc, "wrong number of balances")
        index = self.index_of_username(username)
        self.entries[index] = (username, list(new_balances))
        self._updates += 1
        u, b = self._entry_fields(username, new_balances)
        ub, bb = np.frombuffer(u, dtype=np.uint8), np.frombuffer(b, dtype=np.uint8)
        self._set_node(0, index, _hash_batch("leaf", ub, bb, n=1, nc=nc), bb)
        cur = index
        for level in range(1, self.depth + 1):
            parent = cur // 2
            lh, lb = self.node(level - 1, 2 * parent)
            rh, rb = self.node(level - 1, 2 * parent + 1)
            h, bsum = _hash_batch("middle", np.concatenate([lh, rh]), np.concatenate([lb, rb]), n=1, nc=nc)
            self._set_node(level, parent, h, bsum)
            cur = parent
        return self.root()

    def get_middle_node_hash_preimage(self, level: int, index: int) -> np.ndarray:
        """tree.rs:22-56: [left.balances + right.balances ..., left.hash, right.hash] of the middle node (level, index) as
        Montgomery bytes; "Invalid depth" for the leaf level or above the root, "Node not found" beyond the level's width"""
        if level == 0 or level > self.depth:
            raise ValueError("Invalid depth")
        if not 0 <= index < (1 << (self.depth - level)):
            raise IndexError("Node not found")
        lh, _ = self.node(level - 1, 2 * index)
        rh, _ = self.node(level - 1, 2 * index + 1)
        return np.concatenate([self.node(level, index)[1], lh, rh])

    def get_leaf_node_hash_preimage(self, index: int) -> np.ndarray:
        """tree.rs:59-81: [username, balances ...] of entry `index` as Montgomery bytes"""
        name, bal = self.get_entry(index)
        u, b = self._entry_fields(name, bal)
        return np.frombuffer(u + b, dtype=np.uint8).copy()

    @staticmethod
    def middle_node_from_preimage(preimage, n_currencies: int):
        """node.rs:73-84 `Node::middle_node_from_preimage`: (hash, balances) with hash = H(preimage) on the device"""
        pre = np.asarray(preimage, dtype=np.uint8)
        bal = pre[:32 * n_currencies]
        zeros = np.zeros(32 * n_currencies, dtype=np.uint8)
        h, _ = _hash_batch("middle", pre[32 * n_currencies:], np.concatenate([bal, zeros]), n=1, nc=n_currencies)
        return h, bal.copy()

    @staticmethod
    def leaf_node_from_preimage(preimage, n_currencies: int):
        """node.rs:57-68 `Node::leaf_node_from_preimage`"""
        pre = np.asarray(preimage, dtype=np.uint8)
        return _hash_batch("leaf", pre[:32], pre[32:], n=1, nc=n_currencies), pre[32:].copy()

    def generate_proof(self, index: int):
        """tree.rs:85-137.  Besides the sibling nodes (hash, balances) the proof carries what the reference's
        MerkleProof holds: the sibling leaf's hash preimage [username, balances...] and, for every level above,
        the sibling middle node's preimage [left.bal + right.bal ..., left.hash, right.hash]."""
        path = self._path(index)
        return {"entry": self.entries[index], "leaf": self.node(0, index),
                "siblings": [self.node(level, sib) for level, (_, sib) in enumerate(path)],
                "path_indices": [bit for bit, _ in path], "root": self.root(),
                "sibling_leaf_node_hash_preimage": self.get_leaf_node_hash_preimage(index ^ 1) if self.depth else None,
                "sibling_middle_node_hash_preimages": [self.get_middle_node_hash_preimage(level, sib)
                                                       for level, (_, sib) in enumerate(path) if level > 0]}


def pack_entries(entries, n_currencies: int):
    """[(username, [balances])] -> (name_bytes, name_off, digit_bytes, digit_off), the host buffers of sg_mst_entries_dev:
    the UTF-8 names back to back with n + 1 byte offsets, the balances as `str(int)` back to back (entry-major, one field
    per currency) with n * n_currencies + 1 offsets.  Host code only; refuses what MerkleSumTree.from_entries refuses."""
    # _check_balance_rows' checks, in its order, inside the one pass that packs: a pass of their own costs 2 ms in 2^16 entries
    names, flat = [], []
    for name, bal in entries:
        if len(bal) != n_currencies:
            raise ValueError("entry with a wrong number of balances")
        names.append(name.encode())
        flat += bal
    if flat and min(flat) < 0:
        raise ValueError("Invalid balance")
    name_off = np.zeros(len(names) + 1, dtype=np.uint64)
    np.cumsum(np.fromiter(map(len, names), dtype=np.uint64, count=len(names)), out=name_off[1:])
    return (np.frombuffer(b"".join(names), dtype=np.uint8), name_off) + pack_balances(flat)


def pack_balances(flat):
    """non-negative integers -> (digit_bytes, digit_off): `str(int)` back to back with len(flat) + 1 offsets, the balance half
    of sg_mst_entries_dev's host buffers and all of sg_mst_update_dev's"""
    # the balances in one string with a comma between them: a field ends where a comma stood, less the commas before it
    text = np.frombuffer(",".join(map(str, flat)).encode(), dtype=np.uint8)
    comma = text == ord(",")
    ends = np.flatnonzero(comma)
    digit_off = np.zeros(len(flat) + 1, dtype=np.uint64)
    if flat:
        digit_off[1:-1] = ends - np.arange(ends.size)
        digit_off[-1] = text.size - ends.size
    return text[~comma], digit_off


# what sg_mst_csv_scan_dev and sg_mst_csv_entries_dev report of a file outside the device reader's subset (include/summa_gpu.h:
# SG_MST_CSV_FLAG_*, SG_MST_CSV_ROW_*), in the words of csv_fallback_reason
_CSV_FLAGS = ((0x40000000, "a quote, NUL or non-ASCII byte"), (0x80000000, "a carriage return without a line feed"))
_CSV_ROW_PROBLEMS = {1: "longer than csv's field limit", 2: "empty", 3: "not n_currencies + 1 fields", 4: "an empty balance",
                     5: "a balance that is not decimal digits", 6: "row starts out of order",
                     7: "name too long for the device sort"}      # include/summa_snapshot.h: from_csv_sorted alone
_ABSENT = 0xFFFFFFFF          # SS_MST_FIND_ABSENT


class RangeAudit:
    """What `DeviceMerkleSumTree.range_audit` found (include/summa_snapshot.h: ss_mst_range_audit_dev), against top = 2^(8 n_bytes):
      n_bad_nodes     nodes of the tree, the root included, with a balance >= top
      n_unprovable    leaves whose circuit fails a range check
      unprovable      numpy.uint32: those leaves in increasing order (with a `cap`, the first `cap` of them)
      root_in_range, root_currency   the root's sums (the circuit leaves them to verification): the lowest offending currency or None
      ok              no unprovable leaf and the root in range
      d_node_flags    uint8 per node, level-major: 0, or 1 + the lowest currency whose balance is >= top
      d_leaf_reasons  int32 per leaf: bit 0 the leaf's own balances, bit l + 1 the path's sibling at level l -- the circuit's range
                      checks in the order of `synthesize`; 0: the user is provable
    The two arrays are device tensors after `range_audit`; numpy arrays serve as well (the CPU tests make audits by hand).
    An audit is a snapshot of a snapshot: after `update_leaves*` it is stale, and running it again is the remedy."""

    def __init__(self, n_bytes, n_bad_nodes, n_unprovable, unprovable, root_flag, d_node_flags, d_leaf_reasons):
        self.n_bytes, self.n_bad_nodes, self.n_unprovable = n_bytes, int(n_bad_nodes), int(n_unprovable)
        self.unprovable = np.asarray(unprovable, dtype=np.uint32)
        self.root_in_range = root_flag == 0
        self.root_currency = int(root_flag) - 1 if root_flag else None
        self.d_node_flags, self.d_leaf_reasons = d_node_flags, d_leaf_reasons
        self.depth = int(d_leaf_reasons.shape[0]).bit_length() - 1

    @property
    def ok(self) -> bool:
        return self.n_unprovable == 0 and self.root_in_range

    @staticmethod
    def _take(array, indices, dtype):
        if isinstance(array, np.ndarray):
            return array[np.asarray(indices, dtype=np.int64)].astype(dtype)
        import torch
        return array[torch.as_tensor(indices, dtype=torch.int64, device=array.device)].cpu().numpy().astype(dtype)

    def reasons(self, indices) -> np.ndarray:
        """the masks of some leaves as numpy.uint32: one gather and one copy"""
        indices = [int(i) for i in indices]
        if any(not 0 <= i < (1 << self.depth) for i in indices):
            raise IndexError("Index out of bounds")
        return self._take(self.d_leaf_reasons, indices, np.uint32) if indices else np.zeros(0, dtype=np.uint32)

    def checks_of(self, index: int, mask: int):
        """the failing range checks a mask names, in the circuit's order: [(what, level, node within its level)]"""
        out = [("leaf", 0, index)] if mask & 1 else []
        return out + [("sibling", l, (index >> l) ^ 1) for l in range(self.depth) if (mask >> (l + 1)) & 1]

    def first_failures(self, indices):
        """per leaf None (provable) or the first range check its circuit fails, (what, level, node, currency): two gathers"""
        indices = [int(i) for i in indices]
        firsts = [self.checks_of(i, int(m))[0] if m else None for i, m in zip(indices, self.reasons(indices))]
        at = [_level_first(self.depth, f[1]) + f[2] for f in firsts if f is not None]
        flags = iter(self._take(self.d_node_flags, at, np.int64)) if at else iter(())
        return [None if f is None else f + (int(next(flags)) - 1,) for f in firsts]


def range_check_text(failure) -> str:
    """(what, level, node, currency) -> the words prove_batch files the user under"""
    what, level, _, currency = failure
    return f"range check: leaf, currency {currency}" if what == "leaf" else f"range check: sibling at level {level}, currency {currency}"


class DeviceMerkleSumTree(_Tree):
    """A Merkle sum tree whose leaves are already field elements on the device (a snapshot of 2^depth users: username
    field elements and balances as Montgomery Fr), built and KEPT in HBM: level-major node arrays as `sg_mst_build_dev`
    lays them out.  The reference's `Tree` trait [REF zk_prover/src/merkle_sum_tree/tree.rs:8-137] for the two methods a
    prover needs -- `root`, `generate_proof` --; a Merkle proof costs one gather of 3 * depth + 2 rows and one small
    device-to-host copy.  (MerkleSumTree above is the CSV / entries flavour with the nodes mirrored on the host.)

    `from_entries`, `from_csv` and `from_csv_sorted` build the same tree from what an exchange has, usernames and
    integer balances: the leaves' field elements are made on the device (sg_mst_entries_dev) and nothing comes back.  Such
    a tree also knows its entries by name -- `entries`, `get_entry`, `index_of_username`, `cryptocurrencies`, `is_sorted`, and
    the `entry` of a Merkle proof carries the name, as MerkleSumTree's do; after the plain constructor `entries` is None.
    `from_csv` reads the file's text on the device where it can (`csv_ingest`); such a tree parses the file on the host only
    when its entries are first asked for by name, which `root`, `public_inputs_many`, `update_leaves_at` and the provers never do.
    `from_csv_sorted` does the same and sorts the names on the device too (mst.rs:89-100; names of up to 64 bytes).  Such a tree
    keeps the file's text, the file row of every leaf and the span of every leaf's name in HBM -- the file's size plus 12 bytes a
    row (4 of `d_order`, 8 of `d_name_spans`), beside roughly 200 MB of nodes at 2^20 users and two currencies -- and, while its
    entries are unparsed, answers by name from there (ss_mst_find_names: one binary search per name over the text):
    `index_of_username`, `indices_of_usernames`, `update_leaf` / `update_leaves` and the `entry` of `generate_proof` do not parse
    the file.  `entries` still does, once, and puts the rows in leaf order through `d_order`.
    `from_csv(..., name_index=True)` gives a tree in FILE order -- the only order whose root equals a commitment made from the
    same file by the reference -- the same ability: the names are sorted beside the leaves, which stay where they are
    (ss_mst_csv_name_index_dev), the tree keeps the text, `d_order`, the sorted names' spans and the names' spans in file order
    (the file's size plus 20 bytes a row), and the same lookups go through ss_mst_find_leaves, a repeated name to its first row
    in file order as mst.rs:207-223 finds it.  `has_name_index` says whether a tree holds such an order, `name_index_reason` why
    one that was asked for is missing.

    `duplicate_names` reports the usernames that occur more than once -- the reference accepts such a file silently, and every
    row of a name behind its first is a leaf no lookup, update or proof by name can reach -- from the sorted order in HBM where
    the tree holds one (ss_mst_duplicate_names_dev, no parse), else from `entries`; `named_groups` reads the names.

    `update_leaf`, `update_leaves` and `update_leaves_at` change balances in place (sg_mst_update_dev): the leaves and the nodes
    above them are re-hashed on the device, in the arrays the tree was built from (`d_balances` of the plain constructor is
    written too), and nothing comes back but the root when it is next asked for.

    `diff_csv` joins the NEXT round's CSV with the tree by username -- who changed, who is new, who is gone (SnapshotDiff) --, where
    both texts lie when the tree holds the names' order (sr_mst_csv_diff_dev), else from `entries`; `apply_diff` writes the changed
    balances in place without moving a leaf (sr_mst_apply_diff_dev: the balances are folded from the file's text in HBM and never
    visit the host), `apply_csv` does both.  The tree counts its updates, and a diff taken before another update is refused.
    With `admit_new=True` and `zero_gone=True` the apply settles the round in full (sa_mst_admit_measure_dev, sa_mst_settle_dev):
    the new users become leaves in the padding behind the named ones, the name index and the text in HBM grow by them, the gone
    users' balances become zero, and all of it is one run of the update's kernels.  `free_leaves` says how many still fit.

    `to_csv` writes the snapshot the tree commits to NOW back out as a CSV the reader takes -- the names from the text in HBM, the
    balances from `d_bals` as they are after any update or applied round (sx_mst_csv_measure_dev, sx_mst_csv_write_dev) -- when the
    tree holds the names' order in HBM, else from `entries`; `csv_body_dev` leaves the rows on the device.

    `range_audit` says which users of the snapshot can receive a valid inclusion proof at all -- whose circuit would fail a range
    check, and at which one -- from the node balances in HBM (ss_mst_range_audit_dev); `explain_unprovable` names the balances."""

    _entries = None           # [(name, balances)] padded with (None, [0] * n_currencies): trees built from entries only
    _name_index = None        # {name: first index}, made by the first update_leaves
    is_sorted = False
    cryptocurrencies = ()
    csv_ingest = None         # from_csv: "device" (the file's text was read on the device) or "host" (parse_csv_to_entries)
    csv_fallback_reason = None    # ... and why the host read it
    _csv_lazy = None          # a device-read tree whose entries nobody has asked for: (path, {leaf index: balances set since})
    _sorted_dev = None        # a device-sorted tree: {"text", "size", "body_off", "delim", "n", "d_order", "d_name_spans"}
    _applied = ()             # the changed leaves of every device diff applied while the entries were unparsed
    _index_dev = None         # from_csv(name_index=True): the same record beside leaves in file order, plus "d_leaf_name_spans"
    name_index_reason = None  # from_csv(name_index=True) without an index: why
    _csv_delim = None         # a device-read tree: the delimiter of its source file

    @property
    def entries(self):
        """None for a tree built from field elements.  A tree whose CSV the device read parses the file for them only now, on the
        host: the proving paths never ask."""
        if self._entries is None and self._csv_lazy is not None:
            path, changed = self._csv_lazy
            parsed, _ = parse_csv_to_entries(path, self.n_currencies)
            if self._sorted_dev is not None:                  # the device's order: one copy and no host sort
                parsed = [parsed[i] for i in self._sorted_dev["d_order"].cpu().tolist()]
            n_file = len(parsed)
            parsed += [(None, [0] * self.n_currencies)] * ((1 << self.depth) - len(parsed))
            if self._index_dev is not None and self._index_dev["n"] > n_file:     # admitted since: the names from the text in HBM
                for j, name in enumerate(self._names_of_leaves(n_file, self._index_dev["n"])):
                    parsed[n_file + j] = (name, parsed[n_file + j][1])
            if self._applied:                                 # leaves an applied diff changed: their balances are d_bals'
                leaves = np.unique(np.concatenate(self._applied))
                for i, bal in zip(leaves.tolist(), self._balances_of_leaves(leaves)):
                    parsed[i] = (parsed[i][0], bal)
                self._applied = ()
            for i, bal in changed.items():
                parsed[i] = (parsed[i][0], bal)
            self._entries, self._csv_lazy = parsed, None
        return self._entries

    @entries.setter
    def entries(self, value):
        self._entries, self._csv_lazy = value, None

    @property
    def has_name_index(self) -> bool:
        """the names' sorted order lies in HBM beside the tree: `from_csv_sorted` on the device, or `from_csv(name_index=True)`"""
        return self._names_dev() is not None

    def _names_dev(self):
        return self._sorted_dev if self._sorted_dev is not None else self._index_dev

    def __init__(self, d_usernames, d_balances, depth: int, n_currencies: int):
        import torch
        size = 1 << depth
        if d_usernames.numel() != 32 * size or d_balances.numel() != 32 * size * n_currencies:
            raise ValueError("DeviceMerkleSumTree: 2^depth usernames and 2^depth * n_currencies balances expected")
        self.depth, self.n_currencies = depth, n_currencies
        self.d_users, self.d_bals = d_usernames, d_balances
        self.d_h, self.d_b = _build_nodes(d_usernames, d_balances, depth, n_currencies)
        # the snapshot is read from other streams afterwards (proofs in flight run one stream per worker thread, and the
        # first reader caches the root): the build -- one-off, tens of milliseconds -- is complete when the constructor returns
        torch.cuda.current_stream().synchronize()
        self.offsets = [_level_first(depth, level) for level in range(depth + 1)]
        self._root = None

    @classmethod
    def from_entries(cls, entries, n_currencies: int, n_bytes: int = 8, is_sorted: bool = False):
        """mst.rs:103-134 with the tree in HBM: `Entry::new` of every entry on the device (keccak256 of the name, the decimal
        balances folded in the field), zero entries up to 2^depth, then the constructor's build.  As in MerkleSumTree.from_entries
        a balance that does not fit `n_bytes` only fails later, in the circuit's range check (`range_audit` finds it sooner)."""
        import torch
        entries = list(entries)
        n = len(entries)
        if n == 0:
            raise ValueError("empty tree")
        packed = pack_entries(entries, n_currencies)
        name_bytes, name_off, digit_bytes, digit_off = packed
        if name_bytes.size == 0:
            name_bytes = np.zeros(1, dtype=np.uint8)          # only empty names: a buffer to point at all the same
        depth = max(0, (n - 1).bit_length())
        size = 1 << depth
        d_users = torch.empty(32 * size, dtype=torch.uint8, device="cuda")
        d_bals = torch.empty(32 * size * n_currencies, dtype=torch.uint8, device="cuda")
        ffi.check(ffi.lib().sg_mst_entries_dev(ffi.ptr(name_bytes), ffi.ptr(name_off), ffi.ptr(digit_bytes), ffi.ptr(digit_off),
                                               C.c_size_t(n), C.c_size_t(size), C.c_uint32(n_currencies), ffi.dev_ptr(d_users),
                                               ffi.dev_ptr(d_bals), ffi.current_stream_ptr()))
        tree = cls(d_users, d_bals, depth, n_currencies)       # same stream; synchronized when it returns
        tree.entries = entries + [(None, [0] * n_currencies)] * (size - n)
        tree.is_sorted = is_sorted
        tree.cryptocurrencies = []
        return tree

    @classmethod
    def from_csv(cls, path: str, n_currencies: int, n_bytes: int = 8, name_index: bool = False):
        """mst.rs:74-87 with the file's text read where the tree is built (sg_mst_csv_scan_dev, sg_mst_csv_entries_dev): the
        host parses the header line alone, the device finds the rows and fields and hashes and folds them in place.  The
        device takes a strict subset of CSV text (include/summa_gpu.h) and judges no data: any other file goes the way every
        file went before, parse_csv_to_entries and from_entries, which accepts or refuses it.  `csv_ingest` says which way
        it was, `csv_fallback_reason` why the host's.  After the device's `entries` is made on first use, from the file.
        name_index: also sort the names on the device beside the leaves, which stay in file order (ss_mst_csv_name_index_dev),
        and keep the text and the index in HBM -- the file's size plus 20 bytes a row -- so that the tree answers by name and
        reports repeated names without parsing the file.  `has_name_index` says whether it does, `name_index_reason` why not:
        a name of more than 64 bytes (the tree is device-read all the same), or the host's reason for reading the file."""
        tree, reason = cls._from_csv_on_device(path, n_currencies, name_index=name_index)
        if tree is None:
            tree = super().from_csv(path, n_currencies, n_bytes)
            tree.csv_ingest, tree.csv_fallback_reason = "host", reason
            if name_index:
                tree.name_index_reason = reason
        return tree

    @classmethod
    def from_csv_sorted(cls, path: str, n_currencies: int, n_bytes: int = 8):
        """mst.rs:89-100 with the file's text read and its names sorted where the tree is built (sg_mst_csv_scan_dev,
        ss_mst_csv_entries_sorted_dev): `from_csv` with the leaves ordered by the usernames' bytes, equal names in file order.
        The device takes the reader's subset of CSV text and names of at most 64 bytes; any other file goes the way every
        file went before (parse_csv_to_entries, a host sort, from_entries).  `csv_ingest` and `csv_fallback_reason` as for
        `from_csv`."""
        tree, reason = cls._from_csv_on_device(path, n_currencies, sorted_leaves=True)
        if tree is None:
            tree = super().from_csv_sorted(path, n_currencies, n_bytes)
            tree.csv_ingest, tree.csv_fallback_reason = "host", reason
        return tree

    @classmethod
    def _from_csv_on_device(cls, path: str, n_currencies: int, sorted_leaves: bool = False, name_index: bool = False):
        """-> (tree, None), or (None, why the device does not take this file); sorted_leaves: the leaves in the order of the
        names' bytes; name_index: the leaves in file order and the names' sorted order beside them"""
        import torch
        scanned, reason = cls._csv_text_on_device(path, n_currencies)
        if scanned is None:
            return None, reason
        d_text, size, body_off, delim, crypto, d_tiles, n = scanned
        L = ffi.lib()
        stream = ffi.current_stream_ptr()
        depth = max(0, (n - 1).bit_length())
        rows = 1 << depth
        d_users = torch.empty(32 * rows, dtype=torch.uint8, device="cuda")
        d_bals = torch.empty(32 * rows * n_currencies, dtype=torch.uint8, device="cuda")
        problem = C.c_uint64(0)
        if sorted_leaves:
            S = ffi.snapshot_lib()
            sort_bytes = C.c_uint64(0)
            ffi.check(S.ss_mst_sort_scratch(n, C.byref(sort_bytes)))
            d_spans = torch.empty(2 * (n + 1 + 2 * n * (1 + n_currencies)), dtype=torch.int64, device="cuda")
            d_sort = torch.empty(sort_bytes.value, dtype=torch.uint8, device="cuda")
            d_order = torch.empty(n, dtype=torch.int32, device="cuda")
            d_name_spans = torch.empty(2 * n, dtype=torch.int32, device="cuda")
            ffi.check(S.ss_mst_csv_entries_sorted_dev(ffi.dev_ptr(d_text), size, body_off, ffi.dev_ptr(d_tiles), ord(delim), n_currencies, n,
                                                      rows, ffi.dev_ptr(d_spans), ffi.dev_ptr(d_sort), ffi.dev_ptr(d_order),
                                                      ffi.dev_ptr(d_name_spans), ffi.dev_ptr(d_users), ffi.dev_ptr(d_bals),
                                                      C.byref(problem), stream))
        else:
            # with the index the two blocks of the sorted call: the entries call uses the first, the index call both
            span_words = 2 * (n + 1 + 2 * n * (1 + n_currencies)) if name_index else n + 2 + 2 * n * (1 + n_currencies)
            d_spans = torch.empty(span_words, dtype=torch.int64, device="cuda")
            ffi.check(L.sg_mst_csv_entries_dev(ffi.dev_ptr(d_text), size, body_off, ffi.dev_ptr(d_tiles), ord(delim), n_currencies, n, rows,
                                               ffi.dev_ptr(d_spans), ffi.dev_ptr(d_users), ffi.dev_ptr(d_bals), C.byref(problem), stream))
        if problem.value:
            return None, f"row {problem.value >> 8}: {_CSV_ROW_PROBLEMS.get(problem.value & 0xff, 'outside the subset')}"
        index, index_reason = None, None
        if name_index and not sorted_leaves:
            S = ffi.snapshot_lib()
            sort_bytes = C.c_uint64(0)
            ffi.check(S.ss_mst_sort_scratch(n, C.byref(sort_bytes)))
            d_sort = torch.empty(sort_bytes.value, dtype=torch.uint8, device="cuda")
            d_order = torch.empty(n, dtype=torch.int32, device="cuda")
            d_name_spans = torch.empty(2 * n, dtype=torch.int32, device="cuda")
            d_leaf_name_spans = torch.empty(2 * n, dtype=torch.int32, device="cuda")
            ffi.check(S.ss_mst_csv_name_index_dev(ffi.dev_ptr(d_text), size, body_off, ffi.dev_ptr(d_tiles), ord(delim), n_currencies, n,
                                                  ffi.dev_ptr(d_spans), ffi.dev_ptr(d_sort), ffi.dev_ptr(d_order), ffi.dev_ptr(d_name_spans),
                                                  ffi.dev_ptr(d_leaf_name_spans), C.byref(problem), stream))
            if problem.value:                                 # in practice a name over 64 bytes: the tree is device-read all the same
                index_reason = f"row {problem.value >> 8}: {_CSV_ROW_PROBLEMS.get(problem.value & 0xff, 'outside the subset')}"
            else:
                index = {"text": d_text, "size": size, "body_off": body_off, "delim": delim, "n": n, "d_order": d_order,
                         "d_name_spans": d_name_spans, "d_leaf_name_spans": d_leaf_name_spans}
        tree = cls(d_users, d_bals, depth, n_currencies)       # same stream; synchronized when it returns
        if name_index and not sorted_leaves:
            tree._index_dev, tree.name_index_reason = index, index_reason
        if sorted_leaves:
            tree.is_sorted = True
            tree._sorted_dev = {"text": d_text, "size": size, "body_off": body_off, "delim": delim, "n": n, "d_order": d_order,
                                "d_name_spans": d_name_spans}
        tree._csv_lazy = (path, {})
        tree._csv_delim = delim
        tree.cryptocurrencies = crypto
        tree.csv_ingest = "device"
        return tree, None

    @staticmethod
    def _csv_text_on_device(path: str, n_currencies: int):
        """The text of a snapshot CSV in HBM behind its header line, which the host parses, and the reader's scan of it
        (sg_mst_csv_scan_dev): -> ((d_text, size, body_off, delim, cryptocurrencies, d_tiles, n_rows), None), or (None, why the
        device does not take this file)"""
        import torch
        if not 1 <= n_currencies <= 64:
            return None, "n_currencies outside 1..64"
        data = np.fromfile(path, dtype=np.uint8)
        line, eol, _ = data[:1 << 16].tobytes().partition(b"\n")
        if not eol:
            return None, "no line end in the first 64 KiB"
        body_off, size = len(line) + 1, int(data.size)
        line = line[:-1] if line.endswith(b"\r") else line
        if not line.isascii() or any(c in line for c in b'"\r\0'):
            return None, "header line: a quote, carriage return, NUL or non-ASCII byte"
        delim = ";" if b";" in line else ","
        header = line.decode().split(delim)
        crypto = [tuple(h.split("_")[1:]) for h in header[1:]]
        if (len(header) - 1 != n_currencies or header[0] != "username"
                or any(len(h.split("_")) != 3 or h.split("_")[0] != "balance" for h in header[1:])):
            return None, "header line: not username and n_currencies balance_<name>_<chain> columns"
        if body_off == size:
            return None, "no rows"
        if size - body_off >= 1 << 32:
            return None, "a body of 4 GiB or more"
        L = ffi.lib()
        tile, cap = C.c_uint32(0), C.c_uint32(0)
        L.sg_mst_csv_geometry(C.byref(tile), C.byref(cap))
        pad = -body_off % 16                                  # the body on a 16-byte boundary: the kernels' wide loads
        d_file = torch.empty(pad + size, dtype=torch.uint8, device="cuda")
        d_file[pad:].copy_(torch.from_numpy(data))
        d_text = d_file[pad:]
        d_tiles = torch.empty(-(-(size - body_off) // tile.value) + 2, dtype=torch.int32, device="cuda")
        n_rows, flags = C.c_uint64(0), C.c_uint32(0)
        stream = ffi.current_stream_ptr()
        ffi.check(L.sg_mst_csv_scan_dev(ffi.dev_ptr(d_text), size, body_off, ffi.dev_ptr(d_tiles), C.byref(n_rows), C.byref(flags), stream))
        if flags.value:
            return None, " and ".join(text for bit, text in _CSV_FLAGS if flags.value & bit)
        n = n_rows.value
        if n == 0:
            return None, "no rows"
        return (d_text, size, body_off, delim, crypto, d_tiles, n), None

    def _finds_on_device(self) -> bool:
        """a device-read tree that holds the names' sorted order and whose entries are still unparsed: names are looked up in the
        text in HBM"""
        return self._entries is None and self._csv_lazy is not None and self._names_dev() is not None

    def index_of_username(self, username: str) -> int:
        """mst.rs:207-223; on a tree with the names' order in HBM whose entries are unparsed a binary search on the device, no
        parse"""
        if self._finds_on_device():
            return self.indices_of_usernames([username])[0]
        return super().index_of_username(username)

    def indices_of_usernames(self, usernames):
        """`index_of_username` of every name, a repeated name's first leaf: one device call on a tree with the names' order in HBM
        whose entries are unparsed (ss_mst_find_names on a device-sorted tree; ss_mst_find_leaves, which answers through `d_order`,
        on one in file order).  KeyError("Username not found") if any name is missing."""
        usernames = list(usernames)
        if not self._finds_on_device():
            return [self.index_of_username(name) for name in usernames]
        if not usernames:
            return []
        names = [name.encode() for name in usernames]
        name_off = np.zeros(len(names) + 1, dtype=np.uint64)
        np.cumsum(np.fromiter(map(len, names), dtype=np.uint64, count=len(names)), out=name_off[1:])
        name_bytes = np.frombuffer(b"".join(names) or b"\0", dtype=np.uint8)       # only empty names: a buffer to point at all the same
        found = np.zeros(len(names), dtype=np.uint32)
        d = self._names_dev()
        if self._sorted_dev is not None:
            ffi.check(ffi.snapshot_lib().ss_mst_find_names(ffi.dev_ptr(d["text"]), d["size"], d["body_off"], ffi.dev_ptr(d["d_name_spans"]),
                                                           d["n"], ffi.ptr(name_bytes), ffi.ptr(name_off), len(names), ffi.ptr(found),
                                                           ffi.current_stream_ptr()))
        else:
            ffi.check(ffi.snapshot_lib().ss_mst_find_leaves(ffi.dev_ptr(d["text"]), d["size"], d["body_off"], ffi.dev_ptr(d["d_name_spans"]),
                                                            ffi.dev_ptr(d["d_order"]), d["n"], ffi.ptr(name_bytes), ffi.ptr(name_off),
                                                            len(names), ffi.ptr(found), ffi.current_stream_ptr()))
        if (found == _ABSENT).any():
            raise KeyError("Username not found")
        return [int(i) for i in found]

    def _entry_from_text(self, index: int):
        """entry `index` of a tree with the names' order in HBM whose entries are unparsed, from the row's text there: two small
        copies.  The leaf's name span is the sorted one on a device-sorted tree, `d_leaf_name_spans` on one in file order."""
        nc, d = self.n_currencies, self._names_dev()
        if index >= d["n"]:
            return (None, [0] * nc)
        leaf_spans = d.get("d_leaf_name_spans", d["d_name_spans"])
        begin, end = (int(x) & 0xFFFFFFFF for x in leaf_spans[2 * index:2 * index + 2].cpu().tolist())
        lo, text = d["body_off"] + begin, b""
        if index in self._csv_lazy[1]:
            balances = self._csv_lazy[1][index]
        elif any(a[min(int(np.searchsorted(a, index)), a.size - 1)] == index for a in self._applied):
            balances = self._balances_of_leaves([index])[0]   # an applied diff wrote it: the leaf's own row of d_bals says what it holds
        else:
            balances = None
        if balances is not None:                              # the name alone: an admitted leaf has no row behind it
            return (bytes(d["text"][lo:lo + end - begin].cpu().numpy()).decode(), balances)
        want = end - begin + 1 + 24 * nc
        size = d.get("file_size", d["size"])                  # the source file's own end: admitted names lie behind it, unseparated
        while b"\n" not in text[end - begin:] and lo + len(text) < size:           # the row ends at its line end or the file's
            text = bytes(d["text"][lo:min(size, lo + want)].cpu().numpy())
            want *= 4
        row = text[end - begin + 1:].split(b"\n")[0].rstrip(b"\r")
        return (text[:end - begin].decode(), [int(x) for x in row.split(d["delim"].encode())])

    def _names_of_leaves(self, lo: int, hi: int):
        """the names of the admitted leaves lo .. hi - 1 from the text in HBM, where they lie one after the other: two small copies"""
        d = self._index_dev
        spans = [int(x) & 0xFFFFFFFF for x in d["d_leaf_name_spans"][2 * lo:2 * hi].cpu().tolist()]
        first = spans[0]
        blob = bytes(d["text"][d["body_off"] + first:d["body_off"] + spans[-1]].cpu().numpy())
        return [blob[b - first:e - first].decode() for b, e in zip(spans[0::2], spans[1::2])]

    @property
    def free_leaves(self) -> int:
        d = self._names_dev()
        return (1 << self.depth) - d["n"] if d is not None else super().free_leaves

    def get_entry(self, index: int):
        """tree.rs's get_entry; on a tree with the names' order in HBM whose entries are unparsed from the row's text there, no parse"""
        if self._finds_on_device() and 0 <= index < (1 << self.depth):
            return self._entry_from_text(index)
        return super().get_entry(index)

    def update_leaf(self, username: str, new_balances):
        """mst.rs:169-204: new balances for one user; the leaf and its `depth` ancestors are re-hashed in place on the device.
        Returns the new root (hash, balances)."""
        return self.update_leaves([(username, new_balances)])

    def update_leaves(self, updates):
        """`update_leaf` for every (username, [balances]) of `updates` as one device call (sg_mst_update_dev): the leaves, then
        the distinct ancestors level by level.  A username that appears twice keeps its last balances, which is what the
        updates applied one after another leave.  Everything is checked first: a refused batch leaves the tree as it was."""
        updates = list(updates)
        if self._finds_on_device():       # the names are found where the text lies: no parse
            return self.update_leaves_at(self.indices_of_usernames([name for name, _ in updates]), [bal for _, bal in updates])
        if self.entries is None:
            raise KeyError("Username not found")
        if self._name_index is None:      # names never change: the first index of each, as index_of_username finds it
            self._name_index = {}
            for i, (name, _) in enumerate(self.entries):
                if name is not None:
                    self._name_index.setdefault(name, i)
        indices = []
        for name, _ in updates:
            if name not in self._name_index:
                raise KeyError("Username not found")
            indices.append(self._name_index[name])
        return self.update_leaves_at(indices, [bal for _, bal in updates])

    def update_leaves_at(self, indices, balances):
        """the same by leaf index: `balances[j]` are the new balances of leaf `indices[j]`, padded rows and the leaves of a tree
        built from field elements included.  A repeated index keeps its last balances."""
        indices, balances = list(indices), list(balances)
        if len(indices) != len(balances):
            raise ValueError("as many balance rows as indices expected")
        nc = self.n_currencies
        if not indices:
            return self.root()
        if min(indices) < 0 or max(indices) >= (1 << self.depth):
            raise IndexError("Index out of bounds")
        _check_balance_rows(balances, nc, "wrong number of balances")
        last = dict(zip(indices, balances))                   # a repeated index keeps its last row
        order = sorted(last)
        flat = [int(b) for i in order for b in last[i]]
        digit_bytes, digit_off = pack_balances(flat)
        self._update_dev(np.array(order, dtype=np.uint32), digit_bytes, digit_off)
        self._root = None
        if self._csv_lazy is not None:                        # entries nobody has read yet: kept for when somebody does
            self._csv_lazy[1].update((i, flat[nc * j:nc * j + nc]) for j, i in enumerate(order))
        elif self.entries is not None:
            for j, i in enumerate(order):
                self.entries[i] = (self.entries[i][0], flat[nc * j:nc * j + nc])
        return self.root()

    def _update_dev(self, indices, digit_bytes, digit_off):
        """sg_mst_update_dev over the tree's four arrays, on the current stream; complete when it returns, for the
        constructor's reason -- and no proof may be reading the tree from another stream while it runs"""
        import torch
        ffi.check(ffi.lib().sg_mst_update_dev(ffi.ptr(indices), ffi.ptr(digit_bytes), ffi.ptr(digit_off), indices.size, self.depth,
                                              self.n_currencies, ffi.dev_ptr(self.d_users), ffi.dev_ptr(self.d_bals),
                                              ffi.dev_ptr(self.d_h), ffi.dev_ptr(self.d_b), ffi.current_stream_ptr()))
        torch.cuda.current_stream().synchronize()
        self._updates += 1

    def diff_csv(self, path: str, cap=None) -> SnapshotDiff:
        """The next round's CSV against this tree (SnapshotDiff has the rules).  A tree with the names' order in HBM
        (`has_name_index`) joins the two texts where they lie, in one device call on the current stream (sr_mst_csv_diff_dev), when
        the file is inside the device reader's subset: neither file is parsed on the host, and the lists and the summary are all
        that comes back.  Any other tree or file goes the host's way, `diff_entries` of the parsed file, and the diff says why
        (`ingest`, `fallback_reason`).  cap: list at most that many new rows and gone leaves (None: all)."""
        if cap is not None and cap < 0:
            raise ValueError("cap below 0")
        diff, reason = self._diff_csv_on_device(path, cap)
        if diff is None:
            diff = super().diff_csv(path, cap)
            diff.fallback_reason = reason
        return diff

    def _diff_csv_on_device(self, path: str, cap):
        """-> (diff, None), or (None, why the device does not take this tree or this file)"""
        import torch
        t = self._names_dev()
        if t is None:
            return None, "the tree holds no name index"
        nc, depth = self.n_currencies, self.depth
        scanned, reason = self._csv_text_on_device(path, nc)
        if scanned is None:
            return None, reason
        d_text, size, body_off, delim, _, d_tiles, n = scanned
        R = ffi.rounds_lib()
        leaves = 1 << depth
        list_cap = max(n, leaves) if cap is None else min(int(cap), max(n, leaves))
        scratch_bytes = C.c_uint64(0)
        ffi.check(R.sr_mst_diff_scratch(n, depth, C.byref(scratch_bytes)))
        i32 = lambda count: torch.empty(count, dtype=torch.int32, device="cuda")
        d_spans = torch.empty(n + 2 + 2 * n * (1 + nc), dtype=torch.int64, device="cuda")
        d_row_leaf, d_owner, d_changed = i32(n), i32(leaves), i32(min(n, leaves))
        d_row_state = torch.empty(n, dtype=torch.uint8, device="cuda")
        d_leaf_state = torch.empty(leaves, dtype=torch.uint8, device="cuda")
        d_new, d_gone = (i32(list_cap), i32(list_cap)) if list_cap else (None, None)
        d_scratch = i32(scratch_bytes.value // 4)
        problem, summary = C.c_uint64(0), (C.c_uint64 * 8)()
        ffi.check(R.sr_mst_csv_diff_dev(ffi.dev_ptr(d_text), size, body_off, ffi.dev_ptr(d_tiles), ord(delim), nc, n, ffi.dev_ptr(d_spans),
                                        ffi.dev_ptr(t["text"]), t["size"], t["body_off"], ffi.dev_ptr(t["d_name_spans"]),
                                        None if self._sorted_dev is not None else ffi.dev_ptr(t["d_order"]), t["n"], depth,
                                        ffi.dev_ptr(self.d_bals), ffi.dev_ptr(d_row_leaf), ffi.dev_ptr(d_row_state), ffi.dev_ptr(d_leaf_state),
                                        ffi.dev_ptr(d_owner), ffi.dev_ptr(d_changed), ffi.dev_ptr(d_new) if list_cap else None,
                                        ffi.dev_ptr(d_gone) if list_cap else None, list_cap, ffi.dev_ptr(d_scratch), C.byref(problem), summary,
                                        ffi.current_stream_ptr()))
        if problem.value:
            return None, f"row {problem.value >> 8}: {_CSV_ROW_PROBLEMS.get(problem.value & 0xff, 'outside the subset')}"
        take = lambda d, count: d[:count].cpu().numpy().view(np.uint32) if count else np.zeros(0, dtype=np.uint32)
        diff = SnapshotDiff(list(summary)[:6], take(d_changed, int(summary[2])), take(d_new, int(summary[6])), take(d_gone, int(summary[7])),
                            {"row_leaf": d_row_leaf, "row_state": d_row_state, "leaf_state": d_leaf_state, "owner": d_owner}, "device",
                            dev={"text": d_text, "size": size, "body_off": body_off, "n": n, "d_spans": d_spans, "d_owner": d_owner,
                                 "d_changed": d_changed, "d_new": d_new, "d_gone": d_gone, "d_row_state": d_row_state,
                                 "d_leaf_state": d_leaf_state})
        diff._tree, diff._epoch, diff._n_tree = self, self._updates, t["n"]
        return diff, None

    def apply_diff(self, diff: SnapshotDiff, admit_new: bool = False, zero_gone: bool = False):
        """Write the changed balances of `diff` into the tree in place and return the new root.  A device diff's balances are folded
        once more where the file's text lies and go through the update's kernels (sr_mst_apply_diff_dev): they never visit the
        host; only the list of changed leaves does, for the plan of the levels.  A host diff goes through `update_leaves_at`.
        With both keywords at their defaults new users are not inserted and gone users are not zeroed.
        zero_gone: every GONE leaf of the diff also gets zero balances.  Its username, its place and its entry in the name index
        stay: a lookup still finds it, `to_csv` writes it as name,0,0 and a later diff of the same file still calls it GONE, with
        nothing to change.  The liabilities leave the committed sums; the row stays until a rebuild drops it.  UNREACHABLE leaves
        are not touched.  Every tree and both ingests.
        admit_new: every NEW row of the diff also becomes a leaf, the j-th in the file's order leaf `diff.admitted[j]`, in the
        padding behind the named leaves: username and balances as `from_csv` makes them, from the text in HBM; a name twice among
        the new rows gets two leaves, the later one shadowed (`duplicate_names`).  The tree's text and name index in HBM grow by
        the names and the tree answers by name as a fresh tree of the same leaves would.  Needs a device diff of a tree in file
        order with a name index (`from_csv(name_index=True)`): a sorted tree's leaves are its order.
        With either keyword a device diff is settled by sa_mst_admit_measure_dev / sa_mst_settle_dev: changed, gone and admitted
        leaves in ONE run of the leaf and level kernels.
        ValueError, with the tree untouched: a diff taken of another tree, or of this tree before another update; admit_new on a
        sorted tree, a tree without a name index or a host diff; more new rows than `free_leaves` (the depth has to grow: the
        rebuild that really is due); a new row with a name of more than 64 bytes; a text in HBM that would reach 4 GiB; a diff whose
        `cap` left the list that is asked for incomplete."""
        import torch
        if diff._tree is not self:
            raise ValueError("a diff of another tree")
        if diff._epoch != self._updates:
            raise ValueError("a diff taken before another update of the tree")
        if admit_new:
            if diff.ingest != "device":
                raise ValueError("admit_new needs a device diff: the host's way admits nobody")
            if self._index_dev is None:
                raise ValueError("admit_new needs a tree in file order with a name index (from_csv(name_index=True)): "
                                 "a sorted tree's leaves are its order")
            if len(diff.new_rows) != diff.n_new:
                raise ValueError("the diff's cap left the list of new rows incomplete")
            if diff.admitted.stop > 1 << self.depth:
                raise ValueError(f"{diff.n_new} new users and {self.free_leaves} free leaves: the depth has to grow, a rebuild is due")
        if zero_gone and len(diff.gone) != diff.n_gone:
            raise ValueError("the diff's cap left the list of gone leaves incomplete")
        n_new, n_gone = diff.n_new if admit_new else 0, diff.n_gone if zero_gone else 0
        if diff.n_changed + n_new + n_gone == 0:
            return self.root()
        if diff.ingest != "device":
            zeros = [[0] * self.n_currencies] * n_gone
            return self.update_leaves_at(diff.changed.tolist() + diff.gone.tolist()[:n_gone], list(diff.new_balances) + zeros)
        d = diff._dev
        touched = diff.changed
        if admit_new or zero_gone:
            self._settle_dev(diff, n_new, n_gone)
            touched = np.sort(np.concatenate([diff.changed, diff.gone[:n_gone], np.array(diff.admitted[:n_new], dtype=np.uint32)]))
        else:
            ffi.check(ffi.rounds_lib().sr_mst_apply_diff_dev(ffi.dev_ptr(d["text"]), d["size"], d["body_off"], ffi.dev_ptr(d["d_spans"]), d["n"],
                                                             ffi.dev_ptr(d["d_owner"]), ffi.dev_ptr(d["d_changed"]), diff.n_changed, self.depth,
                                                             self.n_currencies, ffi.dev_ptr(self.d_users), ffi.dev_ptr(self.d_bals),
                                                             ffi.dev_ptr(self.d_h), ffi.dev_ptr(self.d_b), ffi.current_stream_ptr()))
        torch.cuda.current_stream().synchronize()             # for the constructor's reason, as _update_dev
        self._updates += 1
        self._root = None
        if self._csv_lazy is not None:                        # entries nobody has read yet: these leaves' balances are d_bals' now
            self._applied = tuple(self._applied) + (touched,)
            if self._csv_lazy[1]:
                for i in touched.tolist():
                    self._csv_lazy[1].pop(i, None)
        elif self._entries is not None:
            names = dict(zip(diff.admitted, self._names_of_leaves(diff.admitted.start, diff.admitted.stop))) if n_new else {}
            for i, bal in zip(touched.tolist(), self._balances_of_leaves(touched)):
                self._entries[i] = (names.get(i, self._entries[i][0]), bal)
        if n_new:
            self._name_index = None                           # update_leaves' own: names were added
        return self.root()

    def _settle_dev(self, diff: SnapshotDiff, n_new: int, n_gone: int):
        """sa_mst_admit_measure_dev (for new rows) and sa_mst_settle_dev on the current stream; every refusal comes before anything
        of the tree is written, and the new text and index replace the old ones only behind a settle that was accepted"""
        import torch
        A, d, t = ffi.admit_lib(), diff._dev, self._names_dev()
        nc, stream = self.n_currencies, ffi.current_stream_ptr()
        opt = lambda x: ffi.dev_ptr(x) if x is not None else None
        outs, d_scratch, name_bytes = {}, None, C.c_uint64(0)
        if n_new:
            scratch_bytes, problem = C.c_uint64(0), C.c_uint64(0)
            ffi.check(A.sa_mst_admit_scratch(d["n"], nc, n_new, C.byref(scratch_bytes)))
            d_scratch = torch.empty(scratch_bytes.value, dtype=torch.uint8, device="cuda")
            ffi.check(A.sa_mst_admit_measure_dev(ffi.dev_ptr(d["text"]), d["size"], d["body_off"], ffi.dev_ptr(d["d_spans"]), d["n"], nc,
                                                 ffi.dev_ptr(d["d_row_state"]), ffi.dev_ptr(d["d_new"]), n_new, t["n"], self.depth,
                                                 ffi.dev_ptr(d_scratch), C.byref(name_bytes), C.byref(problem), stream))
            if problem.value:
                torch.cuda.current_stream().synchronize()
                raise ValueError(f"row {problem.value >> 8}: {_CSV_ROW_PROBLEMS.get(problem.value & 0xff, 'a name of more than 64 bytes')}")
            if t["size"] - t["body_off"] + name_bytes.value >= 1 << 32:
                torch.cuda.current_stream().synchronize()
                raise ValueError("the tree's text would reach 4 GiB with the new names appended")
            pad, n_all = -t["body_off"] % 16, t["n"] + n_new      # the body on a 16-byte boundary, as the reader placed it
            i32 = lambda count: torch.empty(count, dtype=torch.int32, device="cuda")
            d_file = torch.empty(pad + t["size"] + name_bytes.value, dtype=torch.uint8, device="cuda")
            # file_size: where the source file's own text ends; the rows are read up to there, the names behind it through spans
            outs = {"text": d_file[pad:], "size": t["size"] + name_bytes.value, "file_size": t.get("file_size", t["size"]), "n": n_all,
                    "d_order": i32(n_all), "d_name_spans": i32(2 * n_all), "d_leaf_name_spans": i32(2 * n_all)}
        index = t if n_new else {}
        ffi.check(A.sa_mst_settle_dev(ffi.dev_ptr(d["text"]), d["size"], d["body_off"], ffi.dev_ptr(d["d_spans"]), d["n"], nc,
                                      ffi.dev_ptr(d["d_owner"]), ffi.dev_ptr(d["d_leaf_state"]), ffi.dev_ptr(d["d_changed"]), diff.n_changed,
                                      opt(d["d_gone"]) if n_gone else None, n_gone, opt(d["d_new"]) if n_new else None, n_new,
                                      opt(d_scratch), opt(index.get("text")), index.get("size", 0), index.get("body_off", 0),
                                      opt(index.get("d_name_spans")), opt(index.get("d_order")), opt(index.get("d_leaf_name_spans")), t["n"],
                                      self.depth, opt(outs.get("text")), name_bytes.value, opt(outs.get("d_name_spans")),
                                      opt(outs.get("d_order")), opt(outs.get("d_leaf_name_spans")), ffi.dev_ptr(self.d_users),
                                      ffi.dev_ptr(self.d_bals), ffi.dev_ptr(self.d_h), ffi.dev_ptr(self.d_b), stream))
        if n_new:
            self._index_dev = dict(t, **outs)

    def apply_csv(self, path: str, cap=None, admit_new: bool = False, zero_gone: bool = False) -> SnapshotDiff:
        """`diff_csv` followed by `apply_diff`; returns the diff"""
        diff = self.diff_csv(path, cap)
        self.apply_diff(diff, admit_new=admit_new, zero_gone=zero_gone)
        return diff

    def _csv_body_on_device(self, delimiter=None):
        """-> (the body as a uint8 device tensor, None), or (None, why the device does not write this tree)"""
        import torch
        t = self._names_dev()
        if t is None:
            return None, "the tree holds no name index"
        delim = _csv_delimiter(t["delim"] if delimiter is None else delimiter)
        X = ffi.export_lib()
        n, nc, stream = t["n"], self.n_currencies, ffi.current_stream_ptr()
        leaf_spans = t.get("d_leaf_name_spans", t["d_name_spans"])     # a sorted tree's sorted spans are its leaves'
        scratch_bytes, body_bytes = C.c_uint64(0), C.c_uint64(0)
        ffi.check(X.sx_mst_csv_scratch(n, C.byref(scratch_bytes)))
        d_row_off = torch.empty(n, dtype=torch.int32, device="cuda")
        d_scratch = torch.empty(scratch_bytes.value // 4, dtype=torch.int32, device="cuda")
        ffi.check(X.sx_mst_csv_measure_dev(ffi.dev_ptr(t["text"]), t["size"], t["body_off"], ffi.dev_ptr(leaf_spans), n, nc,
                                           ffi.dev_ptr(self.d_bals), ffi.dev_ptr(d_row_off), ffi.dev_ptr(d_scratch), C.byref(body_bytes),
                                           stream))
        if body_bytes.value >= 1 << 32:
            return None, "a body of 4 GiB or more"
        d_out = torch.empty(body_bytes.value, dtype=torch.uint8, device="cuda")
        ffi.check(X.sx_mst_csv_write_dev(ffi.dev_ptr(t["text"]), t["size"], t["body_off"], ffi.dev_ptr(leaf_spans), n, nc,
                                         ffi.dev_ptr(self.d_bals), ord(delim), ffi.dev_ptr(d_row_off), body_bytes.value, ffi.dev_ptr(d_out),
                                         stream))
        return d_out, None

    def csv_body_dev(self, delimiter=None):
        """The body of `to_csv` -- every row behind the header line -- as a uint8 device tensor, made where the tree lies
        (sx_mst_csv_measure_dev, sx_mst_csv_write_dev) and enqueued on the current stream: the names from the text the tree keeps
        in HBM, the balances from `d_bals` as they are now in that stream's order.  The measure waits for the stream once, for the
        body's length.  delimiter: the tree's own unless given.  ValueError for a tree without the names' order in HBM
        (`has_name_index`) and for a body of 4 GiB or more."""
        body, reason = self._csv_body_on_device(delimiter)
        if body is None:
            raise ValueError(reason)
        return body

    def to_csv(self, path: str, cryptocurrencies=None, delimiter=None) -> CsvExport:
        """The snapshot CSV this tree commits to NOW, after any `update_leaves*`, `apply_diff` or `apply_csv` (_Tree.to_csv has
        the text's rules).  A tree with the names' order in HBM (`has_name_index`: `from_csv_sorted`, `from_csv(name_index=True)`)
        writes it where it lies: the header line on the host, `csv_body_dev`, one copy, one write.  That way parses no file and
        reads nothing the host keeps of earlier updates: the balances are `d_bals`' and the names the text's.  A sorted tree is
        written sorted, a tree in file order in file order, each with its own delimiter unless one is given; an un-updated tree in
        file order gives a canonical source file (line ends "\\n", a final one, no leading zeros, values below r) back byte for
        byte.  Any other tree goes the host's way, over `entries`, and the result says why (`ingest`, `fallback_reason`); there the
        delimiter is that of the source file where the device read it, else ",", unless one is given.
        A padding leaf given non-zero balances by `update_leaves_at` has no name and is not written: the file then reads back
        to another root."""
        t = self._names_dev()
        if t is not None:                                     # refused before any device work
            delimiter = _csv_delimiter(t["delim"] if delimiter is None else delimiter)
            header = _csv_header(cryptocurrencies or self.cryptocurrencies, self.n_currencies, delimiter).encode()
        body, reason = self._csv_body_on_device(delimiter)
        if body is None:
            done = super().to_csv(path, cryptocurrencies, self._csv_delim if delimiter is None else delimiter)
            done.fallback_reason = reason
            return done
        data = body.cpu().numpy()
        with open(path, "wb") as f:
            f.write(header)
            data.tofile(f)
        return CsvExport(self._names_dev()["n"], len(header) + data.size, "device")

    def _balances_of_leaves(self, leaves):
        """the balances of some leaves as integers from their rows of `d_bals`: one gather and one copy"""
        import torch
        nc = self.n_currencies
        at = torch.as_tensor(np.asarray(leaves, dtype=np.int64), device="cuda")
        rows = self.d_bals.view(-1, 32 * nc)[at].cpu().numpy()
        return [[_mont_to_int(row[32 * c:32 * c + 32]) for c in range(nc)] for row in rows]

    def range_audit(self, n_bytes: int = 8, cap=None) -> RangeAudit:
        """Which users of this snapshot can receive a valid inclusion proof from a circuit of `n_bytes`: one device call
        (ss_mst_range_audit_dev) on the current stream over `d_b`, one small copy for the summary and one for the list.  cap: list
        at most that many unprovable leaves (None: all).  The result describes the tree as it is now: after `update_leaves*` it
        is stale, and running the audit again is the remedy."""
        import torch
        if not 1 <= n_bytes <= 31:
            raise ValueError("n_bytes outside 1..31")
        if cap is not None and cap < 0:
            raise ValueError("cap below 0")
        S = ffi.snapshot_lib()
        leaves = 1 << self.depth
        bad_cap = leaves if cap is None else min(int(cap), leaves)
        scratch_bytes = C.c_uint64(0)
        ffi.check(S.ss_mst_range_audit_scratch(self.depth, C.byref(scratch_bytes)))
        d_flags = torch.empty(2 * leaves - 1, dtype=torch.uint8, device="cuda")
        d_reasons = torch.empty(leaves, dtype=torch.int32, device="cuda")
        d_bad = torch.empty(bad_cap, dtype=torch.int32, device="cuda") if bad_cap else None
        d_scratch = torch.empty(scratch_bytes.value // 4, dtype=torch.int32, device="cuda")
        summary = (C.c_uint64 * 4)()
        ffi.check(S.ss_mst_range_audit_dev(ffi.dev_ptr(self.d_b), self.depth, self.n_currencies, n_bytes, ffi.dev_ptr(d_flags),
                                           ffi.dev_ptr(d_reasons), ffi.dev_ptr(d_bad) if bad_cap else None, bad_cap,
                                           ffi.dev_ptr(d_scratch), summary, ffi.current_stream_ptr()))
        listed = int(summary[2])
        bad = d_bad[:listed].cpu().numpy().view(np.uint32) if listed else np.zeros(0, dtype=np.uint32)
        return RangeAudit(n_bytes, summary[0], summary[1], bad, int(summary[3]), d_flags, d_reasons)

    def duplicate_names(self, cap=None) -> DuplicateNames:
        """The usernames that occur more than once.  A tree with the names' order in HBM (`has_name_index`) answers from there in
        one device call (ss_mst_duplicate_names_dev) on the current stream, one small copy for the summary and one for each list,
        and parses nothing; any other tree answers from `entries` on the host.  cap: list at most that many shadowed leaves
        (None: all).  Updates never change names, so the report holds until `apply_diff(admit_new=True)` adds some."""
        import torch
        d = self._names_dev()
        if d is None:
            return super().duplicate_names(cap)
        if cap is not None and cap < 0:
            raise ValueError("cap below 0")
        S = ffi.snapshot_lib()
        n = d["n"]
        list_cap = n if cap is None else min(int(cap), n)
        scratch_bytes = C.c_uint64(0)
        ffi.check(S.ss_mst_duplicate_names_scratch(n, C.byref(scratch_bytes)))
        d_scratch = torch.empty(scratch_bytes.value // 4, dtype=torch.int32, device="cuda")
        d_shadowed = torch.empty(list_cap, dtype=torch.int32, device="cuda") if list_cap else None
        d_first = torch.empty(list_cap, dtype=torch.int32, device="cuda") if list_cap else None
        summary = (C.c_uint64 * 3)()
        ffi.check(S.ss_mst_duplicate_names_dev(ffi.dev_ptr(d["text"]), d["size"], d["body_off"], ffi.dev_ptr(d["d_name_spans"]),
                                               None if self._sorted_dev is not None else ffi.dev_ptr(d["d_order"]), n,
                                               ffi.dev_ptr(d_shadowed) if list_cap else None, ffi.dev_ptr(d_first) if list_cap else None,
                                               list_cap, ffi.dev_ptr(d_scratch), summary, ffi.current_stream_ptr()))
        listed = int(summary[2])
        take = lambda t: t[:listed].cpu().numpy().view(np.uint32) if listed else np.zeros(0, dtype=np.uint32)
        return DuplicateNames(summary[0], summary[1], take(d_shadowed), take(d_first))

    def _name_of_leaf(self, index: int):
        return self._entry_from_text(index)[0] if self._finds_on_device() else self.entries[index][0]

    def explain_unprovable(self, audit: RangeAudit, index: int):
        """What is wrong with user `index`: [(what, level, node, currency, value)] for every balance >= 2^(8 audit.n_bytes) that the
        circuit of that user range-checks, in the circuit's order -- what: "leaf" (the user's own) or "sibling" (node `node` of
        level `level` on the path); value: the balance as an integer.  Only the flagged nodes' rows are fetched.  [] for a
        provable user.  `audit` must be of this tree as it is now."""
        checks = audit.checks_of(index, int(audit.reasons([index])[0]))
        if not checks:
            return []
        nc, top = self.n_currencies, 1 << (8 * audit.n_bytes)
        _, rows, _, _ = self._rows([], [self.offsets[level] + node for _, level, node in checks], [])
        out = []
        for (what, level, node), row in zip(checks, rows):
            values = [_mont_to_int(row[32 * c:32 * c + 32]) for c in range(nc)]
            out += [(what, level, node, c, v) for c, v in enumerate(values) if v >= top]
        return out

    def _rows(self, hash_nodes, balance_nodes, users):
        """one gather + one copy: rows of the hash array, of the balance array (n_currencies rows per node), leaf inputs"""
        import torch
        nc = self.n_currencies
        dev = lambda idx: torch.tensor(idx, dtype=torch.int64, device="cuda")
        parts = [self.d_h.view(-1, 32)[dev(hash_nodes)].reshape(-1) if hash_nodes else None,
                 self.d_b.view(-1, 32 * nc)[dev(balance_nodes)].reshape(-1) if balance_nodes else None,
                 self.d_users.view(-1, 32)[dev(users)].reshape(-1) if users else None,
                 self.d_bals.view(-1, 32 * nc)[dev(users)].reshape(-1) if users else None]
        flat = torch.cat([p for p in parts if p is not None]).cpu().numpy()
        out, pos = [], 0
        for p, width in zip(parts, (32, 32 * nc, 32, 32 * nc)):
            count = 0 if p is None else p.numel() // width
            out.append([flat[pos + width * i:pos + width * (i + 1)] for i in range(count)])
            pos += width * count
        return out

    def root(self):
        if self._root is None:
            h, b, _, _ = self._rows([self.offsets[self.depth]], [self.offsets[self.depth]], [])
            self._root = (h[0], b[0])
        return self._root

    def public_inputs(self, index: int):
        """[leaf hash, root hash, root balances..] of user `index` as integers: `circuit.instances()[0]`"""
        return self.public_inputs_many([index])[0]

    def public_inputs_many(self, indices):
        """`public_inputs` of several users with one gather and one copy"""
        if any(not 0 <= i < (1 << self.depth) for i in indices):
            raise IndexError("Index out of bounds")
        h, _, _, _ = self._rows([int(i) for i in indices], [], [])
        rh, rb = self.root()
        tail = [_mont_to_int(rh)] + [_mont_to_int(rb[32 * c:32 * c + 32]) for c in range(self.n_currencies)]
        return [[_mont_to_int(row)] + tail for row in h]

    def generate_proof(self, index: int):
        """the fields of the reference's MerkleProof (see MerkleSumTree.generate_proof); `entry` carries the username as
        its field element (int) where the snapshot holds no names, and the entry itself (name, integer balances) where the
        tree was built from entries"""
        path = self._path(index)
        hash_nodes, bal_nodes = [self.offsets[0] + index], []
        for level, (_, sib) in enumerate(path):
            if level > 0:   # the sibling middle node's preimage: its balances, its children's hashes
                bal_nodes.append(self.offsets[level] + sib)
                hash_nodes += [self.offsets[level - 1] + 2 * sib, self.offsets[level - 1] + 2 * sib + 1]
        h, b, users, bals = self._rows(hash_nodes, bal_nodes, [index, index ^ 1] if self.depth else [index])
        nc = self.n_currencies
        entry = (_mont_to_int(users[0]), [_mont_to_int(bals[0][32 * c:32 * c + 32]) for c in range(nc)])
        if self._finds_on_device():
            entry = self._entry_from_text(index)
        elif self.entries is not None:
            entry = self.entries[index]
        pre_mid = [np.concatenate([b[l], h[1 + 2 * l], h[2 + 2 * l]]) for l in range(max(0, self.depth - 1))]
        pre_leaf = np.concatenate([users[1], bals[1]]) if self.depth else None
        return {"entry": entry, "leaf": (h[0], bals[0]), "path_indices": [bit for bit, _ in path], "root": self.root(),
                "sibling_leaf_node_hash_preimage": pre_leaf, "sibling_middle_node_hash_preimages": pre_mid}
