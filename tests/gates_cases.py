"""The gate compiler's corpus and an independent reading of what it emits (no GPU): the graphs whose lowering
tests/golden/gates_lowering.json pins, their text form for tests/cpp/gates_compile_check.cpp, a restatement of the interpreter's
tile rule, and a Python interpreter of the ten opcodes over integers mod r that re-derives the operand bounds on the way."""
import ctypes as C
import hashlib

import numpy as np

from circuits_halo2_amd import arithmetic as A

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
OPCODES = ["loadcol", "loadprev", "add", "sub", "mul", "sqr", "dbl", "neg", "red", "muladd"]
LOADCOL, LOADPREV, G_ADD, G_SUB, G_MUL, G_SQR, G_DBL, G_NEG, G_RED, G_MULADD = range(10)
SLOT, CONST = 0, 1
NO_B = (0, 0, 0)


# ----------------------------------------------------------------------------- graphs
class RawGraph:
    """an sg_graph as plain lists, faults included (GraphEvaluator cannot express them): calcs = (op, a, b, parts_offset,
    parts_len), value sources = (kind, index, rotation index); `null` names the arrays handed over as null pointers"""

    def __init__(self, n_constants=0, rotations=(), calcs=(), parts=(), null=()):
        self.n_constants, self.rotations, self.calcs, self.parts, self.null = n_constants, list(rotations), list(calcs), list(parts), set(null)

    @classmethod
    def of(cls, g):
        calcs, parts = [], []
        for cal in g.calculations:
            own = cal[3] if len(cal) > 3 else []
            calcs.append((cal[0], cal[1], cal[2], len(parts) if own else 0, len(own)))
            parts.extend(own)
        return cls(len(g.constants), g.rotations, calcs, parts)

    def _struct(self):   # what circuits_halo2_amd.arithmetic hands to the library
        consts = np.zeros(32 * max(1, self.n_constants), np.uint8)
        rots = np.asarray(self.rotations or [0], dtype=np.int32)
        calcs = (A._Calc * max(1, len(self.calcs)))()
        for i, (op, a, b, off, n) in enumerate(self.calcs):
            calcs[i].op, calcs[i].a, calcs[i].b, calcs[i].parts_offset, calcs[i].parts_len = op, A._VS(*a), A._VS(*b), off, n
        parr = (A._VS * max(1, len(self.parts)))(*[A._VS(*p) for p in self.parts])
        at = lambda name, p: None if name in self.null else p
        g = A._Graph(at("constants", consts.ctypes.data), self.n_constants, at("rotations", rots.ctypes.data), len(self.rotations),
                     at("calculations", C.addressof(calcs)), len(self.calcs), at("parts", C.addressof(parr)), len(self.parts))
        return g, (consts, rots, calcs, parr)

    def as_dict(self, constants):
        """the form oracle.pyref.eval_graph reads, with `constants` as the table's values"""
        return {"constants": list(constants), "rotations": self.rotations,
                "calculations": [(op, a, b, self.parts[off:off + n]) for op, a, b, off, n in self.calcs]}


class Case:
    def __init__(self, name, graph, n_fixed, n_advice, n_instance, n_challenges):
        self.name, self.n_fixed, self.n_advice, self.n_instance, self.n_challenges = name, n_fixed, n_advice, n_instance, n_challenges
        self.graph = graph if isinstance(graph, RawGraph) else RawGraph.of(graph)

    @property
    def dims(self):
        return self.n_fixed, self.n_advice, self.n_instance, self.n_challenges

    def line(self, command="words", reload_distance=12, convert_above=-1):
        """one request of tests/cpp/gates_compile_check.cpp"""
        g = self.graph
        null = sum(1 << i for i, n in enumerate(("constants", "rotations", "calculations", "parts")) if n in g.null)
        ints = [*self.dims, reload_distance, convert_above, g.n_constants, len(g.rotations), len(g.calcs), len(g.parts), null, *g.rotations]
        for op, a, b, off, n in g.calcs:
            ints += [op, *a, *b, off, n]
        for p in g.parts:
            ints += p
        return command + " " + " ".join(map(str, ints))


def random_graph(rng, n_fixed, n_advice, n_instance, n_chal, n_calc, O):
    """a random, valid GraphEvaluator program that exercises every calculation and value source"""
    from conftest import fr_np
    g = A.GraphEvaluator()
    consts = [g.add_constant(O.random_fr(int(rng.integers(1 << 30)), 1)) for _ in range(3)]
    consts.append(g.add_constant(fr_np([0])))
    consts.append(g.add_constant(fr_np([1])))
    rots = [0, 1, -1, 2, -5]

    def src(upto):
        kind = int(rng.integers(0, 8))
        if kind == 0:
            return consts[int(rng.integers(len(consts)))]
        if kind in (1, 2) and upto:
            return (A.INTERMEDIATE, int(rng.integers(max(0, upto - 6), upto)), 0)   # mostly recent values
        if kind == 3 and n_fixed:
            return g.query(A.FIXED, int(rng.integers(n_fixed)), rots[int(rng.integers(len(rots)))])
        if kind == 4 and n_instance:
            return g.query(A.INSTANCE, int(rng.integers(n_instance)), rots[int(rng.integers(2))])
        if kind == 5 and n_chal:
            return (A.CHALLENGE, int(rng.integers(n_chal)), 0)
        if kind == 6:
            return (int(rng.choice([A.BETA, A.GAMMA, A.THETA, A.Y, A.PREVIOUS_VALUE])), 0, 0)
        return g.query(A.ADVICE, int(rng.integers(n_advice)), rots[int(rng.integers(len(rots)))])

    while len(g.calculations) < n_calc:
        q = len(g.calculations)
        op = int(rng.choice([A.ADD, A.ADD, A.SUB, A.SUB, A.MUL, A.MUL, A.SQUARE, A.DOUBLE, A.NEGATE, A.HORNER, A.STORE]))
        if op == A.HORNER:
            g.add_calculation(op, src(q), src(q), [src(q) for _ in range(int(rng.integers(0, 5)))])
        elif op in (A.SQUARE, A.DOUBLE, A.NEGATE, A.STORE):
            g.add_calculation(op, src(q))
        else:
            g.add_calculation(op, src(q), src(q))
    return g


def long_lazy_chain():
    """sums of 200 terms with alternating subtractions, negations and doublings (test_quotient_gates_bounds_and_slots)"""
    g = A.GraphEvaluator()
    acc = g.query(A.ADVICE, 0, 0)
    for i in range(200):
        term = g.query(A.ADVICE, i % 40, (i % 3) - 1)
        acc = g.add_calculation([A.ADD, A.SUB, A.ADD, A.SUB][i % 4], acc, term)
        if i % 17 == 0:
            acc = g.add_calculation(A.DOUBLE, acc)
        if i % 23 == 0:
            acc = g.add_calculation(A.NEGATE, acc)
    g.add_calculation(A.MUL, acc, acc)
    return g


def lifo_chain(n):
    """n squared loads, consumed last-in-first-out: n values live at once"""
    g = A.GraphEvaluator()
    loads = [g.add_calculation(A.SQUARE, g.query(A.ADVICE, i, 0)) for i in range(n)]
    acc = loads[-1]
    for v in reversed(loads[:-1]):
        acc = g.add_calculation(A.MUL, acc, v)
    return g


def many_live_values(n):
    """n computed values, each used twice, far apart: n + 1 values live at once (the emission is demand-driven: values that are
    merely consumed in reverse order, as in lifo_chain, are computed when they are needed and never wait).  With n = 70
    (test_quotient_gates_errors) it compiles, and the ABI refuses it"""
    g = A.GraphEvaluator()
    xs = [g.add_calculation(A.SQUARE, g.query(A.ADVICE, 0, i - 35)) for i in range(n)]
    acc = xs[0]
    for v in xs[1:]:
        acc = g.add_calculation(A.MUL, acc, v)
    for v in reversed(xs):
        acc = g.add_calculation(A.ADD, g.add_calculation(A.MUL, acc, v), v)
    return g


def square_chain(depth):
    adv = (A.ADVICE, 0, 0)
    return RawGraph(0, [0], [(A.SQUARE, adv, NO_B, 0, 0)] + [(A.SQUARE, (A.INTERMEDIATE, i, 0), NO_B, 0, 0) for i in range(depth - 1)])


RANDOM_SEEDS = [(seed, n_calc, ni, nch) for n_calc in (1, 8, 40, 120, 300) for seed, (ni, nch) in
                enumerate([(1, 2), (0, 2), (1, 0), (0, 0), (1, 2), (0, 0), (1, 2), (1, 2)], start=10 * n_calc)]
INTERPRETER_TILE_PROGRAMS = {256: 7, 128: 19, 64: 39}   # rows per workgroup: the n of a many_live_values(n) that gets them (n + 1 slots)

_corpus = None


def corpus(O):
    """every named graph of tests/golden/gates_lowering.json, in its order"""
    global _corpus
    if _corpus is not None:
        return _corpus
    from circuits_halo2_amd import mst_inclusion as M
    adv, adv1, c0 = (A.ADVICE, 0, 0), (A.ADVICE, 1, 0), (A.CONSTANT, 0, 0)
    it = lambda i: (A.INTERMEDIATE, i, 0)
    one = lambda calcs, parts=(), n_constants=1, **kw: RawGraph(n_constants, [0], calcs, parts, **kw)
    cases = [Case(f"mst_gates_nc{nc}", M.gate_graph(nc), M.NUM_FIXED, M.NUM_ADVICE, 0, len(M.gate_challenge_exponents(nc))) for nc in (1, 2, 3, 4)]
    cases.append(Case("mst_lookup_input", M.lookup_input_graph(), M.NUM_FIXED, M.NUM_ADVICE, 1, 0))
    for seed, n_calc, ni, nch in RANDOM_SEEDS:
        g = random_graph(np.random.default_rng(seed), 3, 4, ni, nch, n_calc, O)
        cases.append(Case(f"random_seed{seed}_calc{n_calc}_inst{ni}_chal{nch}", g, 3, 4, ni, nch))
    cases.append(Case("long_lazy_chain", long_lazy_chain(), 0, 40, 0, 0))
    cases.append(Case("lifo_chain_40", lifo_chain(40), 0, 40, 0, 0))
    cases += [Case(f"live_values_{n}", many_live_values(n), 0, 1, 0, 0) for n in (70, *INTERPRETER_TILE_PROGRAMS.values())]
    cases.append(Case("horner_without_parts", one([(A.HORNER, adv, adv1, 0, 0)]), 0, 2, 0, 0))
    cases.append(Case("result_constant", one([(A.STORE, c0, NO_B, 0, 0)]), 0, 1, 0, 0))
    cases.append(Case("result_column", one([(A.STORE, adv, NO_B, 0, 0)]), 0, 1, 0, 0))
    cases.append(Case("result_previous_value", one([(A.STORE, (A.PREVIOUS_VALUE, 0, 0), NO_B, 0, 0)]), 0, 1, 0, 0))
    # one graph per message
    cases.append(Case("error_empty", one([]), 0, 1, 0, 0))
    cases.append(Case("error_null_rotations", one([(A.SQUARE, adv, NO_B, 0, 0)], null=["rotations"]), 0, 1, 0, 0))
    cases.append(Case("error_null_calculations", one([(A.SQUARE, adv, NO_B, 0, 0)], null=["calculations"]), 0, 1, 0, 0))
    cases.append(Case("error_null_constants", one([(A.SQUARE, adv, NO_B, 0, 0)], null=["constants"]), 0, 1, 0, 0))
    cases.append(Case("error_null_parts", one([(A.HORNER, adv, adv, 0, 1)], [adv], null=["parts"]), 0, 1, 0, 0))
    cases.append(Case("error_65537_calculations", one([(A.STORE, c0, NO_B, 0, 0)] * 65537), 0, 1, 0, 0))
    cases.append(Case("error_forward_reference", one([(A.ADD, it(0), adv, 0, 0)]), 0, 1, 0, 0))
    cases.append(Case("error_forward_reference_unreached", one([(A.NEGATE, it(1), NO_B, 0, 0), (A.SQUARE, adv, NO_B, 0, 0), (A.SQUARE, adv1, NO_B, 0, 0)]), 0, 2, 0, 0))
    cases.append(Case("error_forward_reference_in_parts", one([(A.HORNER, adv, adv, 0, 2)], [adv, it(0)]), 0, 1, 0, 0))
    cases.append(Case("error_horner_parts_out_of_range", one([(A.HORNER, adv, adv, 1, 2)], [adv, adv]), 0, 1, 0, 0))
    cases.append(Case("error_forward_reference_before_parts_range", one([(A.HORNER, adv, it(3), 1, 2)], [adv, adv]), 0, 1, 0, 0))
    cases.append(Case("error_constant_index", one([(A.ADD, (A.CONSTANT, 1, 0), adv, 0, 0)]), 0, 1, 0, 0))
    cases.append(Case("error_column_index", one([(A.ADD, adv1, adv, 0, 0)]), 0, 1, 0, 0))
    cases.append(Case("error_rotation_index", one([(A.ADD, (A.ADVICE, 0, 1), adv, 0, 0)]), 0, 1, 0, 0))
    cases.append(Case("error_instance_index", one([(A.SQUARE, (A.INSTANCE, 0, 0), NO_B, 0, 0)]), 1, 1, 0, 0))
    cases.append(Case("error_challenge_index", one([(A.SQUARE, (A.CHALLENGE, 2, 0), NO_B, 0, 0)]), 0, 1, 0, 2))
    cases.append(Case("error_value_source", one([(A.SQUARE, (11, 0, 0), NO_B, 0, 0)]), 0, 1, 0, 0))
    cases.append(Case("error_calculation", one([(8, adv, NO_B, 0, 0)]), 0, 1, 0, 0))
    cases.append(Case("error_last_fault_is_reported", one([(A.ADD, (A.CONSTANT, 1, 0), (A.CHALLENGE, 0, 0), 0, 0)]), 0, 1, 0, 0))
    cases.append(Case("error_constant_operand_above_65535", one([(A.MUL, adv, adv1, 0, 0), (A.ADD, it(0), (A.CONSTANT, 65536, 0), 0, 0)],
                                                                n_constants=65537), 0, 2, 0, 0))
    # a fault only where the result never looks
    cases.append(Case("unreached_constant_index", one([(A.ADD, (A.CONSTANT, 9, 0), adv, 0, 0), (A.SQUARE, adv, NO_B, 0, 0)]), 0, 1, 0, 0))
    cases.append(Case("unreached_calculation_and_column", one([(99, (A.FIXED, 7, 3), NO_B, 0, 0), (A.DOUBLE, adv, NO_B, 0, 0)]), 0, 1, 0, 0))
    cases.append(Case("depth_4096", square_chain(4096), 0, 1, 0, 0))
    cases.append(Case("error_depth_4097", square_chain(4097), 0, 1, 0, 0))
    assert len({c.name for c in cases}) == len(cases)
    _corpus = cases
    return cases


def digest(words):
    return hashlib.sha256(np.asarray(words, dtype="<u4").tobytes()).hexdigest()


def library_lowering(case):
    """{"sha256": ...} or {"error": ...} of a case through the built library (arithmetic.gates_program_words)"""
    from circuits_halo2_amd.ffi import SummaGpuError
    try:
        return {"sha256": digest(A.gates_program_words(case.graph, *case.dims))}
    except SummaGpuError as e:
        return {"error": str(e).split("sg_gates_program_words: ", 1)[1]}


# ----------------------------------------------------------------------------- the interpreter's tile, restated
LDS_BUDGET, LDS_PER_CU, LIMB_BYTES = 144 * 1024, 160 * 1024, 36


def interpreter_tile(n_slots, n_consts):
    """(rows per workgroup, dynamic LDS bytes, fits, waves per CU by LDS): the shape that keeps the most waves per CU, and among
    shapes within one wave of each other the larger workgroup"""
    consts = n_consts * LIMB_BYTES
    rows, best = 256, 0
    for t in (256, 128, 64):
        need = consts + n_slots * t * LIMB_BYTES
        if need > LDS_BUDGET:
            continue
        waves = min(32, LDS_PER_CU // need * (t // 64))
        if best == 0 or waves > best + 1:
            rows, best = t, waves
    lds = consts + n_slots * rows * LIMB_BYTES
    return rows, lds, lds <= LDS_BUDGET, best


# with the four constants every program has, plus one, by hand: a workgroup of T rows and s slots needs 180 + 36 s T bytes, a CU
# holds floor(163840 / that) of them, i.e. that many times T / 64 waves (at most 32).  256 rows are left only for a shape two waves
# ahead: 128 rows are at 3 slots (22 waves against 20), 5 .. 7 (14 : 12, 10 : 8, 10 : 8) and 9 .. 11 (6 : 4); 64 rows never are.
# From 16 slots on 256 rows do not fit, from 32 on 128 rows do not; 64 slots of 64 rows are the whole budget, so nothing is left
# for the constants.
TILE_ROWS_AT_5_CONSTANTS = {256: [1, 2, 4, 8, 12, 13, 14, 15], 128: [3, 5, 6, 7, 9, 10, 11, *range(16, 32)], 64: [*range(32, 64)], None: [64]}


# ----------------------------------------------------------------------------- an independent reading of the lowered words
def decode(words):
    n_slots, result_kind, result_index, n_ops = words[:4]
    assert len(words) == 4 + 4 * n_ops
    ops = []
    for i in range(n_ops):
        w0, dst, a, b = words[4 + 4 * i: 8 + 4 * i]
        ops.append({"code": w0 & 0xff, "kidx": (w0 >> 8) & 0xff, "ak": (w0 >> 16) & 0xff, "bk": w0 >> 24, "dst": dst & 0xffff, "c": dst >> 16,
                    "a": a, "b": b if b < 1 << 31 else b - (1 << 32)})
    return n_slots, result_kind, result_index, ops


def run_program(words, consts, column, previous):
    """the program's result over integers mod r.  consts: the constant table; column(index, rotation) -> value of fixed ++ advice
    ++ instance.  Re-derives every operand's bound by the compiler's rules and asserts them, and that a slot is written before
    it is read and lies below n_slots.  Returns (value, largest bound met)."""
    n_slots, result_kind, result_index, ops = decode(words)
    assert n_slots >= 1
    slot = [None] * n_slots       # (value, bound)
    top = 2

    def get(kind, idx):
        if kind == CONST:
            return consts[idx] % R, 2
        assert kind == SLOT and idx < n_slots and slot[idx] is not None, ("slot read before it is written, or out of range", idx)
        return slot[idx]

    for pc, o in enumerate(ops):
        code, kidx = o["code"], o["kidx"]
        if code == LOADCOL:
            assert kidx in (0, 1)
            r = column(o["a"], o["b"]) % R, (2 if kidx else 32)
        elif code == LOADPREV:
            r = previous % R, 32
        else:
            (x, bx), (y, by) = get(o["ak"], o["a"]), get(o["bk"], o["b"])
            if code == G_ADD:
                r = (x + y) % R, bx + by
            elif code == G_SUB:
                assert kidx <= 5 and by <= 2 << kidx, (pc, "subtrahend bound", by, kidx)
                r = (x - y) % R, bx + (2 << kidx)
            elif code == G_MUL:
                assert bx * by <= 170, (pc, "product bound", bx, by)
                r = x * y % R, 2
            elif code == G_SQR:
                assert bx * bx <= 170, (pc, "square bound", bx)
                r = x * x % R, 2
            elif code == G_DBL:
                r = 2 * x % R, 2 * bx
            elif code == G_NEG:
                assert kidx <= 5 and bx <= 2 << kidx, (pc, "negated bound", bx, kidx)
                r = -x % R, 2 << kidx
            elif code == G_RED:
                r = x, 2
            else:
                assert code == G_MULADD and bx * by <= 170, (pc, "product bound", bx, by)
                z, bz = get(kidx, o["c"])
                r = (x * y + z) % R, 2 + bz
        assert o["dst"] < n_slots
        slot[o["dst"]] = r
        top = max(top, r[1])
    return get(result_kind, result_index)[0], top
