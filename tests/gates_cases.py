"""The gate compiler's corpus and an independent reading of what it emits (no GPU): the graphs whose lowering
tests/golden/gates_lowering.json pins, their text form for tests/cpp/gates_compile_check.cpp, a restatement of the interpreter's
tile rule, and a Python interpreter of the ten opcodes over integers mod r that re-derives the operand bounds on the way.
Below that the device corpus (what tests/test_gpu_gates_edges.py runs: those graphs and hand-written ones at the compiler's bounds,
rotations beyond the domain, the LDS budget and the blob ring's slot size), the word patterns, the rows expected of the device by
the C oracle and by halo2's definition in Python integers, and the device's lazy arithmetic replayed in integers."""
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

    def _struct(self, constants=None):   # what circuits_halo2_amd.arithmetic hands to the library (constants: n_constants x 32 B, else zeros)
        consts = np.zeros(32 * max(1, self.n_constants), np.uint8)
        if constants is not None:
            assert constants.size == 32 * self.n_constants
            consts[:constants.size] = constants
        if getattr(self, "_arrays", None) is None or self._arrays[0] != (len(self.calcs), len(self.parts)):   # (the large graphs: built once)
            rots = np.asarray(self.rotations or [0], dtype=np.int32)
            calcs = (A._Calc * max(1, len(self.calcs)))()
            for i, (op, a, b, off, n) in enumerate(self.calcs):
                calcs[i].op, calcs[i].a, calcs[i].b, calcs[i].parts_offset, calcs[i].parts_len = op, A._VS(*a), A._VS(*b), off, n
            parr = (A._VS * max(1, len(self.parts)))(*[A._VS(*p) for p in self.parts])
            self._arrays = ((len(self.calcs), len(self.parts)), rots, calcs, parr)
        _, rots, calcs, parr = self._arrays
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


def run_program(words, consts, column, previous, trace=None):
    """the program's result over integers mod r.  consts: the constant table; column(index, rotation) -> value of fixed ++ advice
    ++ instance.  Re-derives every operand's bound by the compiler's rules and asserts them, and that a slot is written before
    it is read and lies below n_slots.  Returns (value, largest bound met).  trace: a list that receives, per instruction,
    (opcode, kidx, bound of a, bound of b, bound of a G_MULADD's addend, bound of the result), None where there is none."""
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
        bx = by = bz = None
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
        if trace is not None:
            trace.append((code, kidx, bx, by, bz, r[1]))
    return get(result_kind, result_index)[0], top


# ============================================================================= the device corpus
# What the GPU tests of the gate evaluator run (tests/test_gpu_gates_edges.py) and what tests/test_gates_cases_cpu.py checks
# without one: every graph of corpus() that lowers, and hand-written graphs named after what they reach.
class _Build:
    """a RawGraph written by hand: nothing is deduplicated, every constant is a table entry of its own"""

    def __init__(self):
        self.n_constants, self.rotations, self.calcs, self.parts = 0, [], [], []

    def const(self):
        self.n_constants += 1
        return (A.CONSTANT, self.n_constants - 1, 0)

    def q(self, kind, column, rot=0):
        if rot not in self.rotations:
            self.rotations.append(rot)
        return (kind, column, self.rotations.index(rot))

    def op(self, op, a, b=NO_B):
        self.calcs.append((op, tuple(a), tuple(b), 0, 0))
        return (A.INTERMEDIATE, len(self.calcs) - 1, 0)

    def horner(self, start, parts, factor):
        self.calcs.append((A.HORNER, tuple(start), tuple(factor), len(self.parts), len(parts)))
        self.parts += [tuple(p) for p in parts]
        return (A.INTERMEDIATE, len(self.calcs) - 1, 0)

    def sum_of(self, terms):
        acc = terms[0]
        for t in terms[1:]:
            acc = self.op(A.ADD, acc, t)
        return acc

    def raw(self):
        return RawGraph(self.n_constants, self.rotations or [0], self.calcs, self.parts)


def _loads_and_constants(b, n_loads, n_consts, column=0):
    """n_loads cells of advice columns from `column` on (bound 32 each) plus n_consts constants (bound 2 each), summed"""
    return b.sum_of([b.q(A.ADVICE, column + i, i % 2) for i in range(n_loads)] + [b.const() for _ in range(n_consts)])


def fill_mul_160():
    """two loads plus eight constants: an addition result at 80; times a constant: a product at 80 x 2 = 160"""
    b = _Build()
    b.op(A.MUL, _loads_and_constants(b, 2, 8), b.const())
    return b.raw()


def fill_muladd_160_plus_78():
    """x y + z in one G_MULADD with x y at 80 x 2 and z at 78 (two loads, seven constants: the compiler lets an addend run to
    80 - 2, so that the fused sum stays within 80)"""
    b = _Build()
    z = _loads_and_constants(b, 2, 7, column=2)
    b.op(A.ADD, b.op(A.MUL, _loads_and_constants(b, 2, 8), b.const()), z)
    return b.raw()


def fill_sqr_144():
    """the square of a sum of six constants: 12 x 12 = 144"""
    b = _Build()
    b.op(A.SQUARE, b.sum_of([b.const() for _ in range(6)]))
    return b.raw()


SUBTRAHENDS = {0: (0, 1), 1: (0, 2), 2: (0, 4), 3: (0, 8), 4: (1, 0), 5: (2, 0)}   # kidx -> (loads, constants): bound 2 << kidx


def fill_sub_neg(kidx, small_minuend=False):
    """a - b and -b with b at the whole of K = 2 << kidx (above half of it: no smaller K would do), then (a - b) c + (-b).
    a is a load (bound 32), at kidx 5 a load and twelve constants (56: the subtraction's result at 56 + 64 = 120); with
    small_minuend a constant, so that a - b + K p has nothing to spare when every word is the largest"""
    b = _Build()
    sub = _loads_and_constants(b, *SUBTRAHENDS[kidx], column=1)
    a =b.const() if small_minuend else _loads_and_constants(b, 1, 12 if kidx == 5 else 0)
    t, n = b.op(A.SUB, a, sub), b.op(A.NEGATE, sub)
    b.op(A.ADD, b.op(A.MUL, t, b.const()), n)
    return b.raw()


def fill_doubling():
    """doublings of a constant to 64 and on (the seventh reduces first), of a load to 64 and on, and of 40 (a load and four
    constants) to 80, which a constant then multiplies: 160"""
    b = _Build()
    x = b.const()
    for _ in range(8):
        x = b.op(A.DOUBLE, x)
    y = b.q(A.ADVICE, 0, 0)
    for _ in range(3):
        y = b.op(A.DOUBLE, y)
    z = b.op(A.MUL, b.op(A.DOUBLE, _loads_and_constants(b, 1, 4, column=1)), b.const())
    b.op(A.ADD, b.op(A.ADD, x, y), z)
    return b.raw()


def fill_product_at_the_top():
    """a product the compiler reduces one operand of: a = two loads and eight constants (80), b = P + P for a square P of a sum
    of constants (4), so G_RED(a) first; then -(a b) with K = 2.  (Canonical words do not bring a b to the top of 320 with the
    reduction left out: a constant's 2^261 form is what a product leaves, about p for the word r - 1, half its bound of 2.)"""
    b = _Build()
    p = b.op(A.SQUARE, b.sum_of([b.const() for _ in range(5)]))
    a = _loads_and_constants(b, 2, 8)
    b.op(A.NEGATE, b.op(A.MUL, a, b.op(A.ADD, p, p)))
    return b.raw()


ROTATION_KS = (1, 2, 5, 6)


def rotation_list(k):
    n = 1 << k
    out = []
    for r in (0, 1, -1, n - 1, -(n - 1), n, -n, n + 1, -(n + 1), -5, 17):
        if r not in out:
            out.append(r)
    return out


def rotations_graph(k):
    """a fixed, an advice and an instance column at rotations 0, +-1, +-(n - 1), +-n, +-(n + 1), -5 and 17 of n = 2^k (they wrap
    more than once at k = 1 and 2), folded by Horner in y so that no two queries may change places"""
    b = _Build()
    parts = [b.q(kind, 0, r) for r in rotation_list(k) for kind in (A.FIXED, A.ADVICE, A.INSTANCE)]
    b.horner(b.const(), parts, (A.Y, 0, 0))
    return b.raw()


MANY_CONSTANTS = 1500


def many_constants_graph():
    """40 live values (many_live_values(39)), then a Horner over 1500 constants of the table: 1504 entries with beta, gamma,
    theta and y.  At 64 rows per workgroup that is within one slot of the LDS budget"""
    g = RawGraph.of(many_live_values(39))
    last = (A.INTERMEDIATE, len(g.calcs) - 1, 0)
    g.parts = [(A.CONSTANT, i, 0) for i in range(MANY_CONSTANTS)]
    g.calcs.append((A.HORNER, last, (A.THETA, 0, 0), 0, MANY_CONSTANTS))
    g.n_constants = MANY_CONSTANTS
    return g


LARGE_PRODUCTS = 7000


def large_program_graph():
    """a balanced sum of 7000 products of two cells: more than 16384 lowered instructions (a blob above 256 KiB), 14 levels deep"""
    b = _Build()
    rots = (0, 1, -1, 2)
    level = [b.op(A.MUL, b.q(A.ADVICE, i % 4, rots[(i // 4) % 4]), b.q(A.FIXED, i % 3, rots[(i // 12) % 4])) for i in range(LARGE_PRODUCTS)]
    while len(level) > 1:
        level = [b.op(A.ADD, level[i], level[i + 1]) if i + 1 < len(level) else level[i] for i in range(0, len(level), 2)]
    return b.raw()


def random_folded_graph(rng, n_fixed, n_advice, n_instance, n_chal, n_calc, O):
    """random_graph ended the way halo2 ends a program, Horner(previous value, [every calculation], y): the last calculation
    of a random_graph reaches only a handful of the others (the lowering is demand-driven), this one reaches them all"""
    g = random_graph(rng, n_fixed, n_advice, n_instance, n_chal, n_calc, O)
    g.add_calculation(A.HORNER, (A.PREVIOUS_VALUE, 0, 0), (A.Y, 0, 0), [(A.INTERMEDIATE, q, 0) for q in range(len(g.calculations))])
    return g


FOLDED_SEEDS = [(501, 8, (3, 4, 1, 2)), (502, 40, (3, 4, 1, 2)), (503, 40, (1, 2, 0, 0)), (504, 120, (3, 4, 1, 2)), (505, 120, (2, 5, 1, 3)),
                (506, 300, (3, 4, 1, 2)), (507, 300, (4, 3, 0, 1))]
BOUND_FILLERS = ["fill_mul_160", "fill_muladd_160_plus_78", "fill_sqr_144", "fill_doubling", "fill_product_at_the_top",
                 *[f"fill_sub_neg_kidx{k}" for k in range(6)], *[f"fill_sub_neg_small_minuend_kidx{k}" for k in range(6)]]
REFUSED = ("live_values_70", "live_values_63")     # they lower; sg_quotient_gates* refuses them (65 slots and more; 64 slots)
_device_corpus = None


def device_corpus(O):
    """every graph of corpus(O) that lowers (the error_* graphs are the ones that do not), then the hand-written ones"""
    global _device_corpus
    if _device_corpus is not None:
        return _device_corpus
    cases = [c for c in corpus(O) if not c.name.startswith("error_")]
    own = lambda name, graph, na, nf=0, ni=0: cases.append(Case(name, graph, nf, na, ni, 0))
    for seed, n_calc, dims in FOLDED_SEEDS:
        cases.append(Case(f"random_folded_seed{seed}_calc{n_calc}", random_folded_graph(np.random.default_rng(seed), *dims, n_calc, O), *dims))
    own("fill_mul_160", fill_mul_160(), 2)
    own("fill_muladd_160_plus_78", fill_muladd_160_plus_78(), 4)
    own("fill_sqr_144", fill_sqr_144(), 1)
    own("fill_doubling", fill_doubling(), 2)
    own("fill_product_at_the_top", fill_product_at_the_top(), 2)
    for kidx in range(6):
        own(f"fill_sub_neg_kidx{kidx}", fill_sub_neg(kidx), 3)
        own(f"fill_sub_neg_small_minuend_kidx{kidx}", fill_sub_neg(kidx, small_minuend=True), 3)
    for k in ROTATION_KS:
        own(f"rotations_k{k}", rotations_graph(k), 1, 1, 1)
    own("many_constants", many_constants_graph(), 1)
    own("large_program", large_program_graph(), 4, 3)
    own("live_values_62", many_live_values(62), 1)
    own("live_values_63", many_live_values(63), 1)
    assert len({c.name for c in cases}) == len(cases) and set(BOUND_FILLERS) <= {c.name for c in cases}
    _device_corpus = cases
    return cases


def device_case(O, name):
    return next(c for c in device_corpus(O) if c.name == name)


# ----------------------------------------------------------------------------- words
# Every word fed is canonical (below r).  That is the compiler's contract (gates_compile.h at convert_at_load: "column words
# (canonical, < p) enter as x~ << 5 = x^ with bound 32"), and the prover hands the evaluator nothing else: NTT outputs and columns
# it has counted canonical.  A word at or above r would break the bound 32 the lowering starts from, so none is fed here.
PATTERNS = ["top", "zero", "one", "columns_alternate", "columns_alternate_reversed", "rows_cycle", "random"]
ONE = (1 << 256) % R
CYCLE = [0, 1, R - 1, R - 2, 1 << 253, None]    # None: a random word


def _words(values):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), dtype=np.uint8).copy()


def _ints(words):
    raw = bytes(np.ascontiguousarray(words, dtype=np.uint8))
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


def _pattern_words(O, pattern, n, j, seed):
    """n words of the j-th array (a column, the previous values, the constants, the challenges, beta .. y)"""
    if pattern == "random" or n == 0:
        return O.random_fr(seed, n)
    if pattern == "rows_cycle":
        rnd = _ints(O.random_fr(seed, n))
        return _words([rnd[i] if CYCLE[i % 6] is None else CYCLE[i % 6] for i in range(n)])
    if pattern.startswith("columns_alternate"):
        pattern = "top" if (j % 2 == 0) != pattern.endswith("reversed") else "zero"
    return np.tile(_words([{"top": R - 1, "zero": 0, "one": ONE}[pattern]]), n)


def make_inputs(O, case, pattern, rows, seed=0):
    """{"fixed" / "advice" / "instance": [rows x 32 B], "previous": rows x 32 B, "constants", "challenges", "beta", "gamma",
    "theta", "y"}: the pattern applies to all of them alike.  beta .. y are the four words of one array (rows_cycle: 0, 1,
    r - 1, r - 2); under columns_alternate the arrays count on from the columns: previous, constants, challenges, beta .. y."""
    assert pattern in PATTERNS
    j, inp = 0, {}

    def take(n):
        nonlocal j
        j += 1
        return _pattern_words(O, pattern, n, j - 1, 7919 * seed + 31 * j + 1)
    for group, n in (("fixed", case.n_fixed), ("advice", case.n_advice), ("instance", case.n_instance)):
        inp[group] = [take(rows) for _ in range(n)]
    inp["previous"] = take(rows)
    inp["constants"] = take(case.graph.n_constants)
    inp["challenges"] = take(case.n_challenges)
    four = take(4)
    for i, name in enumerate(("beta", "gamma", "theta", "y")):
        inp[name] = four[32 * i:32 * i + 32].copy()
    return inp


class GraphWithConstants:
    """what circuits_halo2_amd.arithmetic.quotient_gates* takes for a graph: the case's structure with these constants"""

    def __init__(self, case, constants):
        self.case, self.constants = case, np.ascontiguousarray(constants, dtype=np.uint8)

    def _struct(self):
        return self.case.graph._struct(self.constants)


# ----------------------------------------------------------------------------- the expectation
def _reached(graph):
    calcs = graph.calcs
    seen, todo = set(), [len(calcs) - 1]
    while todo:
        q = todo.pop()
        if q in seen:
            continue
        seen.add(q)
        op, a, b, off, n = calcs[q]
        srcs = [a] + ([b] if op <= A.MUL or op == A.HORNER else []) + (graph.parts[off:off + n] if op == A.HORNER else [])
        todo += [s[1] for s in srcs if s[0] == A.INTERMEDIATE]
    return seen


def _oracle_graph(case, constants):
    """the graph as oracle.quotient_gates reads it.  The C oracle evaluates every calculation in order, also those the result
    never looks at; the unreached_* graphs keep their faults there, so an unreached calculation becomes a copy of the previous
    value (the library never lowers it, halo2 never reads it)"""
    g = case.graph
    if not hasattr(case, "_oracle_calcs"):
        seen = _reached(g)
        case._oracle_calcs = [(op, a, b, g.parts[off:off + n]) if q in seen else (A.STORE, (A.PREVIOUS_VALUE, 0, 0), NO_B, [])
                              for q, (op, a, b, off, n) in enumerate(g.calcs)]
    return {"constants": np.ascontiguousarray(constants, dtype=np.uint8), "rotations": g.rotations, "calculations": case._oracle_calcs}


def _blocks(k, ext_k, cosets):
    """(rows per block, number of blocks, rows a unit rotation moves by)"""
    return (1 << k, cosets, 1) if cosets else (1 << ext_k, 1, 1 << (ext_k - k))


def expected_rows(O, case, inp, k, ext_k, cosets=0):
    """the rows sg_quotient_gates_dev (cosets = 0: one block of 2^ext_k rows) or sg_quotient_gates_cosets_dev (cosets blocks of 2^k
    rows, each a domain of its own) must give, by the C oracle"""
    n, blocks, _ = _blocks(k, ext_k, cosets)
    g = _oracle_graph(case, inp["constants"])
    out = []
    for b in range(blocks):
        blk = lambda a: a[32 * n * b:32 * n * (b + 1)]
        out.append(O.quotient_gates(blk(inp["previous"]), g, *[[blk(c) for c in inp[grp]] for grp in ("fixed", "advice", "instance")],
                                    inp["challenges"], inp["beta"], inp["gamma"], inp["theta"], inp["y"], *((k, k) if cosets else (k, ext_k))))
    return np.concatenate(out)


MONT_INV = pow(1 << 256, -1, R)


def definition_rows(case, inp, k, ext_k, cosets=0, rows=None, rotation_wraps_at_k=False):
    """the same rows from halo2's definition in Python integers (oracle.pyref.eval_graph, row by row) under the Montgomery reading:
    a word w stands for w 2^-256 mod r, the result v is the word v 2^256 mod r, and rotation rho reads row
    (i + rho 2^(ext_k - k)) mod 2^ext_k of the block (coset-major: ext_k = k inside every block).  rows: only these.
    rotation_wraps_at_k: the wrong reading (i + rho) mod 2^k within the row's 2^k, for showing that the cases tell the two apart"""
    from oracle import pyref
    n, blocks, step = _blocks(k, ext_k, cosets)
    val = lambda words: [w * MONT_INV % R for w in _ints(words)]
    cols = {A.FIXED: [val(c) for c in inp["fixed"]], A.ADVICE: [val(c) for c in inp["advice"]], A.INSTANCE: [val(c) for c in inp["instance"]]}
    prev, consts, chal = val(inp["previous"]), val(inp["constants"]), val(inp["challenges"])
    beta, gamma, theta, y = (val(inp[name])[0] for name in ("beta", "gamma", "theta", "y"))
    graph = case.graph.as_dict(consts)
    out = []
    for i in (range(n * blocks) if rows is None else rows):
        base, at = i - i % n, i % n
        if rotation_wraps_at_k:
            cell = lambda kind, index, rot: cols[kind][index][base + (at - at % (1 << k)) + (at + rot) % (1 << k)]
        else:
            cell = lambda kind, index, rot: cols[kind][index][base + (at + rot * step) % n]
        out.append(pyref.eval_graph(graph, cell, chal, beta, gamma, theta, y, prev[i]) * (1 << 256) % R)
    return _words(out)


# ----------------------------------------------------------------------------- the device's arithmetic, in integers
# What gates_kernel does to a row, value for value, where run_program above only keeps residues: a value is the integer its nine
# limbs hold (csrc/bn254_f29.cuh).  A load is the word shifted left by 5 bits; a constant, and a load with kidx 1, is the
# Montgomery product with 2^266; a product is (a b + m p) / 2^261 with m = -a b / p mod 2^261, below (Ba Bb / 170.7 + 1) p; a
# subtraction adds K p = (2 << kidx) p first and must not go below zero (the top limb is 32 bits wide: a negative value is out by
# 2^264); a reduction takes off q p with q estimated from the top limb.  The row's word is the product with 2^256, less p if
# it is not below p.  Beside the value every tracked bound is re-derived as in run_program.
R261 = 1 << 261
_NEG_P_INV = -pow(R, -1, R261) % R261
_RECIP = (1 << 40) // ((R >> 232) + 1)


def mont261(a, b):
    t = a * b
    return (t + t * _NEG_P_INV % R261 * R) >> 261


class DeviceModelFault(AssertionError):
    pass


def run_device_model(words, const_words, column_word, previous_word, skip_reduction=None, kidx_delta=0, check=True, products=None):
    """the word the interpreter stores for one row.  const_words: the table's words; column_word(index, rotation) -> word.
    check: every value stays below its tracked bound times p, no subtraction goes below zero and the stored word is canonical
    (DeviceModelFault otherwise).  Two ways to break the program, for showing that the cases notice: skip_reduction = n turns
    the n-th G_RED into a copy that keeps its operand's bound (the compiler letting a product through at a bound above 170;
    products, a list, receives every product's Ba Bb); kidx_delta = -1 subtracts with half the K the compiler chose."""
    n_slots, result_kind, result_index, ops = decode(words)
    r266, r256 = (1 << 266) % R, (1 << 256) % R
    consts = [mont261(w, r266) for w in const_words]
    slot = [None] * n_slots

    def get(kind, idx):
        return (consts[idx], 2) if kind == CONST else slot[idx]

    def minus(x, y, kidx):
        v = x + (2 << max(0, kidx + kidx_delta)) * R - y
        if v < 0:
            if check:
                raise DeviceModelFault(("a subtraction below zero", pc, kidx))
            v += 1 << 264
        return v

    n_red = 0
    for pc, o in enumerate(ops):
        code, kidx = o["code"], o["kidx"]
        if code == LOADCOL:
            w = column_word(o["a"], o["b"])
            r = (mont261(w, r266), 2) if kidx else (w << 5, 32)
        elif code == LOADPREV:
            r = previous_word << 5, 32
        else:
            (x, bx), (y, by) = get(o["ak"], o["a"]), get(o["bk"], o["b"])
            if code == G_ADD:
                r = x + y, bx + by
            elif code == G_SUB:
                r = minus(x, y, kidx), bx + (2 << kidx)
            elif code == G_MUL:
                r = mont261(x, y), 2
            elif code == G_SQR:
                r = mont261(x, x), 2
            elif code == G_DBL:
                r = 2 * x, 2 * bx
            elif code == G_NEG:
                r = minus(0, x, kidx), 2 << kidx
            elif code == G_RED:
                r = (x, bx) if n_red == skip_reduction else (x - (((x >> 232) * _RECIP) >> 40) * R, 2)
                n_red += 1
            else:
                z, bz = get(kidx, o["c"])
                r = mont261(x, y) + z, 2 + bz
            if products is not None and code in (G_MUL, G_SQR, G_MULADD):
                products.append(bx * (bx if code == G_SQR else by))
        if check and not 0 <= r[0] <= r[1] * R:
            raise DeviceModelFault(("a value at or above its bound", pc, OPCODES[code], r[1], r[0] / R))
        slot[o["dst"]] = r
    v = mont261(get(result_kind, result_index)[0], r256)
    v = v - R if v >= R else v
    if check and not 0 <= v < R:
        raise DeviceModelFault(("the stored word is not canonical", v / R))
    return v % (1 << 256)
