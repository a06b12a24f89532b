// Host side of the custom-gate block (see gates.hip for the device side), free of HIP: tests/cpp/gates_compile_check.cpp runs it
// on the CPU.  A halo2 GraphEvaluator graph is lowered to a straight-line program over LDS slots --
//   * every value lives in the 2^261 (hat) limb form; column words are shifted left by 5 bits on load
//     (which is that form, with bound 32, at no cost), constants are converted once per workgroup;
//   * additions / subtractions are lazy (bound tracking as in the curve code); a reduction (f29_reduce_small: the
//     quotient from the top limb, ~45 instructions, no product) is inserted only where the next product would exceed
//     bound_a * bound_b <= 170;
//   * a product that only an addition reads is fused into it (G_MULADD = f29_mul_add: the addend joins the high columns
//     of the product, one instruction stream entry and one LDS round trip less); Horner is a chain of those;
//   * Store is an alias, loads are emitted at first use;
//   * slots are allocated by liveness (last use), so the LDS footprint is the maximum number of
//     simultaneously live values, not the number of intermediates.
// The lowered program depends on the graph's structure alone: the values (constants, challenges, beta, gamma, theta, y) are a
// table beside it (gate_const_table), refreshed per call.  Also here: the interpreter's rows per workgroup
// (gates_interpreter_tile) and the cache of lowered programs (GateProgramCache).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/summa_gpu.h"

namespace sg {

struct GateOp {  // one instruction of the compiled program (4 words, read with scalar loads)
  uint32_t w0;   // opcode | kidx << 8 | a_kind << 16 | b_kind << 24   (MULADD: the kidx byte holds the kind of c)
  uint32_t dst;  // LDS slot (low 16 bits); MULADD: the third operand c in the high 16 bits
  uint32_t a, b; // slot / constant index / (LOADCOL: column index, rotation)
};
// G_RED: the same residue below 2p (f29_reduce_small); G_MULADD: a * b + c under one reduction (f29_mul_add)
enum GateOpcode : uint32_t { G_LOADCOL, G_LOADPREV, G_ADD, G_SUB, G_MUL, G_SQR, G_DBL, G_NEG, G_RED, G_MULADD };
enum GateOperandKind : uint32_t { GK_SLOT = 0, GK_CONST = 1 };

struct GateProgram {
  std::vector<GateOp> ops;
  std::vector<uint32_t> const_words;  // 8 words per constant (memory-domain Fr): gate_const_table, per call
  uint32_t n_slots = 0, result_kind = GK_SLOT, result_index = 0;
  uint32_t n_columns = 0;             // fixed ++ advice ++ instance
  std::vector<uint8_t> signature;     // structure bytes this program was lowered from (cache confirmation)
};

// The knobs of the lowering.  The library fills them from the environment in one place (gates_env, gates.hip).
struct GateLowering {
  // (column, rotation): a loaded value is reused only while its previous use is at most this many instructions back; beyond
  // that a fresh load (a 32-byte read, L2-resident: the row's cache lines were touched a moment ago) is cheaper than pinning
  // an LDS slot -- the slot count sets the kernel's occupancy
  size_t reload_distance = 12;
  // development aid: a column the graph refers to more than convert_above times is converted at the load (one product, bound 2).
  // Off by default: column words (canonical, < p) enter as x~ << 5 = x^ with bound 32 for free; the bound tracker inserts a
  // reduction only where a consumer needs one (a product with a bound-2 value does not), and once a value has been reduced
  // its later uses see the reduced copy, so nothing is gained by converting at the load
  bool convert_at_load = false;
  uint32_t convert_above = 0;
};

// constants ++ challenges ++ beta, gamma, theta, y: the table the lowered program's GK_CONST operands index, 8 words each
inline void gate_const_table(const sg_graph& g, const uint8_t* challenges, uint32_t n_challenges, const uint8_t beta[32],
                             const uint8_t gamma[32], const uint8_t theta[32], const uint8_t y[32], std::vector<uint32_t>* words) {
  words->resize(8 * ((size_t)g.n_constants + n_challenges + 4));
  uint8_t* at = reinterpret_cast<uint8_t*>(words->data());
  auto push = [&](const uint8_t* p, size_t n) {
    if (n) std::memcpy(at, p, 32 * n);
    at += 32 * n;
  };
  push(g.constants, g.n_constants);
  push(challenges, n_challenges);
  push(beta, 1); push(gamma, 1); push(theta, 1); push(y, 1);
}

// every value source a calculation reads: a, then b where the operation has one, then a Horner's parts (those of a Horner
// whose range lies outside horner_parts are not walked: gates_validate refuses such a graph)
template <class F>
void for_each_operand(const sg_calculation& cal, const sg_graph& g, F&& f) {
  f(cal.a);
  if (cal.op <= SG_OP_MUL || cal.op == SG_OP_HORNER) f(cal.b);
  if (cal.op == SG_OP_HORNER && (uint64_t)cal.parts_offset + cal.parts_len <= g.n_horner_parts)
    for (uint32_t t = 0; t < cal.parts_len; t++) f(g.horner_parts[cal.parts_offset + t]);
}

namespace gates_detail {
constexpr uint32_t MAX_CALCULATIONS = 1u << 16, MAX_DEPTH = 4096;
constexpr uint32_t LOAD_BOUND = 32;

struct Val {         // a virtual value of the lowered program
  uint32_t kind;     // GK_SLOT (virtual id in `index`) or GK_CONST
  uint32_t index;
};
struct IrOp {
  uint32_t code, kidx;
  uint32_t dst;      // virtual id
  Val a, b;
  uint32_t col = 0;
  int32_t rot = 0;
  Val c{GK_CONST, 0};   // MULADD: the addend
};
inline bool is_load(const IrOp& op) { return op.code == G_LOADCOL || op.code == G_LOADPREV; }
template <class F>
void for_each_slot_read(const IrOp& op, F&& f) {   // the virtual values an instruction reads, repeats included
  if (is_load(op)) return;
  if (op.a.kind == GK_SLOT) f(op.a.index);
  if (op.b.kind == GK_SLOT) f(op.b.index);
  if (op.code == G_MULADD && op.c.kind == GK_SLOT) f(op.c.index);
}

// the instructions so far, with the bound of every value: each operation reduces its operands only as far as it must
struct BoundTracker {
  std::vector<IrOp> ir;
  std::vector<uint32_t> bound;     // per virtual id
  std::vector<uint32_t> redirect;  // virtual id -> reduced replacement (or itself)
  uint32_t new_value(uint32_t b) {
    bound.push_back(b);
    redirect.push_back((uint32_t)redirect.size());
    return (uint32_t)bound.size() - 1;
  }
  Val resolve(Val v) {
    if (v.kind == GK_SLOT)
      while (redirect[v.index] != v.index) v.index = redirect[v.index];
    return v;
  }
  uint32_t bnd(const Val& v) const { return v.kind == GK_CONST ? 2u : bound[v.index]; }
  Val reduce(Val v) {  // f29_reduce_small: bound 2
    v = resolve(v);
    if (v.kind == GK_CONST || bound[v.index] <= 2) return v;
    uint32_t d = new_value(2);
    ir.push_back({G_RED, 0, d, v, v});
    redirect[v.index] = d;  // later uses see the reduced copy
    return Val{GK_SLOT, d};
  }
  void reduce_for_product(Val& a, Val& b) {
    while (bnd(a) * bnd(b) > 170) {
      if (bnd(a) >= bnd(b)) a = reduce(a); else b = reduce(b);
    }
  }
  Val emit2(uint32_t code, uint32_t kidx, Val a, Val b, uint32_t out_bound) {
    uint32_t d = new_value(out_bound);
    ir.push_back({code, kidx, d, a, b});
    return Val{GK_SLOT, d};
  }
  Val load(uint32_t code, uint32_t kidx, uint32_t col, int32_t rot, uint32_t out_bound) {
    uint32_t d = new_value(out_bound);
    IrOp op{code, kidx, d, Val{GK_CONST, 0}, Val{GK_CONST, 0}};
    op.col = col; op.rot = rot;
    ir.push_back(op);
    return Val{GK_SLOT, d};
  }
  Val add(Val a, Val b) {
    a = resolve(a); b = resolve(b);
    while (bnd(a) + bnd(b) > 80) {
      if (bnd(a) >= bnd(b)) a = reduce(a); else b = reduce(b);
    }
    return emit2(G_ADD, 0, a, b, bnd(a) + bnd(b));
  }
  static uint32_t kidx_for(uint32_t b) {  // smallest K = 2 << kidx >= b
    uint32_t k = 0;
    while ((2u << k) < b) k++;
    return k;
  }
  Val sub(Val a, Val b) {
    a = resolve(a); b = resolve(b);
    if (bnd(b) > 64) b = reduce(b);
    uint32_t k = kidx_for(bnd(b));
    if (bnd(a) + (2u << k) > 120) a = reduce(a);
    return emit2(G_SUB, k, a, b, bnd(a) + (2u << k));
  }
  Val neg(Val a) {
    a = resolve(a);
    if (bnd(a) > 64) a = reduce(a);
    uint32_t k = kidx_for(bnd(a));
    return emit2(G_NEG, k, a, a, 2u << k);
  }
  Val dbl(Val a) {
    a = resolve(a);
    if (bnd(a) > 40) a = reduce(a);
    return emit2(G_DBL, 0, a, a, 2 * bnd(a));
  }
  Val mul(Val a, Val b) {
    a = resolve(a); b = resolve(b);
    reduce_for_product(a, b);
    return emit2(G_MUL, 0, a, b, 2);
  }
  Val sqr(Val a) {
    a = resolve(a);
    if (bnd(a) * bnd(a) > 170) a = reduce(a);
    return emit2(G_SQR, 0, a, a, 2);
  }
  Val muladd(Val a, Val b, Val z) {   // a b + z under one reduction: bound 2 + bound(z)
    a = resolve(a); b = resolve(b); z = resolve(z);
    reduce_for_product(a, b);
    if (bnd(z) + 2 > 80) z = reduce(z);
    uint32_t d = new_value(bnd(z) + 2);
    IrOp op{G_MULADD, 0, d, a, b};
    op.c = z;
    ir.push_back(op);
    return Val{GK_SLOT, d};
  }
};

// Step 1.  What is refused wherever it stands in the graph: a reference to a calculation that is not earlier (the emission
// recurses along references and trusts them), a Horner whose parts lie outside horner_parts, a dependency chain deeper than
// the recursion may go (halo2 graphs are a few hundred deep).  Every other fault is met by the emission, and only in a
// calculation the result depends on.
inline const char* gates_validate(const sg_graph& g) {
  if (g.n_calculations == 0) return "empty program";
  if ((g.n_constants && !g.constants) || (g.n_rotations && !g.rotations) || !g.calculations || (g.n_horner_parts && !g.horner_parts))
    return "null array in graph";
  if (g.n_calculations > MAX_CALCULATIONS) return "more than 65536 calculations";
  for (uint32_t q = 0; q < g.n_calculations; q++) {
    const sg_calculation& cal = g.calculations[q];
    bool forward = false;
    for_each_operand(cal, g, [&](const sg_value_source& s) { forward = forward || (s.kind == SG_VS_INTERMEDIATE && s.index >= q); });
    if (forward) return "intermediate used before it is defined";
    if (cal.op == SG_OP_HORNER && (uint64_t)cal.parts_offset + cal.parts_len > g.n_horner_parts) return "horner parts out of range";
  }
  std::vector<uint32_t> depth(g.n_calculations, 1);
  for (uint32_t q = 0; q < g.n_calculations; q++) {
    uint32_t d = 0;
    for_each_operand(g.calculations[q], g, [&](const sg_value_source& s) { if (s.kind == SG_VS_INTERMEDIATE) d = std::max(d, depth[s.index]); });
    depth[q] = d + 1;
    if (depth[q] > MAX_DEPTH) return "dependency chain deeper than 4096 calculations";
  }
  return nullptr;
}

// Step 2.  How often each intermediate is read (the result counts as a reader), and each (column, rotation) of the graph
struct GateUses {
  std::vector<uint32_t> of_intermediate;
  std::map<std::pair<uint32_t, int32_t>, uint32_t> of_column;
};
inline uint32_t gates_column_base(uint32_t kind, uint32_t n_fixed, uint32_t n_advice) {   // columns run fixed ++ advice ++ instance
  return kind == SG_VS_FIXED ? 0 : kind == SG_VS_ADVICE ? n_fixed : n_fixed + n_advice;
}
inline GateUses gates_count_uses(const sg_graph& g, uint32_t n_fixed, uint32_t n_advice) {
  GateUses uses;
  uses.of_intermediate.assign(g.n_calculations, 0);
  for (uint32_t q = 0; q < g.n_calculations; q++)
    for_each_operand(g.calculations[q], g, [&](const sg_value_source& s) {
      if (s.kind == SG_VS_INTERMEDIATE) uses.of_intermediate[s.index]++;
      if (s.kind >= SG_VS_FIXED && s.kind <= SG_VS_INSTANCE && s.rotation < g.n_rotations)
        uses.of_column[std::make_pair(gates_column_base(s.kind, n_fixed, n_advice) + s.index, g.rotations[s.rotation])]++;
    });
  uses.of_intermediate[g.n_calculations - 1]++;
  return uses;
}

// Step 3.  Demand-driven emission: an intermediate is lowered when it is first needed, starting from the last
// calculation.  halo2 ends a program with Horner(PreviousValue, [all gate polynomials], Y); emitted in
// program order every gate value would stay live until that final fold, emitted on demand each one
// is folded right after it is computed (and unused calculations disappear).
struct Emitter {
  const sg_graph& g;
  const uint32_t n_fixed, n_advice, n_instance, n_challenges;
  const GateLowering& how;
  GateUses uses;
  BoundTracker c;
  std::map<std::pair<uint32_t, int32_t>, std::pair<Val, size_t>> loaded;   // (column, rotation) -> (value, index of its latest use)
  Val prev{GK_SLOT, 0xffffffffu};
  std::vector<Val> inter;
  std::vector<uint8_t> done;
  const char* err = nullptr;   // of the fault met last: the emission goes on with a placeholder

  Emitter(const sg_graph& graph, uint32_t nf, uint32_t na, uint32_t ni, uint32_t nc, const GateLowering& lowering)
      : g(graph), n_fixed(nf), n_advice(na), n_instance(ni), n_challenges(nc), how(lowering), uses(gates_count_uses(graph, nf, na)),
        inter(graph.n_calculations, Val{GK_CONST, 0}), done(graph.n_calculations, 0) {}
  Val fail(const char* what) {
    err = what;
    return Val{GK_CONST, 0};
  }
  Val column(const sg_value_source& s) {
    const uint32_t lim = s.kind == SG_VS_FIXED ? n_fixed : s.kind == SG_VS_ADVICE ? n_advice : n_instance;
    if (s.index >= lim || s.rotation >= g.n_rotations) return fail("column query out of range");
    const auto key = std::make_pair(gates_column_base(s.kind, n_fixed, n_advice) + s.index, g.rotations[s.rotation]);
    auto it = loaded.find(key);
    if (it != loaded.end() && c.ir.size() - it->second.second <= how.reload_distance) {
      it->second.second = c.ir.size();
      return it->second.first;
    }
    const bool convert = how.convert_at_load && uses.of_column[key] > how.convert_above;
    const Val v = c.load(G_LOADCOL, convert ? 1u : 0u, key.first, key.second, convert ? 2 : LOAD_BOUND);
    loaded[key] = std::make_pair(v, c.ir.size());
    return v;
  }
  Val source(const sg_value_source& s) {
    const uint32_t c_chal = g.n_constants, c_beta = c_chal + n_challenges;   // gate_const_table's order
    switch (s.kind) {
      case SG_VS_CONSTANT: return s.index < g.n_constants ? Val{GK_CONST, s.index} : fail("constant index out of range");
      case SG_VS_INTERMEDIATE: return inter[s.index];
      case SG_VS_FIXED: case SG_VS_ADVICE: case SG_VS_INSTANCE: return column(s);
      case SG_VS_CHALLENGE: return s.index < n_challenges ? Val{GK_CONST, c_chal + s.index} : fail("challenge index out of range");
      case SG_VS_BETA: return Val{GK_CONST, c_beta};
      case SG_VS_GAMMA: return Val{GK_CONST, c_beta + 1};
      case SG_VS_THETA: return Val{GK_CONST, c_beta + 2};
      case SG_VS_Y: return Val{GK_CONST, c_beta + 3};
      case SG_VS_PREVIOUS_VALUE:
        if (prev.index == 0xffffffffu) prev = c.load(G_LOADPREV, 0, 0, 0, LOAD_BOUND);
        return prev;
      default: return fail("unknown value source");
    }
  }
  Val need(const sg_value_source& s) {
    if (s.kind == SG_VS_INTERMEDIATE) lower(s.index);
    return source(s);
  }
  void lower(uint32_t q) {
    if (done[q] || err) return;   // (after a fault an intermediate stays the placeholder it was created as)
    done[q] = 1;
    const sg_calculation& cal = g.calculations[q];
    if (cal.op == SG_OP_ADD) {
      // x * y + z: one operand a product (or a square) that nothing else reads and that has not been lowered yet
      auto fusable = [&](const sg_value_source& s) {
        return s.kind == SG_VS_INTERMEDIATE && uses.of_intermediate[s.index] == 1 && !done[s.index] &&
               (g.calculations[s.index].op == SG_OP_MUL || g.calculations[s.index].op == SG_OP_SQUARE);
      };
      const bool fa = fusable(cal.a), fb = !fa && fusable(cal.b);
      if (fa || fb) {
        const sg_value_source& prod = fa ? cal.a : cal.b;
        const sg_calculation& m = g.calculations[prod.index];
        done[prod.index] = 1;
        const Val z = need(fa ? cal.b : cal.a);          // the addend first: one live value while the factors are computed
        const Val x = need(m.a);
        const Val y = m.op == SG_OP_SQUARE ? x : need(m.b);
        inter[q] = c.muladd(x, y, z);
        return;
      }
    }
    Val a = need(cal.a);
    switch (cal.op) {
      case SG_OP_ADD: inter[q] = c.add(a, need(cal.b)); break;
      case SG_OP_SUB: inter[q] = c.sub(a, need(cal.b)); break;
      case SG_OP_MUL: inter[q] = c.mul(a, need(cal.b)); break;
      case SG_OP_SQUARE: inter[q] = c.sqr(a); break;
      case SG_OP_DOUBLE: inter[q] = c.dbl(a); break;
      case SG_OP_NEGATE: inter[q] = c.neg(a); break;
      case SG_OP_HORNER: {
        Val f = need(cal.b), acc = a;
        for (uint32_t t = 0; t < cal.parts_len && !err; t++) acc = c.muladd(acc, f, need(g.horner_parts[cal.parts_offset + t]));
        inter[q] = acc;
        break;
      }
      case SG_OP_STORE: inter[q] = a; break;
      default: fail("unknown calculation");
    }
  }
};

// Step 4.  Slots by liveness: a value holds its slot from the instruction that writes it to the last one that reads it (the
// result: to the end); operands dying at an instruction free their slots before its destination is chosen (in-place update)
struct SlotPlan {
  std::vector<uint32_t> slot;   // per virtual value
  uint32_t n_slots = 0;
};
inline SlotPlan gates_allocate_slots(const std::vector<IrOp>& ir, uint32_t n_values, Val result) {
  const uint32_t END = 0xffffffffu;
  std::vector<uint32_t> last(n_values, 0);   // the last instruction that reads each value
  for (uint32_t i = 0; i < ir.size(); i++) for_each_slot_read(ir[i], [&](uint32_t v) { last[v] = i; });
  if (result.kind == GK_SLOT) last[result.index] = END;
  SlotPlan plan;
  plan.slot.assign(n_values, END);
  std::vector<uint32_t> free_slots;
  for (uint32_t i = 0; i < ir.size(); i++) {
    const IrOp& op = ir[i];
    uint32_t seen[3] = {0, 0, 0}, n_seen = 0;
    for_each_slot_read(op, [&](uint32_t v) {
      if (last[v] == i && std::find(seen, seen + n_seen, v) == seen + n_seen) free_slots.push_back(plan.slot[v]);
      seen[n_seen++] = v;
    });
    if (free_slots.empty()) free_slots.push_back(plan.n_slots++);
    plan.slot[op.dst] = free_slots.back();
    // a value that is never read still needs somewhere to land: its slot stays free, immediately reusable
    const bool never_read = last[op.dst] == 0 && !(result.kind == GK_SLOT && result.index == op.dst);
    if (!never_read) free_slots.pop_back();
  }
  return plan;
}

// Step 5.  The instruction words (GateOp)
inline const char* gates_encode(const std::vector<IrOp>& ir, const SlotPlan& plan, std::vector<GateOp>* ops) {
  auto index = [&](const Val& v) { return v.kind == GK_SLOT ? plan.slot[v.index] : v.index; };
  for (const IrOp& op : ir) {
    const bool three = op.code == G_MULADD;
    const uint32_t d = plan.slot[op.dst], c_idx = three ? index(op.c) : 0;
    if (d > 0xffff || c_idx > 0xffff) return "program too large (slot or constant index above 65535)";
    GateOp o{};
    o.w0 = op.code | ((three ? op.c.kind : op.kidx) << 8) | (op.a.kind << 16) | (op.b.kind << 24);
    o.dst = d | (c_idx << 16);
    o.a = is_load(op) ? op.col : index(op.a);
    o.b = is_load(op) ? (uint32_t)op.rot : index(op.b);
    ops->push_back(o);
  }
  return nullptr;
}
}  // namespace gates_detail

// halo2-shaped graph -> compiled program (its constant table left empty: gate_const_table).  Returns an empty string on
// success, a message otherwise.
inline std::string compile_gates(const sg_graph& g, uint32_t n_fixed, uint32_t n_advice, uint32_t n_instance, uint32_t n_challenges,
                                 const GateLowering& how, GateProgram* out) {
  using namespace gates_detail;
  if (const char* err = gates_validate(g)) return err;
  Emitter e(g, n_fixed, n_advice, n_instance, n_challenges, how);
  e.lower(g.n_calculations - 1);
  if (e.err) return e.err;
  const Val result = e.c.resolve(e.inter[g.n_calculations - 1]);
  const SlotPlan plan = gates_allocate_slots(e.c.ir, (uint32_t)e.c.bound.size(), result);
  GateProgram prog;
  if (const char* err = gates_encode(e.c.ir, plan, &prog.ops)) return err;
  prog.n_slots = std::max<uint32_t>(1, plan.n_slots);
  prog.result_kind = result.kind;
  prog.result_index = result.kind == GK_SLOT ? plan.slot[result.index] : result.index;
  prog.n_columns = n_fixed + n_advice + n_instance;
  *out = std::move(prog);
  return "";
}

// ------------------------------------------------------------------ the interpreter's rows per workgroup
// slots in LDS as [slot][limb][row], 9 limbs of 4 bytes, behind the converted constants: (constants + slots * rows) * 36 B
constexpr size_t GATES_LDS_BUDGET = 144 * 1024, GATES_LDS_PER_CU = 160 * 1024, GATES_VALUE_BYTES = 36;
// more simultaneously live values than this fit no shape (sg_quotient_gates* refuses the program by this name; with exactly
// this many nothing is left for the constants, and gates_run refuses it by `fits`)
constexpr uint32_t GATES_MAX_SLOTS = (uint32_t)(GATES_LDS_BUDGET / (64 * GATES_VALUE_BYTES));
struct GateTile {
  uint32_t rows;      // per workgroup: 256, 128 or 64
  size_t lds_bytes;   // dynamic LDS of a workgroup
  bool fits;          // within GATES_LDS_BUDGET
  uint32_t waves;     // per CU, by LDS (0: no shape fits)
};
// What limits the interpreter is waves per SIMD, i.e. LDS per row (the slot count).  Take the shape that keeps the most waves per
// CU; among shapes within one wave of each other the larger workgroup (measured: for programs of few slots 256 rows beat 64
// rows although the latter keeps one more wave).  forced_rows: a development aid (SG_GATES_ROWS), 0 or any other value: none.
inline GateTile gates_interpreter_tile(uint32_t n_slots, uint32_t n_consts, uint32_t forced_rows = 0) {
  const size_t cbytes = (size_t)n_consts * GATES_VALUE_BYTES;
  GateTile t{256, 0, false, 0};
  for (uint32_t rows : {256u, 128u, 64u}) {
    const size_t need = cbytes + (size_t)n_slots * rows * GATES_VALUE_BYTES;
    if (need > GATES_LDS_BUDGET) continue;
    const uint32_t waves = std::min<uint32_t>(32, (uint32_t)(GATES_LDS_PER_CU / need) * (rows / 64));
    if (waves > t.waves + 1 || t.waves == 0) {
      t.waves = waves;
      t.rows = rows;
    }
  }
  if (forced_rows == 64 || forced_rows == 128 || forced_rows == 256) t.rows = forced_rows;
  t.lds_bytes = cbytes + (size_t)n_slots * t.rows * GATES_VALUE_BYTES;
  t.fits = t.lds_bytes <= GATES_LDS_BUDGET;
  return t;
}

// ------------------------------------------------------------------ lowered programs by structure
// The lowered program depends on the graph's structure and the GateLowering only, so it is cached under those themselves.  A prover sends the
// same two programs proof after proof, so the most recent hits are tried first with one memcmp each (the structure of the
// reference circuit's gate program is 100+ KB: hashing it byte by byte cost 0.3 ms of host time per proof, with the device
// idle behind it); only a miss there hashes.
inline uint64_t gate_signature_key(const std::vector<uint8_t>& sig) {   // FNV-1a over 8-byte words, then the tail's bytes
  uint64_t key = 1469598103934665603ull;
  size_t i = 0;
  for (; i + 8 <= sig.size(); i += 8) {
    uint64_t w;
    std::memcpy(&w, sig.data() + i, 8);
    key = (key ^ w) * 1099511628211ull;
  }
  for (; i < sig.size(); i++) key = (key ^ sig[i]) * 1099511628211ull;
  return key;
}
struct GateProgramCache {
  static constexpr size_t CAPACITY = 64;
  std::map<uint64_t, GateProgram> programs;   // by key_of(signature)
  uint64_t recent[4] = {0, 0, 0, 0};          // keys of the programs used last (tried first, by comparison)
  uint32_t recent_next = 0;
  uint64_t (*key_of)(const std::vector<uint8_t>&) = gate_signature_key;   // (a seam for tests: colliding keys)

  // everything the lowered words depend on: the graph's structure, the column counts and the knobs of the lowering (a lane that
  // has compiled a graph under one GateLowering must not hand that program out under another)
  static std::vector<uint8_t> signature(const sg_graph& g, uint32_t n_fixed, uint32_t n_advice, uint32_t n_instance, uint32_t n_challenges,
                                        const GateLowering& how) {
    const uint64_t reload = how.reload_distance;
    const uint32_t hdr[12] = {g.n_constants, g.n_rotations, g.n_calculations, g.n_horner_parts, n_fixed, n_advice, n_instance, n_challenges,
                              (uint32_t)reload, (uint32_t)(reload >> 32), how.convert_at_load ? 1u : 0u, how.convert_at_load ? how.convert_above : 0u};
    const size_t parts[4] = {sizeof hdr, g.rotations ? sizeof(int32_t) * g.n_rotations : 0,
                             g.calculations ? sizeof(sg_calculation) * g.n_calculations : 0,
                             g.horner_parts ? sizeof(sg_value_source) * g.n_horner_parts : 0};
    const void* src[4] = {hdr, g.rotations, g.calculations, g.horner_parts};
    std::vector<uint8_t> sig(parts[0] + parts[1] + parts[2] + parts[3]);
    size_t at = 0;
    for (int i = 0; i < 4; i++) {
      if (parts[i]) std::memcpy(sig.data() + at, src[i], parts[i]);
      at += parts[i];
    }
    return sig;
  }
  // the cache is emptied when it is full; after reserve(n) the next n look-ups keep each other's programs
  void reserve(size_t n) {
    if (programs.size() + n >= CAPACITY) programs.clear();
  }
  // the program of a graph, compiled on first sight; *out stays valid until a later look-up compiles.  Returns
  // compile_gates' message.
  std::string lookup_or_compile(const sg_graph& g, uint32_t n_fixed, uint32_t n_advice, uint32_t n_instance, uint32_t n_challenges,
                                const GateLowering& how, GateProgram** out) {
    std::vector<uint8_t> sig = signature(g, n_fixed, n_advice, n_instance, n_challenges, how);
    auto hit = programs.end();
    for (uint64_t key : recent) {
      auto it = programs.find(key);
      if (it != programs.end() && it->second.signature == sig) {
        hit = it;
        break;
      }
    }
    uint64_t key = 0;
    if (hit == programs.end()) {
      key = key_of(sig);
      hit = programs.find(key);
      if (hit != programs.end() && hit->second.signature != sig) {  // 64-bit collision: recompile
        programs.erase(hit);
        hit = programs.end();
      }
    }
    if (hit == programs.end()) {
      GateProgram fresh;
      const std::string err = compile_gates(g, n_fixed, n_advice, n_instance, n_challenges, how, &fresh);
      if (!err.empty()) return err;
      fresh.signature = std::move(sig);
      if (programs.size() >= CAPACITY) programs.clear();
      hit = programs.emplace(key, std::move(fresh)).first;
    }
    if (std::find(recent, recent + 4, hit->first) == recent + 4) recent[recent_next++ % 4] = hit->first;
    *out = &hit->second;
    return "";
  }
};

}  // namespace sg
