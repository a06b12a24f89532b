// The host side of the custom-gate block (csrc/gates_compile.h) run on the CPU.  Reads one request per line from stdin and answers
// each on stdout:
//   words G      the lowering of a graph: "words n_slots result_kind result_index n_ops (w0 dst a b)..." or "error <message>"
//   dump G       the same as a listing with its slot pressure, one instruction per line, then "end"
//   tile s c     gates_interpreter_tile for s live values and c constants
//   cache        exercises GateProgramCache; "cache ok", or what went wrong
// G, all integers: n_fixed n_advice n_instance n_challenges reload_distance convert_above(-1: off) n_constants n_rotations
//   n_calculations n_horner_parts null_mask(1 constants, 2 rotations, 4 calculations, 8 parts: handed over as null pointers)
//   rotations...  (op a.kind a.index a.rotation b.kind b.index b.rotation parts_offset parts_len)...  (kind index rotation)...
// tests/test_gates_cases_cpu.py builds it with g++ and the address and undefined-behaviour sanitizers; tests/gates_cases.py
// writes the requests.
#include <pthread.h>

#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "gates_compile.h"

using namespace sg;

struct Request {
  uint32_t dims[4];
  GateLowering how;
  std::vector<uint8_t> constants;
  std::vector<int32_t> rotations;
  std::vector<sg_calculation> calcs;
  std::vector<sg_value_source> parts;
  sg_graph g;
};

static bool parse(std::istringstream& in, Request* r) {
  long long reload, convert, n_const, n_rot, n_calc, n_parts, null_mask;
  if (!(in >> r->dims[0] >> r->dims[1] >> r->dims[2] >> r->dims[3] >> reload >> convert >> n_const >> n_rot >> n_calc >> n_parts >> null_mask)) return false;
  r->how.reload_distance = (size_t)reload;
  r->how.convert_at_load = convert >= 0;
  r->how.convert_above = convert >= 0 ? (uint32_t)convert : 0;
  r->constants.assign(32 * (size_t)std::max<long long>(1, n_const), 0);
  r->rotations.resize((size_t)n_rot);
  for (int32_t& x : r->rotations)
    if (!(in >> x)) return false;
  auto source = [&](sg_value_source& s) { return (bool)(in >> s.kind >> s.index >> s.rotation); };
  r->calcs.resize((size_t)n_calc);
  for (sg_calculation& c : r->calcs)
    if (!(in >> c.op) || !source(c.a) || !source(c.b) || !(in >> c.parts_offset >> c.parts_len)) return false;
  r->parts.resize((size_t)n_parts);
  for (sg_value_source& s : r->parts)
    if (!source(s)) return false;
  r->g = sg_graph{null_mask & 1 ? nullptr : r->constants.data(), (uint32_t)n_const, null_mask & 2 ? nullptr : r->rotations.data(), (uint32_t)n_rot,
                  null_mask & 4 ? nullptr : r->calcs.data(), (uint32_t)n_calc, null_mask & 8 ? nullptr : r->parts.data(), (uint32_t)n_parts};
  return true;
}

// the lowered program with its slot pressure.  Not the allocator's own view: `live` and `last use` are derived again here from
// the encoded words alone (a slot is live from the instruction that writes it to the last one that reads it before it is
// written again), which is what the device sees.  Per instruction: the values still to be read after it, and the last
// instruction that reads what it wrote (0: never read; 4294967295: the result)
static void dump(const GateProgram& p) {
  static const char* names[] = {"loadcol", "loadprev", "add", "sub", "mul", "sqr", "dbl", "neg", "red", "muladd"};
  const uint32_t n = (uint32_t)p.ops.size(), END = 0xffffffffu;
  auto reads = [&](const GateOp& o, uint32_t slot) {
    const uint32_t code = o.w0 & 0xff;
    if (code == G_LOADCOL || code == G_LOADPREV) return false;
    return (((o.w0 >> 16) & 0xff) == GK_SLOT && o.a == slot) || ((o.w0 >> 24) == GK_SLOT && o.b == slot) ||
           (code == G_MULADD && ((o.w0 >> 8) & 0xff) == GK_SLOT && (o.dst >> 16) == slot);
  };
  std::vector<uint32_t> last(n, 0);
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t d = p.ops[i].dst & 0xffff;
    uint32_t j = i + 1;
    for (; j < n; j++) {
      if (reads(p.ops[j], d)) last[i] = j;
      if ((p.ops[j].dst & 0xffff) == d) break;
    }
    if (j == n && p.result_kind == GK_SLOT && p.result_index == d) last[i] = END;
  }
  for (uint32_t i = 0; i < n; i++) {
    const GateOp& o = p.ops[i];
    const uint32_t code = o.w0 & 0xff;
    const bool load = code == G_LOADCOL || code == G_LOADPREV;
    uint32_t live = 0;
    for (uint32_t v = 0; v <= i; v++) live += last[v] > i;
    std::printf("%3u %-8s dst s%-2u", i, code < 10 ? names[code] : "?", o.dst & 0xffff);
    if (load) std::printf(" col %u rot %d", o.a, (int32_t)o.b);
    else std::printf(" %c%u %c%u", ((o.w0 >> 16) & 0xff) == GK_SLOT ? 's' : 'c', o.a, (o.w0 >> 24) == GK_SLOT ? 's' : 'c', o.b);
    if (code == G_MULADD) std::printf(" %c%u", ((o.w0 >> 8) & 0xff) == GK_SLOT ? 's' : 'c', o.dst >> 16);
    std::printf("   live %u (last use of dst: %u)\n", live, last[i]);
  }
  std::printf("end\n");
}

// ---- GateProgramCache: graphs of one calculation that differ in their number of advice columns
static unsigned g_hashed = 0;
static uint64_t counting_key(const std::vector<uint8_t>& sig) { return g_hashed++, gate_signature_key(sig); }
static uint64_t colliding_key(const std::vector<uint8_t>&) { return 7; }

static const char* cache_check() {
  static const int32_t rot[1] = {0};
  static const sg_calculation cal[1] = {{SG_OP_SQUARE, {SG_VS_ADVICE, 0, 0}, {0, 0, 0}, 0, 0}};
  const sg_graph g{nullptr, 0, rot, 1, cal, 1, nullptr, 0};
  const GateLowering how;
  auto look = [&](GateProgramCache& c, uint32_t n_advice) {
    GateProgram* p = nullptr;
    return c.lookup_or_compile(g, 0, n_advice, 0, 0, how, &p).empty() && p->n_columns == n_advice && p->ops.size() == 3 ? p : nullptr;
  };
  g_hashed = 0;
  {  // a recent hit compares and does not hash
    GateProgramCache c;
    c.key_of = counting_key;
    GateProgram* first = look(c, 1);
    if (!first || g_hashed != 1) return "first sight hashes once";
    if (look(c, 1) != first || g_hashed != 1) return "a recent hit returns the same program without hashing";
    for (uint32_t i = 2; i <= 5; i++)
      if (!look(c, i)) return "compile";
    if (g_hashed != 5 || look(c, 1) != first || g_hashed != 6) return "the fifth program back is found by its key";
    GateProgram* p = nullptr;
    const sg_graph empty{nullptr, 0, rot, 1, cal, 0, nullptr, 0};
    if (c.lookup_or_compile(empty, 0, 1, 0, 0, how, &p) != "empty program" || c.programs.size() != 5) return "a refused graph is not kept";
  }
  {  // two structures under one key: the newcomer replaces the other, and each look-up gets its own program
    GateProgramCache c;
    c.key_of = colliding_key;
    if (!look(c, 1) || !look(c, 2) || c.programs.size() != 1) return "a collision recompiles";
    if (!look(c, 1) || c.programs.size() != 1 || !look(c, 1)) return "and again for the first";
  }
  {  // full at 64: the 65th empties it
    GateProgramCache c;
    for (uint32_t i = 1; i <= 64; i++)
      if (!look(c, i) || c.programs.size() != i) return "64 programs are kept";
    if (!look(c, 65) || c.programs.size() != 1) return "the 65th clears";
  }
  for (uint32_t before : {61u, 62u}) {  // reserve(2): the next two look-ups keep each other's program
    GateProgramCache c;
    for (uint32_t i = 1; i <= before; i++)
      if (!look(c, i)) return "compile";
    c.reserve(2);
    if (c.programs.size() != (before == 61 ? 61u : 0u)) return "reserve(2) clears from 62 programs on";
    GateProgram *a = look(c, 101), *b = look(c, 102);
    if (!a || !b || a == b || c.programs.size() != (before == 61 ? 63u : 2u) || a->n_columns != 101 || a->signature.empty()) return "a reserved pair stays";
  }
  {  // one graph, several lowerings, one cache: each GateLowering gets the program compile_gates gives for it, and keeps it
    static const int32_t rots[2] = {0, 1};
    const sg_value_source a0{SG_VS_ADVICE, 0, 0}, a1{SG_VS_ADVICE, 0, 1}, none{0, 0, 0};
    std::vector<sg_calculation> cals;   // the two cells of a column, added over and over: 40 additions, then their square
    cals.push_back({SG_OP_ADD, a0, a1, 0, 0});
    for (uint32_t i = 1; i < 40; i++) cals.push_back({SG_OP_ADD, {SG_VS_INTERMEDIATE, i - 1, 0}, i % 2 ? a0 : a1, 0, 0});
    cals.push_back({SG_OP_SQUARE, {SG_VS_INTERMEDIATE, 39, 0}, none, 0, 0});
    const sg_graph chain{nullptr, 0, rots, 2, cals.data(), (uint32_t)cals.size(), nullptr, 0};
    GateLowering plain, never_reuse, convert;
    never_reuse.reload_distance = 0;
    convert.convert_at_load = true;
    convert.convert_above = 1;
    GateProgramCache c;
    auto same = [](const GateProgram& p, const GateProgram& q) {
      return p.n_slots == q.n_slots && p.result_kind == q.result_kind && p.result_index == q.result_index && p.ops.size() == q.ops.size() &&
             (p.ops.empty() || std::memcmp(p.ops.data(), q.ops.data(), p.ops.size() * sizeof(GateOp)) == 0);
    };
    std::vector<GateProgram> fresh(3), got;
    const GateLowering* hows[3] = {&plain, &never_reuse, &convert};
    for (int round = 0; round < 2; round++)
      for (int i = 0; i < 3; i++) {
        GateProgram* p = nullptr;
        if (!compile_gates(chain, 0, 1, 0, 0, *hows[i], &fresh[i]).empty() || !c.lookup_or_compile(chain, 0, 1, 0, 0, *hows[i], &p).empty()) return "compile";
        if (!same(*p, fresh[i])) return "a look-up gives the program of its own lowering";
        if (round == 0) got.push_back(*p);
      }
    if (same(got[0], got[1]) || same(got[0], got[2]) || same(got[1], got[2])) return "different lowerings give different programs";
    if (c.programs.size() != 3) return "one entry per lowering";
    GateLowering off_but_above = plain;   // convert_above means nothing while convert_at_load is off: the same entry
    off_but_above.convert_above = 9;
    GateProgram* p = nullptr;
    if (!c.lookup_or_compile(chain, 0, 1, 0, 0, off_but_above, &p).empty() || !same(*p, fresh[0]) || c.programs.size() != 3) return "an idle knob is no new entry";
  }
  return nullptr;
}

static bool answer(const std::string& line) {
  std::istringstream in(line);
  std::string what;
  if (!(in >> what)) return false;
  if (what == "tile") {
    uint32_t s = 0, c = 0;
    if (!(in >> s >> c)) return false;
    const GateTile t = gates_interpreter_tile(s, c);
    std::printf("tile slots=%u consts=%u rows=%u lds=%zu fits=%d waves=%u\n", s, c, t.rows, t.lds_bytes, (int)t.fits, t.waves);
    return true;
  }
  if (what == "cache") {
    const char* wrong = cache_check();
    std::printf("cache %s\n", wrong ? wrong : "ok");
    return true;
  }
  if (what != "words" && what != "dump") return false;
  Request r;
  if (!parse(in, &r)) return false;
  GateProgram p;
  const std::string err = compile_gates(r.g, r.dims[0], r.dims[1], r.dims[2], r.dims[3], r.how, &p);
  if (!err.empty()) {
    std::printf("error %s\n", err.c_str());
  } else if (what == "dump") {
    dump(p);
  } else {
    std::printf("words %u %u %u %zu", p.n_slots, p.result_kind, p.result_index, p.ops.size());
    for (const GateOp& o : p.ops) std::printf(" %u %u %u %u", o.w0, o.dst, o.a, o.b);
    std::printf("\n");
  }
  return true;
}

static void* serve(void*) {
  static int status = 0;
  std::string line;
  while (!status && std::getline(std::cin, line))
    if (!line.empty() && !answer(line)) status = (std::fprintf(stderr, "bad request: %.60s\n", line.c_str()), 2);
  return &status;
}

// on a stack of its own: the lowering recurses up to 4096 calculations deep, and an instrumented build has large frames
int main() {
  pthread_attr_t attr;
  pthread_t thread;
  void* status = nullptr;
  if (pthread_attr_init(&attr) || pthread_attr_setstacksize(&attr, (size_t)256 << 20) || pthread_create(&thread, &attr, serve, nullptr) ||
      pthread_join(thread, &status))
    return std::fprintf(stderr, "no thread\n"), 3;
  return *static_cast<int*>(status);
}
