// The NTT engine's planning (csrc/ntt_plan.h) run on the CPU: reads one job per line from stdin,
//   log_n in_len nbatch scale pre3 post3 pre_tab [name=value ...]
// (nbatch = 0: a single transform, NttEngine::transform; scale / pre3 / post3 / pre_tab: 0 or 1, whether the call brings a plain
// scale, three pre factors, three post factors, a table for the load; name: a field of NttConfig, so radix4 counts as the struct
// does: 0 never, 1 the throughput shapes, 2 always), and prints what the engine would launch for it, one line per job: the plan,
// then every pass with its geometry, its workgroup and what rides on its load and store.
// tests/test_ntt_cases_cpu.py builds it with plain g++ and compares it with the restatement in tests/ntt_cases.py, field by field.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "ntt_plan.h"

using namespace sg;

static bool set_param(NttConfig& cfg, const std::string& name, uint32_t v) {
  const struct { const char* name; uint32_t NttConfig::*field; } table[] = {
      {"max_single_log", &NttConfig::max_single_log}, {"max_multi_log", &NttConfig::max_multi_log}, {"tile_log", &NttConfig::tile_log},
      {"threads", &NttConfig::threads}, {"big_tile_log", &NttConfig::big_tile_log}, {"big_threads", &NttConfig::big_threads},
      {"batch_min", &NttConfig::batch_min}, {"big_log", &NttConfig::big_log}, {"radix4", &NttConfig::radix4}};
  for (const auto& row : table)
    if (name == row.name) {
      cfg.*row.field = v;
      return true;
    }
  return false;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    uint32_t log_n = 0, in_len = 0, nbatch = 0, scale = 0, pre3 = 0, post3 = 0, pre_tab = 0;
    if (!(in >> log_n >> in_len >> nbatch >> scale >> pre3 >> post3 >> pre_tab) || log_n < 1 || log_n > 28 || nbatch > NTT_BATCH_MAX) {
      std::fprintf(stderr, "bad case: %s\n", line.c_str());
      return 2;
    }
    NttConfig cfg;
    for (std::string kv; in >> kv;) {
      const size_t eq = kv.find('=');
      if (eq == std::string::npos || !set_param(cfg, kv.substr(0, eq), (uint32_t)std::stoul(kv.substr(eq + 1)))) {
        std::fprintf(stderr, "bad parameter: %s\n", kv.c_str());
        return 2;
      }
    }
    const NttFactors f = ntt_factor(cfg, log_n);
    const bool in_table = ntt_scale_in_table(f, scale != 0, post3 != 0);
    // (scratch: whether an in-place call of this size needs the scratch vector)
    std::printf("npass=%d l=%u,%u,%u scale_in_table=%d batched=%d scratch=%d", f.npass, f.l[0], f.l[1], f.l[2], in_table ? 1 : 0,
                ntt_batched(log_n) ? 1 : 0, ntt_needs_scratch(cfg, log_n, true) ? 1 : 0);
    for (int i = 0; i < f.npass; i++) {
      const NttPassGeom g = ntt_pass_geom(f, i);
      const NttPassRide r = ntt_pass_ride(f, i, in_len, scale != 0, pre3 != 0, post3 != 0, pre_tab != 0);
      const NttPassShape s = ntt_pass_shape(cfg, g, log_n, r.in_len, nbatch);
      std::printf(" | kind=%c log_r=%u log_b=%u sig=%u,%u skip=%u big=%d log_t=%u E=%zu r4=%u threads=%u grid=%u,%u lds=%zu pre3=%d pre_tab=%d "
                  "post3=%d fold29=%u tw_pass=%d",
                  g.kind ? 'X' : 'Y', g.log_r, g.log_b, g.sig_lo, g.sig_hi, s.skip, s.big ? 1 : 0, s.log_t, s.elems, s.radix4, s.threads,
                  s.grid_x, s.grid_y, s.lds_bytes, r.pre3 ? 1 : 0, r.pre_tab ? 1 : 0, r.post != NTT_POST_NONE ? 1 : 0, g.fold29, g.tw_pass);
    }
    std::printf("\n");
  }
  return 0;
}
