// The MSM engine's planning (csrc/msm_plan.h) run on the CPU: reads one job per line from stdin,
//   n M fixed c jobs_in_flight cus largest_bucket tasks [name=value ...]
// (c = 0: the engine chooses; tasks = 0: the host's upper bound; name: a field of MsmConfig), and prints what the engine would
// plan for it, one line per job: the fields tests/msm_cases.py restates (expected_backend, accumulate_threads, auto_log_seg,
// generic_window_bits, window_plan), the kernel names in launch order derived from the plan's dispatch fields, or "invalid".
// tests/test_msm_cases_cpu.py builds it with plain g++ and compares the two, field by field.
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "msm_plan.h"

using namespace sg;

static bool set_param(MsmConfig& cfg, const std::string& name, uint32_t v) {
  const struct { const char* name; uint32_t MsmConfig::*field; } table[] = {
      {"window_bits", &MsmConfig::window_bits}, {"log_seg", &MsmConfig::log_seg}, {"red_threads", &MsmConfig::red_threads},
      {"log_red_chunk", &MsmConfig::log_red_chunk}, {"two_pass", &MsmConfig::two_pass},
      {"log_scatter_rounds", &MsmConfig::log_scatter_rounds}, {"acc_threads", &MsmConfig::acc_threads},
      {"acc_waves", &MsmConfig::acc_waves}, {"acc_waves_fixed", &MsmConfig::acc_waves_fixed},
      {"merge_quad_tasks", &MsmConfig::merge_quad_tasks}, {"red2d_max_sets", &MsmConfig::red2d_max_sets},
      {"red2d", &MsmConfig::red2d}, {"red2d_fold", &MsmConfig::red2d_fold}, {"red2d_prefold", &MsmConfig::red2d_prefold},
      {"prefold_quad_buckets", &MsmConfig::prefold_quad_buckets}, {"red_lean", &MsmConfig::red_lean},
      {"fused_frontend", &MsmConfig::fused_frontend}, {"quad", &MsmConfig::quad}};
  for (const auto& row : table)
    if (name == row.name) {
      cfg.*row.field = v;
      return true;
    }
  return false;
}

static std::string opt(uint32_t v, bool present) { return present ? std::to_string(v) : "-"; }

// the kernels of the back end in launch order, from the dispatch fields alone
static std::string kernels(const FrontPlan& f, const ReducePlan& r, uint32_t tasks, uint32_t largest, uint32_t* rounds) {
  std::string k = "msm_accumulate";
  *rounds = 0;
  for (MergeRound m = merge_rounds(f, tasks, largest); merge_round_next(f, r, m); ++*rounds)
    k += m.quad ? ",msm_merge<4>" : ",msm_merge<1>";
  const char* q = r.quad ? "<4>" : "<1>";
  if (r.red2d) {
    if (r.prefold) k += std::string(r.fold_quad ? ",msm_fold_buckets<4>" : ",msm_fold_buckets<1>") + ",msm_reduce2d_lines_folded" + q;
    else k += std::string(",msm_reduce2d_lines") + q;
    k += std::string(",msm_reduce2d_bits") + q;
    if (r.combine) k += ",msm_reduce2d_combine";
    return k + ",msm_export_points";
  }
  k += r.quad ? ",msm_reduce_buckets<4>" : r.lean ? ",msm_reduce_buckets_lean<1>" : ",msm_reduce_buckets<1>";
  if (r.T1) k += r.items_quad ? ",msm_reduce_items<4>" : ",msm_reduce_items<1>";
  return k + ",msm_export_windows";
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    unsigned long long n = 0, M = 0;
    uint32_t fixed = 0, c = 0, jobs = 1, cus = 0, largest = 0, tasks = 0;
    if (!(in >> n >> M >> fixed >> c >> jobs >> cus >> largest >> tasks)) {
      std::fprintf(stderr, "bad case: %s\n", line.c_str());
      return 2;
    }
    MsmConfig cfg;
    for (std::string kv; in >> kv;) {
      const size_t eq = kv.find('=');
      if (eq == std::string::npos || !set_param(cfg, kv.substr(0, eq), (uint32_t)std::stoul(kv.substr(eq + 1)))) {
        std::fprintf(stderr, "bad parameter: %s\n", kv.c_str());
        return 2;
      }
    }
    if (!fixed && c) cfg.window_bits = c;
    const bool others = jobs >= 2;
    const WindowPlan table = make_window_plan(fixed ? c : 4);   // a fixed-base job brings its table's plan
    const FrontPlan f = plan_front(cfg, M, n, fixed ? &table : nullptr, c, n, others);
    if (!f.valid || f.trivial) {
      std::puts("invalid");
      continue;
    }
    const AccPlan a = plan_accumulate(f, cfg, cus, others);
    const ReducePlan r = plan_reduce(f, cfg, others);
    if (!r.valid) {
      std::puts("invalid");
      continue;
    }
    uint32_t rounds = 0;
    const std::string ks = kernels(f, r, tasks ? tasks : a.ntasks_ub, largest, &rounds);
    std::string widths;
    for (uint32_t w = 0; w < f.wp.W; w++) widths += (w ? "," : "") + std::to_string(f.wp.width[w]);
    const bool scan = !r.red2d;
    std::printf("c=%u windows=%u widths=%s sets=%u log_seg=%u quad=%u red2d=%u fold=%u log_G=%s threads=%s blocks=%s T1=%s "
                "merge_rounds=%u per_win=%u kernels=%s acc_threads=%u\n",
                f.c, f.W1, widths.c_str(), f.sets, f.log_L, r.quad ? 1u : 0u, r.red2d, r.fold, opt(r.log_G, scan).c_str(),
                opt(r.threads, scan).c_str(), opt(r.blocks, scan).c_str(), opt(r.T1, scan && r.T1).c_str(), rounds, r.per_win,
                ks.c_str(), a.total_threads());
  }
  return 0;
}
