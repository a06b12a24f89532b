// Launch geometry of sg_mst_update_dev, an in-place update of m leaves of a built Merkle sum tree (mst.rs:169-204 for many
// leaves at once): which nodes of every level above the leaves have an updated leaf below them.  Decided on the host, plain
// C++ without HIP (tests/cpp/mst_update_plan_check.cpp): the kernels of witness.hip take one list per level and one launch
// per level, and stream order between the launches is the only barrier between the levels.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "mst_entries.h"

namespace sg {

// The level-major node arrays of a tree of 2^depth leaves: the leaves, then the 2^(depth - 1) parents, .., the root.  The first
// node of level `level` <= depth: 2^depth + .. + 2^(depth - level + 1) = 2^(depth + 1) - 2^(depth - level + 1); depth <= 62.
inline uint64_t mst_level_first(uint32_t level, uint32_t depth) { return ((uint64_t)2 << depth) - ((uint64_t)2 << (depth - level)); }

// For level l = 1 .. depth the distinct parents {index >> l} of the updated leaves, as node numbers within their level,
// strictly increasing; the lists back to back in `nodes`, list l = nodes[offset[l - 1] .. offset[l]), offset[0] = 0.
// At most m entries per list, all lists together fewer than 2^depth (the nodes above the leaves); the last list is {0}.
struct MstUpdatePlan {
  std::vector<uint32_t> nodes;
  std::vector<uint32_t> offset;   // depth + 1 entries
  uint32_t count(uint32_t level) const { return offset[level] - offset[level - 1]; }
  const uint32_t* list(uint32_t level) const { return nodes.data() + offset[level - 1]; }
};

// `index`: m leaf numbers, strictly increasing, each below 2^depth (mst_update_problem refuses anything else).  Equal parents
// of a sorted list are neighbours, so every level is one pass over the level below.
inline MstUpdatePlan mst_update_plan(const uint32_t* index, size_t m, uint32_t depth) {
  MstUpdatePlan plan;
  plan.offset.assign((size_t)depth + 1, 0);
  size_t below_first = 0, below_count = m;   // the list of the level below: `index` itself under level 1
  for (uint32_t level = 1; level <= depth; level++) {
    const size_t first = plan.nodes.size();
    for (size_t t = 0; t < below_count; t++) {
      const uint32_t parent = (level == 1 ? index[t] : plan.nodes[below_first + t]) >> 1;
      if (plan.nodes.size() == first || plan.nodes.back() != parent) plan.nodes.push_back(parent);
    }
    plan.offset[level] = (uint32_t)plan.nodes.size();
    below_first = first;
    below_count = plan.nodes.size() - first;
  }
  return plan;
}

// What sg_mst_update_dev refuses before it touches the device: "" if `index` and the m * nc balance fields describe an
// update of a tree of 2^depth leaves, else what is wrong with them (the first offending position).
inline std::string mst_update_problem(const uint32_t* index, const uint8_t* digit_bytes, const uint64_t* digit_off, size_t m,
                                      uint32_t depth, uint32_t nc) {
  if (depth > 30) return "depth above 30";
  const uint64_t leaves = (uint64_t)1 << depth;
  if (m == 0) return "no leaf to update";
  if (m > leaves) return "more leaves to update than the tree has";
  for (size_t j = 0; j < m; j++) {
    if (index[j] >= leaves) return "leaf index " + std::to_string(index[j]) + " at position " + std::to_string(j) + " is out of range";
    if (j && index[j] <= index[j - 1]) return "leaf indices do not strictly increase at position " + std::to_string(j);
  }
  return mst_digit_fields_problem(digit_bytes, digit_off, m * (size_t)nc);
}

}  // namespace sg
