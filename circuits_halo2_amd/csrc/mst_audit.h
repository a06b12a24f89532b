// The range audit of a device-resident Merkle sum tree (mst_audit.cuh has the kernels, ss_mst_range_audit_dev in abi_mst.hip
// launches them): which nodes hold a balance the inclusion circuit's range check refuses, and which users' circuits fail for it.
//
// The reference builds its tree from any balances (mst.rs:103-134 checks no range); the circuit range-checks, with
// top = 2^(8 n_bytes) (circuits/merkle_sum_tree.rs:348-369, 424-438, in the order of synthesize):
//   the user's own leaf balances, the sibling leaf's balances at level 0, the sibling middle node's balances at every level above.
// The sums on the user's own path above the leaf are NOT range-checked, and the root's are left to verification: a user below an
// overflowing middle node whose siblings are all in range is provable, and the masks below say so.
//
//   flag    one byte per node of the level-major arrays (mst_level_first): 0 if every balance of the node is below top, else
//           1 + the lowest currency whose balance is not (n_currencies <= 64)
//   mask    one uint32 per leaf i, depth <= 30: bit 0 iff leaf i's flag is non-zero, bit l + 1 (0 <= l < depth) iff the flag of
//           node (i >> l) ^ 1 of level l is.  Bit for bit the list of range checks of leaf i's circuit; 0: all of them pass
//   list    the leaves with a non-zero mask in increasing order, the first bad_cap of them
//
// Steps, stream order the only barrier between them, no atomic decides where an output goes:
//   flags     a balance per thread (a wave's loads are 2 KB in a row): the canonical integer by one field product, the predicate,
//             then a node per thread gathers its currencies' bits; the wave's bad nodes by ballot, one atomic add per wave
//   masks     a leaf per thread walks its siblings in the flags; a wave's MST_AUDIT_TILE leaves are a tile: tile_count[tile]
//   groups    a workgroup scans MST_AUDIT_GROUP tile counts in place (exclusive) and leaves group_total[group]
//   scatter   a leaf per thread: its place = the totals of the groups before + the tile's prefix + its rank in the wave's ballot
// Plain C++ below, so that the rules and the tile and group edges are tested without a GPU (tests/cpp/mst_audit_check.cpp runs
// the serial steps, the list over the same tiles and groups).
#pragma once
#include "mst_csv.h"           // SG_HD
#include "mst_update_plan.h"   // mst_level_first

namespace sg {

static constexpr uint32_t MST_AUDIT_THREADS = 256;
static constexpr uint32_t MST_AUDIT_TILE = 64;                  // leaves whose count is one word of the scan: a wave's
static constexpr uint32_t MST_AUDIT_GROUP = MST_AUDIT_THREADS;  // tile counts a workgroup of the groups step scans
static constexpr uint32_t MST_AUDIT_MAX_DEPTH = 30, MST_AUDIT_MAX_CURRENCIES = 64, MST_AUDIT_MAX_BYTES = 31;

// Is the canonical integer w (eight little-endian 32-bit words, a value below r) below 2^(8 n_bytes)?  1 <= n_bytes <= 31: the
// bits from 8 n_bytes up are those of word (8 n_bytes) / 32 from bit (8 n_bytes) % 32 on, and every word above it.
SG_HD bool mst_audit_in_range(const uint32_t w[8], uint32_t n_bytes) {
  const uint32_t word = (8 * n_bytes) >> 5, bit = (8 * n_bytes) & 31;
  uint32_t above = 0;
#pragma unroll
  for (uint32_t k = 0; k < 8; k++) above |= k > word ? w[k] : k == word ? w[k] >> bit : 0u;
  return above == 0;
}

// the flag of a node from one bit per currency (bit c: balance c is out of range), nc <= 64
SG_HD uint8_t mst_audit_flag(uint64_t out_of_range) {
  if (!out_of_range) return 0;
  for (uint32_t c = 0; c < MST_AUDIT_MAX_CURRENCIES; c++)
    if ((out_of_range >> c) & 1) return (uint8_t)(1 + c);
  return 0;
}

// node i of level `level` in the level-major arrays; depth <= 30, so the number fits 32 bits (mst_level_first(level, depth) + i)
SG_HD uint32_t mst_audit_node(uint32_t level, uint32_t i, uint32_t depth) { return (2u << depth) - (2u << (depth - level)) + i; }
SG_HD uint32_t mst_audit_nodes(uint32_t depth) { return (2u << depth) - 1; }

// the reason mask of leaf i
SG_HD uint32_t mst_audit_mask(const uint8_t* flags, uint32_t i, uint32_t depth) {
  uint32_t mask = flags[i] ? 1u : 0u;
  for (uint32_t l = 0; l < depth; l++)
    if (flags[mst_audit_node(l, (i >> l) ^ 1u, depth)]) mask |= 2u << l;
  return mask;
}

// The work space in 32-bit words: what the host reads (bad nodes, unprovable leaves, the root's flag, a spare), the tiles'
// counts, the groups' totals.
static constexpr uint32_t MST_AUDIT_AT_BAD_NODES = 0, MST_AUDIT_AT_UNPROVABLE = 1, MST_AUDIT_AT_ROOT = 2, MST_AUDIT_FRONT_WORDS = 4;
SG_HD uint32_t mst_audit_tiles(uint32_t depth) { return (((uint32_t)1 << depth) + MST_AUDIT_TILE - 1) / MST_AUDIT_TILE; }
SG_HD uint32_t mst_audit_groups(uint32_t depth) { return (mst_audit_tiles(depth) + MST_AUDIT_GROUP - 1) / MST_AUDIT_GROUP; }
SG_HD uint32_t mst_audit_at_tiles() { return MST_AUDIT_FRONT_WORDS; }
SG_HD uint32_t mst_audit_at_groups(uint32_t depth) { return mst_audit_at_tiles() + mst_audit_tiles(depth); }
// the size of d_scratch in bytes: 4 * (4 + tiles + groups), tiles = ceil(2^depth / 64), groups = ceil(tiles / 256)
SG_HD uint64_t mst_audit_scratch_bytes(uint32_t depth) { return 4ull * (mst_audit_at_groups(depth) + mst_audit_groups(depth)); }

// What ss_mst_range_audit_dev refuses before it touches a device: "" or what is wrong with the call.
inline std::string mst_audit_problem(const void* d_node_balances, uint32_t depth, uint32_t nc, uint32_t n_bytes, const void* d_node_flags,
                                     const void* d_leaf_reasons, const void* d_bad_leaves, uint64_t bad_cap, const void* d_scratch,
                                     const void* summary_out) {
  if ((uintptr_t)d_node_balances & 15) return "d_node_balances is not 16-byte aligned";
  if (!d_node_balances || !d_node_flags || !d_leaf_reasons || !d_scratch || !summary_out) return "null argument";
  if (!d_bad_leaves && bad_cap) return "null d_bad_leaves with a non-zero bad_cap";
  if (depth > MST_AUDIT_MAX_DEPTH) return "depth above 30";
  if (nc == 0 || nc > MST_AUDIT_MAX_CURRENCIES) return "n_currencies outside 1..64";
  if (n_bytes == 0 || n_bytes > MST_AUDIT_MAX_BYTES) return "n_bytes outside 1..31";
  if ((uintptr_t)d_leaf_reasons & 3) return "d_leaf_reasons is not 4-byte aligned";
  if ((uintptr_t)d_bad_leaves & 3) return "d_bad_leaves is not 4-byte aligned";
  if ((uintptr_t)d_scratch & 3) return "d_scratch is not 4-byte aligned";
  return "";
}

// ------------------------------------------------------------------ the steps on the host, one after the other
struct MstAuditHost {
  std::vector<uint8_t> flags;       // 2^(depth + 1) - 1
  std::vector<uint32_t> masks;      // 2^depth
  std::vector<uint32_t> bad;        // the first bad_cap leaves with a non-zero mask
  uint64_t summary[4] = {0, 0, 0, 0};   // bad nodes, unprovable leaves, leaves listed, the root's flag
};
// canon: the canonical integers of the node balances, level-major, nc x 8 words a node
inline MstAuditHost mst_audit_host(const uint32_t* canon, uint32_t depth, uint32_t nc, uint32_t n_bytes, uint64_t bad_cap) {
  MstAuditHost r;
  const uint32_t nodes = mst_audit_nodes(depth), leaves = (uint32_t)1 << depth;
  r.flags.resize(nodes);
  for (uint32_t node = 0; node < nodes; node++) {            // flags
    uint64_t bits = 0;
    for (uint32_t c = 0; c < nc; c++)
      if (!mst_audit_in_range(canon + 8 * ((size_t)node * nc + c), n_bytes)) bits |= (uint64_t)1 << c;
    r.flags[node] = mst_audit_flag(bits);
    r.summary[0] += r.flags[node] != 0;
  }
  const uint32_t tiles = mst_audit_tiles(depth), groups = mst_audit_groups(depth);
  std::vector<uint32_t> work(mst_audit_scratch_bytes(depth) / 4, 0);
  uint32_t *tile_count = work.data() + mst_audit_at_tiles(), *group_total = work.data() + mst_audit_at_groups(depth);
  r.masks.resize(leaves);
  for (uint32_t i = 0; i < leaves; i++) {                    // masks
    r.masks[i] = mst_audit_mask(r.flags.data(), i, depth);
    tile_count[i / MST_AUDIT_TILE] += r.masks[i] != 0;
  }
  for (uint32_t g = 0; g < groups; g++) {                    // groups: exclusive in place, the total aside
    uint32_t before = 0;
    for (uint32_t t = g * MST_AUDIT_GROUP; t < tiles && t < (g + 1) * MST_AUDIT_GROUP; t++) {
      const uint32_t count = tile_count[t];
      tile_count[t] = before;
      before += count;
    }
    group_total[g] = before;
  }
  uint32_t rank = 0;                                         // scatter
  for (uint32_t i = 0; i < leaves; i++) {
    if (i % MST_AUDIT_TILE == 0) rank = 0;
    if (!r.masks[i]) continue;
    const uint32_t tile = i / MST_AUDIT_TILE, group = tile / MST_AUDIT_GROUP;
    uint64_t at = (uint64_t)tile_count[tile] + rank++;
    for (uint32_t g = 0; g < group; g++) at += group_total[g];
    if (at < bad_cap) {
      if (r.bad.size() <= at) r.bad.resize(at + 1, 0xffffffffu);
      r.bad[at] = i;
    }
  }
  for (uint32_t g = 0; g < groups; g++) r.summary[1] += group_total[g];
  r.summary[2] = r.summary[1] < bad_cap ? r.summary[1] : bad_cap;
  r.summary[3] = r.flags[nodes - 1];
  return r;
}

#if defined(__HIPCC__)
// the four steps on `stream`; d_work: mst_audit_scratch_bytes(depth), its front zeroed by the caller in stream order
hipError_t mst_audit_launch(const void* d_node_balances, uint32_t depth, uint32_t nc, uint32_t n_bytes, uint8_t* d_flags, uint32_t* d_masks,
                            uint32_t* d_bad, uint64_t bad_cap, uint32_t* d_work, hipStream_t stream);
#endif

}  // namespace sg
