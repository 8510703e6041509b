// registry_layout.h — the host-only arithmetic of the voter registry: the level
// table, the reserved (capacity) layout of a commitment registry, the dirty
// ranges of an append and the sorted, duplicate-free batch of a replace.  Plain
// C++ (no HIP): tools/registry_layout_check.cpp runs it under the sanitizers.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <numeric>
#include <vector>

namespace qpk {

// the circuit has MAX_MERKLE_DEPTH = 32 sibling slots and a 5-bit depth split:
// the deepest path a registry may hold is 31 (N <= 2^31)
constexpr uint32_t REG_PATH_SLOTS = 32, REG_MAX_DEPTH = 31, REG_MAX_LEVELS = REG_MAX_DEPTH + 1;
constexpr uint64_t REG_MAX_VOTERS = (uint64_t)1 << REG_MAX_DEPTH;
// from a level of at most this many nodes up, the rest of the tree is one launch
constexpr uint32_t REG_FOLD_MAX = 64;

// level offsets (in digests) and lengths, leaves first; the root is level nlevels - 1
struct RegistryLevels {
  uint32_t nlevels = 0;
  uint64_t off[REG_MAX_LEVELS] = {0}, len[REG_MAX_LEVELS] = {0};
  uint64_t total() const { return nlevels ? off[nlevels - 1] + len[nlevels - 1] : 0; }
  uint32_t max_depth() const { return nlevels - 1; }
};

// the digests a layout for `capacity` leaves reserves: level l holds
// ceil(capacity / 2^l) of them, down to the one root (0 for capacity 0 or > 2^31)
inline uint64_t registry_reserved(uint64_t capacity) {
  if (!capacity || capacity > REG_MAX_VOTERS) return 0;
  uint64_t o = 0;
  for (uint64_t len = capacity;; len = (len + 1) / 2) {
    o += len;
    if (len == 1) break;
  }
  return o;
}

// the table of n voters in a layout for `capacity` leaves: off[] from the
// capacity (every level the capacity can reach, so the tree grows in place),
// len[] and nlevels from n (n = 0: no levels).  With capacity == n it is
// registry_levels(n).  false (table untouched) unless n <= capacity, 1 <=
// capacity <= 2^31.
inline bool registry_levels_reserved(uint64_t n, uint64_t capacity, RegistryLevels &lv) {
  if (!capacity || capacity > REG_MAX_VOTERS || n > capacity) return false;
  RegistryLevels t;
  uint64_t o = 0;
  uint32_t l = 0;
  for (uint64_t len = capacity;; len = (len + 1) / 2) {
    t.off[l++] = o;
    o += len;
    if (len == 1) break;
  }
  for (uint64_t len = n; len; len = (len + 1) / 2) {
    t.len[t.nlevels++] = len;
    if (len == 1) break;
  }
  lv = t;
  return true;
}

// nodes [first, end) of one level
struct RegistryRange {
  uint64_t first = 0, end = 0;
};

// the nodes of every level that an append from n_old to n_new > n_old voters
// changes: level l's are [n_old >> l, ceil(n_new / 2^l)), one contiguous range
// whose source pairs start at 2 (n_old >> l), pair-aligned; a promoted lone
// last node lies inside it.  Returns the level count of n_new.
inline uint32_t registry_append_ranges(uint64_t n_old, uint64_t n_new, RegistryRange (&rg)[REG_MAX_LEVELS]) {
  uint32_t l = 0;
  for (uint64_t len = n_new; len; len = (len + 1) / 2, l++) {
    rg[l].first = n_old >> l;
    rg[l].end = len;
    if (len == 1) {
      l++;
      break;
    }
  }
  return l;
}

// the order that sorts a replace batch by voter index: order[b] = position in
// idx[] of the b-th smallest index.  false when an index is >= n (*bad = its
// position) or appears twice (*bad = the position of the second one in idx[]).
inline bool registry_replace_order(const uint64_t *idx, uint32_t k, uint64_t n, std::vector<uint32_t> &order,
                                   uint32_t *bad) {
  for (uint32_t b = 0; b < k; b++)
    if (idx[b] >= n) {
      *bad = b;
      return false;
    }
  order.resize(k);
  std::iota(order.begin(), order.end(), 0u);
  std::sort(order.begin(), order.end(),
            [idx](uint32_t a, uint32_t b) { return idx[a] != idx[b] ? idx[a] < idx[b] : a < b; });
  for (uint32_t b = 1; b < k; b++)
    if (idx[order[b]] == idx[order[b - 1]]) {
      *bad = order[b];
      return false;
    }
  return true;
}

}  // namespace qpk
