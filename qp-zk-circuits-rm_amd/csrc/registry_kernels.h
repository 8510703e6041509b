// registry_kernels.h — argument layouts and launchers of registry.hip: the
// voter registry's eligibility tree (voting/src/lib.rs:285-316) and the Merkle
// paths the voting circuit walks (:123-180).  One launcher per step; the
// launcher owns the kernel choice and the grid, block and LDS sizes.
//
// Tree convention (the reference's): leaf = hash_no_pad(4-felt key), node =
// hash_no_pad(left || right), and the last node of an odd-length level moves
// to the next level unchanged.  Level l holds ceil(N / 2^l) nodes; every
// level stays resident, [level][node][4] felts.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "registry_layout.h"

namespace qpk {

// the table for n voters; false (table untouched) for n = 0 or a path deeper than REG_MAX_DEPTH
bool registry_levels(uint64_t n, RegistryLevels &lv);

__global__ void k_registry_leaves(const uint64_t *keys, uint64_t n, uint64_t *dig);
__global__ void k_registry_level(const uint64_t *src, uint64_t nsrc, uint64_t *dst);
__global__ void k_registry_fold(uint64_t *dig, RegistryLevels lv, uint32_t l0);
__global__ void k_registry_paths(const uint64_t *dig, RegistryLevels lv, const uint64_t *idx, uint32_t nidx,
                                 uint64_t *siblings, uint32_t *path_bits, uint32_t *depth, uint64_t *leaves);

// leaf digests: keys key-major [4][n] (felt k of voter i at keys[k n + i]) -> dig[i][4]
void registry_leaves(const uint64_t *keys, uint64_t n, uint64_t *dig, hipStream_t s);
// every level above the leaves, appended after them (dig: lv.total() digests):
// one launch per level wider than REG_FOLD_MAX, then the rest in one workgroup
void registry_tree(uint64_t *dig, const RegistryLevels &lv, hipStream_t s);
// the paths of voters idx[b] < n (the caller checks the bound): siblings
// [nidx][REG_PATH_SLOTS][4] compacted to the levels where the voter's node was
// hashed (the zero digest above the depth), path_bits[b] bit j = side of
// sibling j (1: the voter's node is the right child), depth[b] = siblings;
// leaves (may be null) [nidx][4] = the voters' leaf digests
void registry_paths(const uint64_t *dig, const RegistryLevels &lv, const uint64_t *idx, uint32_t nidx,
                    uint64_t *siblings, uint32_t *path_bits, uint32_t *depth, uint64_t *leaves, hipStream_t s);

// ---- updates of a commitment registry (a reserved layout: off[] from the
// capacity, len[] / nlevels from the current n; registry_layout.h).  Level 0
// is already written when these run; each recomputes the nodes above it that
// the update changes, level by level in launch order, every loop bound from
// the host's table.
// Dirty ranges narrower than this run in the row form (16 lanes per node,
// pc::permute_row) at every level up to the root: measured against the
// one-lane form it wins or ties at every range width up to this one, the
// widest measured (DESIGN §12 has the A/B).  Wider ranges go through
// k_registry_level on the level's suffix and, from a level of at most
// REG_FOLD_MAX nodes, k_registry_fold.  Path hook registry_row=N overrides
// the bound (0 = never the row form).
constexpr long REG_ROW_MAX = 32768;

__global__ void k_registry_range_row(uint64_t *dig, RegistryLevels lv, uint32_t level, uint64_t first, uint32_t count);
__global__ void k_registry_put(uint64_t *dig, const uint64_t *idx, const uint64_t *leaves, uint32_t k);
__global__ void k_registry_scatter(uint64_t *dig, RegistryLevels lv, uint32_t level, const uint64_t *idx, uint32_t k);
__global__ void k_registry_scatter_row(uint64_t *dig, RegistryLevels lv, uint32_t level, const uint64_t *idx,
                                       uint32_t k);

// the levels above the leaves after voters [n_old, lv.len[0]) were written into
// level 0 (lv: the table of the new size); n_old = 0 builds the whole tree
void registry_append(uint64_t *dig, const RegistryLevels &lv, uint64_t n_old, hipStream_t s);
// leaves[b][4] into level 0 at idx[b], then the levels above; idx (device):
// k >= 1 voter indices < lv.len[0], ascending, no index twice (the caller checks)
void registry_replace(uint64_t *dig, const RegistryLevels &lv, const uint64_t *idx, const uint64_t *leaves, uint32_t k,
                      hipStream_t s);

}  // namespace qpk
