// acc_kernels.h — argument layouts and launchers of acc_tree.hip: the levels
// and the Merkle paths of an accumulator tree, the tree of the voter registry
// (the reference's, voting/src/lib.rs:285-316, with the paths the voting
// circuit walks, :123-180) and of the ballot box's log.  One launcher per step;
// the launcher owns the kernel choice and the grid, block and LDS sizes.
//
// Tree convention: node = hash_no_pad(left || right), and the last node of an
// odd-length level moves to the next level unchanged.  Level l holds
// ceil(N / 2^l) nodes; every level stays resident, [level][node][4] felts, in
// a reserved layout (acc_layout.h: off[] from the capacity, len[] / nlevels
// from N).  Level 0 is the owner's: a leaf kernel or an upload writes it first.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "acc_layout.h"
#include "paths.h"

namespace qpk {

__global__ void k_acc_level(const uint64_t *src, uint64_t nsrc, uint64_t *dst);
__global__ void k_acc_fold(uint64_t *dig, AccLevels lv, uint32_t l0);
__global__ void k_acc_paths(const uint64_t *dig, AccLevels lv, const uint64_t *idx, uint32_t nidx, uint64_t *siblings,
                            uint32_t *path_bits, uint32_t *depth, uint64_t *leaves);

// the paths of leaves idx[b] < n (the caller checks the bound): siblings
// [nidx][ACC_PATH_SLOTS][4] compacted to the levels where the leaf's node was
// hashed (the zero digest above the depth), path_bits[b] bit j = side of
// sibling j (1: the leaf's node is the right child), depth[b] = siblings;
// leaves (may be null) [nidx][4] = the leaf digests
void acc_paths(const uint64_t *dig, const AccLevels &lv, const uint64_t *idx, uint32_t nidx, uint64_t *siblings,
               uint32_t *path_bits, uint32_t *depth, uint64_t *leaves, hipStream_t s);

__global__ void k_acc_prefix_roots(const uint64_t *dig, AccLevels lv, const uint64_t *m, uint32_t k, uint64_t *roots);

// roots[i][4] = the root the tree had when it held leaves [0, m[i]) (m device, each in 1..n: the
// caller checks the bound), by acc_layout.h's HostTree::prefix_root fold.  Read-only; after the
// append that made `lv`, on the same stream.
void acc_prefix_roots(const uint64_t *dig, const AccLevels &lv, const uint64_t *m, uint32_t k, uint64_t *roots,
                      hipStream_t s);

// ---- the levels above level 0.  Each launcher recomputes the nodes that a
// change of level 0 changes, level by level in launch order, every loop bound
// from the host's table.
// Dirty ranges narrower than row_max run in the row form (16 lanes per node,
// pc::permute_row) at every level up to the root: measured against the
// one-lane form it wins or ties at every range width up to ACC_ROW_MAX, the
// widest measured (DESIGN §12 has the A/B).  Wider ranges go through
// k_acc_level on the level's suffix and, from a level of at most ACC_FOLD_MAX
// nodes, k_acc_fold.  row_max = 0: never the row form, which for n_old = 0 is
// one launch per level wider than ACC_FOLD_MAX, then the rest in one workgroup.
constexpr long ACC_ROW_MAX = 32768;
// the row bound of an update: ACC_ROW_MAX unless the path hook registry_row=N
// overrides it (read per call)
inline uint64_t acc_row_max() { return (uint64_t)path_opt("registry_row", ACC_ROW_MAX); }

__global__ void k_acc_range_row(uint64_t *dig, AccLevels lv, uint32_t level, uint64_t first, uint32_t count);
__global__ void k_acc_put(uint64_t *dig, const uint64_t *idx, const uint64_t *leaves, uint32_t k);
__global__ void k_acc_scatter(uint64_t *dig, AccLevels lv, uint32_t level, const uint64_t *idx, uint32_t k);
__global__ void k_acc_scatter_row(uint64_t *dig, AccLevels lv, uint32_t level, const uint64_t *idx, uint32_t k);

// the levels above the leaves after leaves [n_old, lv.len[0]) were written into
// level 0 (lv: the table of the new size); n_old = 0 builds the whole tree
void acc_append(uint64_t *dig, const AccLevels &lv, uint64_t n_old, uint64_t row_max, hipStream_t s);
// leaves[b][4] into level 0 at idx[b], then the levels above; idx (device):
// k >= 1 leaf indices < lv.len[0], ascending, no index twice (the caller checks)
void acc_replace(uint64_t *dig, const AccLevels &lv, const uint64_t *idx, const uint64_t *leaves, uint32_t k,
                 uint64_t row_max, hipStream_t s);

}  // namespace qpk
