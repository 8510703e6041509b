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

namespace qpk {

// the circuit has MAX_MERKLE_DEPTH = 32 sibling slots and a 5-bit depth split:
// the deepest path a registry may hold is 31 (N <= 2^31)
constexpr uint32_t REG_PATH_SLOTS = 32, REG_MAX_DEPTH = 31, REG_MAX_LEVELS = REG_MAX_DEPTH + 1;
// from a level of at most this many nodes up, the rest of the tree is one launch
constexpr uint32_t REG_FOLD_MAX = 64;

// level offsets (in digests) and lengths, leaves first; the root is level nlevels - 1
struct RegistryLevels {
  uint32_t nlevels = 0;
  uint64_t off[REG_MAX_LEVELS] = {0}, len[REG_MAX_LEVELS] = {0};
  uint64_t total() const { return nlevels ? off[nlevels - 1] + len[nlevels - 1] : 0; }
  uint32_t max_depth() const { return nlevels - 1; }
};
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

}  // namespace qpk
