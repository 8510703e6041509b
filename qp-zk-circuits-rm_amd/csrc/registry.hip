// registry.hip — level 0 of the voter registry's eligibility tree (gfx950):
// leaf = hash_no_pad(key), the reference's (voting/src/lib.rs:285-316).  The
// levels above and the paths are the accumulator tree's (acc_tree.hip).
// VALU-bound like merkle.hip: one lane per leaf, one capacity-zero
// permutation each (merkle_node.h), the state in registers.
#include "registry.h"
#include "merkle_node.h"

namespace qpk {

// leaf i = hash_no_pad(key i): the four felts of a key are four coalesced
// column loads (64 lanes x 8 B = 512 contiguous bytes each)
__global__ void __launch_bounds__(256) k_registry_leaves(const uint64_t *__restrict__ keys, uint64_t n,
                                                         uint64_t *__restrict__ dig) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t s[12];
#pragma unroll
  for (int k = 0; k < 4; k++) s[k] = keys[(uint64_t)k * n + i];
  s[4] = s[5] = s[6] = s[7] = 0;
  node_digest(s);
  uint64_t *o = dig + i * 4;
#pragma unroll
  for (int k = 0; k < 4; k++) o[k] = s[k];
}

void registry_leaves(const uint64_t *keys, uint64_t n, uint64_t *dig, hipStream_t s) {
  k_registry_leaves<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(keys, n, dig);
}

}  // namespace qpk
