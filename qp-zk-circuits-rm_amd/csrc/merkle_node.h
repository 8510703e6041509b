// merkle_node.h — the node hash every device Merkle tree shares: the prover's
// power-of-two trees (merkle.hip) and the promoted-odd-node accumulator trees of the voter registry and
// the ballot log (acc_tree.hip; their leaves in registry.hip and ballot.hip).
#pragma once
#include <stdint.h>
#include "poseidon_dev.h"

namespace qpk {

// PoseidonHash::hash_no_pad of the at most 8 felts in s[0..7] (two_to_one of
// two digests; a 4-felt leaf with s[4..7] = 0): one capacity-zero
// permutation.  s[0..3] leave as the canonical digest; the other lanes are
// not defined.
__device__ __forceinline__ void node_digest(uint64_t s[12]) {
  s[8] = s[9] = s[10] = s[11] = 0;
  psd::permute_nc_node(s);
#pragma unroll
  for (int j = 0; j < 4; j++) s[j] = psd::canon(s[j]);
}

}  // namespace qpk
