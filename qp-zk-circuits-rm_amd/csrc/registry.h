// registry.h — the voter registry behind the qp_registry handle (qpgpu.h): an accumulator tree (acc_tree.h)
// whose leaf is hash_no_pad(4-felt key), written by k_registry_leaves (registry.hip) or uploaded as a commitment.
#pragma once
#include <stdint.h>
#include <vector>
#include "acc_tree.h"

namespace qpk {
__global__ void k_registry_leaves(const uint64_t *keys, uint64_t n, uint64_t *dig);
// leaf digests: keys key-major [4][n] (felt k of voter i at keys[k n + i]) -> dig[i][4]
void registry_leaves(const uint64_t *keys, uint64_t n, uint64_t *dig, hipStream_t s);
}  // namespace qpk

struct qp_registry {
  qp_ctx *ctx = nullptr;
  AccTree tree;                // the eligibility tree: tree.n() voters in a layout for tree.capacity (keyed: the same)
  std::vector<uint64_t> keys;  // host, [n][4]: prove_voters fills the private key from it (keyed registries only)
  uint64_t root[4] = {0};
  float build_ms[3] = {0};  // HIP-event times of the build: key upload, k_registry_leaves, the levels
  // ---- a commitment registry (qp_registry_new_commitments): no keys, a layout for more leaves than voters
  bool keyed = true;
  uint64_t epoch = 0;            // completed append / replace / reserve calls
  DevBuf d_upd_idx, d_upd_leaf;  // a replace batch: sorted indices [k], their leaves [k][4]; grown on demand
  TimingEvents<3> ev;            // upload start, upload end, levels end of an update
};

// the paths (and, leaves != null, the leaf digests [nidx][4]) of voters idx[]
// into host buffers laid out as k_acc_paths writes them; an index >= n is
// QP_ERR_ARG before anything is launched
int registry_paths(qp_registry *r, const uint64_t *idx, uint32_t nidx, uint64_t *siblings, uint32_t *path_bits,
                   uint32_t *depth, uint64_t *leaves);
