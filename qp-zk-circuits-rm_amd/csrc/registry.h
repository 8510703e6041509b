// registry.h — the voter registry behind the qp_registry handle (qpgpu.h).
#pragma once
#include <stdint.h>
#include <vector>
#include "ctx.h"
#include "registry_kernels.h"

struct qp_registry {
  qp_ctx *ctx = nullptr;
  uint64_t n = 0;
  qpk::RegistryLevels lv;
  DevBuf dig;                  // [level][node][4]: lv.total() digests (keyed), registry_reserved(capacity) (commitments)
  std::vector<uint64_t> keys;  // host, [n][4]: prove_voters fills the private key from it (keyed registries only)
  uint64_t root[4] = {0};
  float build_ms[3] = {0};  // HIP-event times of the build: key upload, k_registry_leaves, the levels
  // one batch of paths (REG_BATCH voters at most per launch)
  DevBuf d_idx, d_sib, d_bits, d_depth, d_leaf;
  // ---- a commitment registry (qp_registry_new_commitments): no keys, a layout for `capacity` leaves
  bool keyed = true;
  uint64_t capacity = 0;  // keyed: n
  uint64_t epoch = 0;     // completed append / replace / reserve calls
  DevBuf d_upd_idx, d_upd_leaf;  // a replace batch: sorted indices [k], their leaves [k][4]; grown on demand
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};  // upload start, upload end, levels end of an update
  ~qp_registry() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

// the paths (and, leaves != null, the leaf digests [nidx][4]) of voters idx[]
// into host buffers laid out as k_registry_paths writes them; an index >= n is
// QP_ERR_ARG before anything is launched
int registry_paths_host(qp_registry *r, const uint64_t *idx, uint32_t nidx, uint64_t *siblings, uint32_t *path_bits,
                        uint32_t *depth, uint64_t *leaves);
