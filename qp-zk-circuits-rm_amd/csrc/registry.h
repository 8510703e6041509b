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
  DevBuf dig;                  // [level][node][4], lv.total() digests
  std::vector<uint64_t> keys;  // host, [n][4]: prove_voters fills the private key from it
  uint64_t root[4] = {0};
  float build_ms[3] = {0};  // HIP-event times of the build: key upload, k_registry_leaves, the levels
  // one batch of paths (REG_BATCH voters at most per launch)
  DevBuf d_idx, d_sib, d_bits, d_depth, d_leaf;
};

// the paths (and, leaves != null, the leaf digests [nidx][4]) of voters idx[]
// into host buffers laid out as k_registry_paths writes them; an index >= n is
// QP_ERR_ARG before anything is launched
int registry_paths_host(qp_registry *r, const uint64_t *idx, uint32_t nidx, uint64_t *siblings, uint32_t *path_bits,
                        uint32_t *depth, uint64_t *leaves);
