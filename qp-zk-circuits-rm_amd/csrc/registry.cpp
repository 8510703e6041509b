// registry.cpp — the qp_registry_* entry points (qpgpu.h): the electorate's
// Merkle tree built once on the device (registry.hip), paths by voter index.
#include "../../include/qpgpu.h"
#include <string.h>
#include <algorithm>
#include <memory>
#include <new>
#include <string>
#include <vector>
#include "field.h"
#include "registry.h"

namespace {
// voters per k_registry_paths launch (the batch buffers hold this many paths: 8 MB of siblings)
constexpr uint32_t REG_BATCH = 8192;
// the build's four timing events, destroyed on every return path
struct Events {
  hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
  ~Events() {
    for (hipEvent_t x : e)
      if (x) (void)hipEventDestroy(x);
  }
};
}  // namespace

int registry_paths_host(qp_registry *r, const uint64_t *idx, uint32_t nidx, uint64_t *siblings, uint32_t *path_bits,
                        uint32_t *depth, uint64_t *leaves) {
  qp_ctx *c = r->ctx;
  for (uint32_t b = 0; b < nidx; b++)
    if (idx[b] >= r->n) {
      c->err = "registry: voter index " + std::to_string(idx[b]) + " (position " + std::to_string(b) +
               ") is outside the " + std::to_string(r->n) + " voters";
      return QP_ERR_ARG;
    }
  QP_HIP_TRY(c, hipSetDevice(c->device));
  if (!r->d_idx.p) {
    QP_HIP_TRY(c, r->d_idx.alloc(REG_BATCH));
    QP_HIP_TRY(c, r->d_sib.alloc((size_t)REG_BATCH * qpk::REG_PATH_SLOTS * 4));
    QP_HIP_TRY(c, r->d_bits.alloc(REG_BATCH / 2));
    QP_HIP_TRY(c, r->d_depth.alloc(REG_BATCH / 2));
    QP_HIP_TRY(c, r->d_leaf.alloc((size_t)REG_BATCH * 4));
  }
  hipStream_t s = c->stream;
  for (uint32_t done = 0; done < nidx;) {
    const uint32_t nb = std::min(REG_BATCH, nidx - done);
    QP_HIP_TRY(c, hipMemcpyAsync(r->d_idx.p, idx + done, (size_t)nb * 8, hipMemcpyHostToDevice, s));
    qpk::registry_paths(r->dig.p, r->lv, r->d_idx.p, nb, r->d_sib.p, r->d_bits.as<uint32_t>(),
                        r->d_depth.as<uint32_t>(), leaves ? r->d_leaf.p : nullptr, s);
    QP_HIP_TRY(c, hipGetLastError());
    QP_HIP_TRY(c, hipMemcpyAsync(siblings + (size_t)done * qpk::REG_PATH_SLOTS * 4, r->d_sib.p,
                                 (size_t)nb * qpk::REG_PATH_SLOTS * 32, hipMemcpyDeviceToHost, s));
    QP_HIP_TRY(c, hipMemcpyAsync(path_bits + done, r->d_bits.p, (size_t)nb * 4, hipMemcpyDeviceToHost, s));
    QP_HIP_TRY(c, hipMemcpyAsync(depth + done, r->d_depth.p, (size_t)nb * 4, hipMemcpyDeviceToHost, s));
    if (leaves)
      QP_HIP_TRY(c, hipMemcpyAsync(leaves + (size_t)done * 4, r->d_leaf.p, (size_t)nb * 32, hipMemcpyDeviceToHost, s));
    QP_HIP_TRY(c, hipStreamSynchronize(s));
    done += nb;
  }
  return QP_OK;
}

extern "C" {

int qp_registry_new(qp_ctx *c, const uint64_t *keys, uint64_t n, qp_registry **out) {
  if (!c || !out) return QP_ERR_ARG;
  *out = nullptr;
  if (!keys || !n) {
    c->err = "qp_registry_new: no voters";
    return QP_ERR_ARG;
  }
  qpk::RegistryLevels lv;
  if (!qpk::registry_levels(n, lv)) {
    c->err = "qp_registry_new: " + std::to_string(n) + " voters need a Merkle path deeper than " +
             std::to_string(qpk::REG_MAX_DEPTH) + ", the most the voting circuit's depth split holds";
    return QP_ERR_ARG;
  }
  std::unique_ptr<qp_registry> r(new (std::nothrow) qp_registry);
  if (!r) return QP_ERR_OOM;
  r->ctx = c;
  r->n = n;
  r->lv = lv;
  std::vector<uint64_t> km;  // key-major [4][n]: the layout k_registry_leaves reads
  try {
    r->keys.assign(keys, keys + 4 * n);
    km.resize(4 * n);
  } catch (const std::bad_alloc &) {
    c->err = "qp_registry_new: host allocation failed";
    return QP_ERR_OOM;
  }
  for (uint64_t i = 0; i < n; i++)
    for (uint32_t k = 0; k < 4; k++) {
      const uint64_t v = keys[4 * i + k];
      if (v >= gl::P) {
        c->err = "qp_registry_new: key " + std::to_string(i) + " felt " + std::to_string(k) +
                 " is not a canonical field element";
        return QP_ERR_ARG;
      }
      km[k * n + i] = v;
    }
  QP_HIP_TRY(c, hipSetDevice(c->device));
  DevBuf dkeys;
  QP_HIP_TRY(c, dkeys.alloc(4 * n));
  QP_HIP_TRY(c, r->dig.alloc(lv.total() * 4));
  hipStream_t s = c->stream;
  Events ev;
  for (hipEvent_t &e : ev.e) QP_HIP_TRY(c, hipEventCreate(&e));
  QP_HIP_TRY(c, hipEventRecord(ev.e[0], s));
  QP_HIP_TRY(c, hipMemcpyAsync(dkeys.p, km.data(), 4 * n * 8, hipMemcpyHostToDevice, s));
  QP_HIP_TRY(c, hipEventRecord(ev.e[1], s));
  qpk::registry_leaves(dkeys.p, n, r->dig.p, s);
  QP_HIP_TRY(c, hipGetLastError());
  QP_HIP_TRY(c, hipEventRecord(ev.e[2], s));
  qpk::registry_tree(r->dig.p, lv, s);
  QP_HIP_TRY(c, hipGetLastError());
  QP_HIP_TRY(c, hipEventRecord(ev.e[3], s));
  QP_HIP_TRY(c, hipMemcpyAsync(r->root, r->dig.p + lv.off[lv.nlevels - 1] * 4, 32, hipMemcpyDeviceToHost, s));
  QP_HIP_TRY(c, hipStreamSynchronize(s));
  for (int k = 0; k < 3; k++) QP_HIP_TRY(c, hipEventElapsedTime(&r->build_ms[k], ev.e[k], ev.e[k + 1]));
  *out = r.release();
  return QP_OK;
}

void qp_registry_free(qp_registry *r) {
  if (!r) return;
  (void)hipSetDevice(r->ctx->device);
  delete r;
}

int qp_registry_root(const qp_registry *r, uint64_t out[4]) {
  if (!r || !out) return QP_ERR_ARG;
  memcpy(out, r->root, 32);
  return QP_OK;
}

int qp_registry_size(const qp_registry *r, uint64_t *n, uint32_t *max_depth) {
  if (!r) return QP_ERR_ARG;
  if (n) *n = r->n;
  if (max_depth) *max_depth = r->lv.max_depth();
  return QP_OK;
}

int qp_registry_paths(qp_registry *r, const uint64_t *idx, uint32_t nidx, uint64_t *siblings, uint32_t *path_bits,
                      uint32_t *depth) {
  if (!r) return QP_ERR_ARG;
  if (!nidx) return QP_OK;
  if (!idx || !siblings || !path_bits || !depth) {
    r->ctx->err = "qp_registry_paths: null buffer";
    return QP_ERR_ARG;
  }
  return registry_paths_host(r, idx, nidx, siblings, path_bits, depth, nullptr);
}

int qp_registry_build_times(const qp_registry *r, double ms[3]) {
  if (!r || !ms) return QP_ERR_ARG;
  for (int k = 0; k < 3; k++) ms[k] = r->build_ms[k];
  return QP_OK;
}

int qp_registry_level(qp_registry *r, uint32_t level, uint64_t *out, uint64_t *len) {
  if (!r) return QP_ERR_ARG;
  if (level >= r->lv.nlevels) {
    r->ctx->err = "qp_registry_level: the tree has " + std::to_string(r->lv.nlevels) + " levels";
    return QP_ERR_ARG;
  }
  if (len) *len = r->lv.len[level];
  if (!out) return QP_OK;
  qp_ctx *c = r->ctx;
  QP_HIP_TRY(c, hipSetDevice(c->device));
  QP_HIP_TRY(c, hipMemcpyAsync(out, r->dig.p + r->lv.off[level] * 4, r->lv.len[level] * 32, hipMemcpyDeviceToHost,
                               c->stream));
  QP_HIP_TRY(c, hipStreamSynchronize(c->stream));
  return QP_OK;
}

}  // extern "C"
