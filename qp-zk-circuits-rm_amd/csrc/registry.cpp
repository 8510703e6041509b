// registry.cpp — the qp_registry_* entry points (qpgpu.h): the electorate's
// Merkle tree built and kept on the device (an AccTree, acc_tree.h; its leaves
// by registry.hip or uploaded), paths by voter index.
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
// a felt >= p among leaves[k][4]; the voter named is idx[its position], or first + its position
int check_commitments(qp_ctx *c, const char *fn, const uint64_t *leaves, uint64_t k, uint64_t first,
                      const uint64_t *idx = nullptr) {
  for (uint64_t i = 0; i < k; i++)
    for (uint32_t f = 0; f < 4; f++)
      if (leaves[4 * i + f] >= gl::P) {
        c->err = std::string(fn) + ": commitment " + std::to_string(idx ? idx[i] : first + i) + " (position " +
                 std::to_string(i) + " of the batch) felt " + std::to_string(f) + " is not a canonical field element";
        return QP_ERR_ARG;
      }
  return QP_OK;
}

int not_for_keyed(const qp_registry *r, const char *fn) {
  r->ctx->err = std::string(fn) + ": the registry was built from private keys (qp_registry_new) and keeps a host " +
                "copy of them, which an update would leave stale; use qp_registry_new_commitments";
  return QP_ERR_STATE;
}

// the first step of an update on the context's stream: the device, the timing events, the start mark
int update_begin(qp_registry *r) {
  qp_ctx *c = r->ctx;
  QP_HIP_TRY(c, hipSetDevice(c->device));
  for (hipEvent_t &e : r->ev.e)
    if (!e) QP_HIP_TRY(c, hipEventCreate(&e));
  QP_HIP_TRY(c, hipEventRecord(r->ev.e[0], c->stream));
  return QP_OK;
}

// the last step: the launches' status, the new root, and only then the new size and table
int update_end(qp_registry *r, const qpk::AccLevels &lv, bool count) {
  qp_ctx *c = r->ctx;
  hipStream_t s = c->stream;
  uint64_t root[4];
  QP_HIP_TRY(c, hipGetLastError());
  QP_HIP_TRY(c, hipEventRecord(r->ev.e[2], s));
  QP_HIP_TRY(c, hipMemcpyAsync(root, r->tree.root(lv), 32, hipMemcpyDeviceToHost, s));
  QP_HIP_TRY(c, hipStreamSynchronize(s));
  QP_HIP_TRY(c, hipEventElapsedTime(&r->build_ms[0], r->ev.e[0], r->ev.e[1]));
  QP_HIP_TRY(c, hipEventElapsedTime(&r->build_ms[2], r->ev.e[1], r->ev.e[2]));
  r->build_ms[1] = 0;
  memcpy(r->root, root, 32);
  r->tree.lv = lv;
  if (count) r->epoch++;
  return QP_OK;
}

// voters [n, n + k) of a commitment registry (the caller checked the batch and the capacity)
int append_checked(qp_registry *r, const uint64_t *leaves, uint64_t k, bool count) {
  qp_ctx *c = r->ctx;
  qpk::AccLevels lv;
  if (!qpk::acc_levels_reserved(r->tree.n() + k, r->tree.capacity, lv)) return QP_ERR_ARG;
  if (int rc = update_begin(r)) return rc;
  hipStream_t s = c->stream;
  // straight into level 0: slots at or beyond len[0] are scratch until the size moves
  QP_HIP_TRY(c, hipMemcpyAsync(r->tree.dig.p + r->tree.n() * 4, leaves, k * 32, hipMemcpyHostToDevice, s));
  QP_HIP_TRY(c, hipEventRecord(r->ev.e[1], s));
  r->tree.append(lv, qpk::acc_row_max(), s);
  return update_end(r, lv, count);
}
}  // namespace

int registry_paths(qp_registry *r, const uint64_t *idx, uint32_t nidx, uint64_t *siblings, uint32_t *path_bits,
                   uint32_t *depth, uint64_t *leaves) {
  qp_ctx *c = r->ctx;
  for (uint32_t b = 0; b < nidx; b++)
    if (idx[b] >= r->tree.n()) {
      c->err = "registry: voter index " + std::to_string(idx[b]) + " (position " + std::to_string(b) +
               ") is outside the " + std::to_string(r->tree.n()) + " voters";
      return QP_ERR_ARG;
    }
  QP_HIP_TRY(c, hipSetDevice(c->device));
  return r->tree.paths({c->err}, c->stream, idx, nidx, siblings, path_bits, depth, leaves);
}

// what has no meaning before the first voter registers
static int empty_registry(const qp_registry *r, const char *fn) {
  r->ctx->err = std::string(fn) + ": the registry is empty (no voter has registered yet)";
  return QP_ERR_STATE;
}

extern "C" {

int qp_registry_new(qp_ctx *c, const uint64_t *keys, uint64_t n, qp_registry **out) {
  if (!c || !out) return QP_ERR_ARG;
  *out = nullptr;
  if (!keys || !n) {
    c->err = "qp_registry_new: no voters";
    return QP_ERR_ARG;
  }
  qpk::AccLevels lv;
  if (!qpk::acc_levels_reserved(n, n, lv)) {  // capacity == n: the dense table
    c->err = "qp_registry_new: " + std::to_string(n) + " voters need a Merkle path deeper than " +
             std::to_string(qpk::ACC_MAX_DEPTH) + ", the most the voting circuit's depth split holds";
    return QP_ERR_ARG;
  }
  std::unique_ptr<qp_registry> r(new (std::nothrow) qp_registry);
  if (!r) return QP_ERR_OOM;
  r->ctx = c;
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
  if (int rc = r->tree.alloc({c->err}, n)) return rc;
  hipStream_t s = c->stream;
  TimingEvents<4> ev;
  for (hipEvent_t &e : ev.e) QP_HIP_TRY(c, hipEventCreate(&e));
  QP_HIP_TRY(c, hipEventRecord(ev.e[0], s));
  QP_HIP_TRY(c, hipMemcpyAsync(dkeys.p, km.data(), 4 * n * 8, hipMemcpyHostToDevice, s));
  QP_HIP_TRY(c, hipEventRecord(ev.e[1], s));
  qpk::registry_leaves(dkeys.p, n, r->tree.dig.p, s);
  QP_HIP_TRY(c, hipGetLastError());
  QP_HIP_TRY(c, hipEventRecord(ev.e[2], s));
  // the whole tree, as an append to none, never in the row form (a launch per wide level, then k_acc_fold)
  r->tree.append(lv, 0, s);
  QP_HIP_TRY(c, hipGetLastError());
  QP_HIP_TRY(c, hipEventRecord(ev.e[3], s));
  QP_HIP_TRY(c, hipMemcpyAsync(r->root, r->tree.root(lv), 32, hipMemcpyDeviceToHost, s));
  QP_HIP_TRY(c, hipStreamSynchronize(s));
  for (int k = 0; k < 3; k++) QP_HIP_TRY(c, hipEventElapsedTime(&r->build_ms[k], ev.e[k], ev.e[k + 1]));
  r->tree.lv = lv;
  *out = r.release();
  return QP_OK;
}

int qp_registry_new_commitments(qp_ctx *c, const uint64_t *leaves, uint64_t n, uint64_t capacity, qp_registry **out) {
  if (!c || !out) return QP_ERR_ARG;
  *out = nullptr;
  if (n && !leaves) {
    c->err = "qp_registry_new_commitments: null leaves";
    return QP_ERR_ARG;
  }
  if (capacity > qpk::ACC_MAX_LEAVES || capacity < std::max<uint64_t>(n, 1)) {
    c->err = "qp_registry_new_commitments: capacity " + std::to_string(capacity) + " for " + std::to_string(n) +
             " voters: it must hold them (and at least one) and be at most 2^31, the most voters a path of depth " +
             std::to_string(qpk::ACC_MAX_DEPTH) + " reaches";
    return QP_ERR_ARG;
  }
  int rc = check_commitments(c, "qp_registry_new_commitments", leaves, n, 0);
  if (rc) return rc;
  std::unique_ptr<qp_registry> r(new (std::nothrow) qp_registry);
  if (!r) return QP_ERR_OOM;
  r->ctx = c;
  r->keyed = false;
  QP_HIP_TRY(c, hipSetDevice(c->device));
  if ((rc = r->tree.alloc({c->err}, capacity))) return rc;
  if (n && (rc = append_checked(r.get(), leaves, n, false))) return rc;
  *out = r.release();
  return QP_OK;
}

int qp_registry_append(qp_registry *r, const uint64_t *leaves, uint64_t k, uint64_t *first) {
  if (!r) return QP_ERR_ARG;
  if (r->keyed) return not_for_keyed(r, "qp_registry_append");
  if (first) *first = r->tree.n();
  if (!k) return QP_OK;
  qp_ctx *c = r->ctx;
  if (!leaves) {
    c->err = "qp_registry_append: null leaves";
    return QP_ERR_ARG;
  }
  if (k > r->tree.capacity - r->tree.n()) {
    c->err = "qp_registry_append: " + std::to_string(r->tree.n()) + " + " + std::to_string(k) +
             " voters exceed the capacity " + std::to_string(r->tree.capacity) + "; call qp_registry_reserve first";
    return QP_ERR_ARG;
  }
  int rc = check_commitments(c, "qp_registry_append", leaves, k, r->tree.n());
  if (rc) return rc;
  return append_checked(r, leaves, k, true);
}

int qp_registry_replace(qp_registry *r, const uint64_t *idx, const uint64_t *leaves, uint32_t k) {
  if (!r) return QP_ERR_ARG;
  if (r->keyed) return not_for_keyed(r, "qp_registry_replace");
  if (!k) return QP_OK;
  qp_ctx *c = r->ctx;
  if (!idx || !leaves) {
    c->err = "qp_registry_replace: null buffer";
    return QP_ERR_ARG;
  }
  std::vector<uint32_t> order;
  std::vector<uint64_t> sidx, sleaf;
  try {
    uint32_t bad = 0;
    if (!qpk::registry_replace_order(idx, k, r->tree.n(), order, &bad)) {
      c->err = "qp_registry_replace: voter index " + std::to_string(idx[bad]) + " (position " + std::to_string(bad) +
               (idx[bad] >= r->tree.n() ? ") is outside the " + std::to_string(r->tree.n()) + " voters"
                                 : ") appears twice in the batch");
      return QP_ERR_ARG;
    }
    sidx.resize(k);
    sleaf.resize((size_t)k * 4);
  } catch (const std::bad_alloc &) {
    c->err = "qp_registry_replace: host allocation failed";
    return QP_ERR_OOM;
  }
  int rc = check_commitments(c, "qp_registry_replace", leaves, k, 0, idx);
  if (rc) return rc;
  for (uint32_t b = 0; b < k; b++) {
    sidx[b] = idx[order[b]];
    memcpy(&sleaf[(size_t)b * 4], leaves + (size_t)order[b] * 4, 32);
  }
  if ((rc = update_begin(r))) return rc;
  if (r->d_upd_idx.words < k) {
    QP_HIP_TRY(c, r->d_upd_idx.alloc(k));
    QP_HIP_TRY(c, r->d_upd_leaf.alloc((size_t)k * 4));
  }
  hipStream_t s = c->stream;
  QP_HIP_TRY(c, hipMemcpyAsync(r->d_upd_idx.p, sidx.data(), (size_t)k * 8, hipMemcpyHostToDevice, s));
  QP_HIP_TRY(c, hipMemcpyAsync(r->d_upd_leaf.p, sleaf.data(), (size_t)k * 32, hipMemcpyHostToDevice, s));
  QP_HIP_TRY(c, hipEventRecord(r->ev.e[1], s));
  r->tree.replace(r->d_upd_idx.p, r->d_upd_leaf.p, k, qpk::acc_row_max(), s);
  return update_end(r, r->tree.lv, true);
}

int qp_registry_reserve(qp_registry *r, uint64_t new_capacity) {
  if (!r) return QP_ERR_ARG;
  if (r->keyed) return not_for_keyed(r, "qp_registry_reserve");
  qp_ctx *c = r->ctx;
  qpk::AccLevels lv;
  if (!qpk::acc_levels_reserved(r->tree.n(), new_capacity, lv)) {
    c->err = "qp_registry_reserve: capacity " + std::to_string(new_capacity) + " for " + std::to_string(r->tree.n()) +
             " voters: it must hold them (and at least one) and be at most 2^31";
    return QP_ERR_ARG;
  }
  if (new_capacity == r->tree.capacity) return QP_OK;
  QP_HIP_TRY(c, hipSetDevice(c->device));
  if (int rc = r->tree.reserve({c->err}, new_capacity, lv, c->stream)) return rc;
  r->epoch++;
  return QP_OK;
}

int qp_registry_state(const qp_registry *r, uint64_t *capacity, uint64_t *epoch) {
  if (!r) return QP_ERR_ARG;
  if (capacity) *capacity = r->tree.capacity;
  if (epoch) *epoch = r->epoch;
  return QP_OK;
}

void qp_registry_free(qp_registry *r) {
  if (!r) return;
  (void)hipSetDevice(r->ctx->device);
  delete r;
}

int qp_registry_root(const qp_registry *r, uint64_t out[4]) {
  if (!r || !out) return QP_ERR_ARG;
  if (!r->tree.n()) return empty_registry(r, "qp_registry_root");
  memcpy(out, r->root, 32);
  return QP_OK;
}

int qp_registry_size(const qp_registry *r, uint64_t *n, uint32_t *max_depth) {
  if (!r) return QP_ERR_ARG;
  if (n) *n = r->tree.n();
  if (max_depth) *max_depth = r->tree.lv.max_depth();
  return QP_OK;
}

int qp_registry_paths(qp_registry *r, const uint64_t *idx, uint32_t nidx, uint64_t *siblings, uint32_t *path_bits,
                      uint32_t *depth) {
  if (!r) return QP_ERR_ARG;
  if (!r->tree.n()) return empty_registry(r, "qp_registry_paths");
  if (!nidx) return QP_OK;
  if (!idx || !siblings || !path_bits || !depth) {
    r->ctx->err = "qp_registry_paths: null buffer";
    return QP_ERR_ARG;
  }
  return registry_paths(r, idx, nidx, siblings, path_bits, depth, nullptr);
}

int qp_registry_build_times(const qp_registry *r, double ms[3]) {
  if (!r || !ms) return QP_ERR_ARG;
  for (int k = 0; k < 3; k++) ms[k] = r->build_ms[k];
  return QP_OK;
}

int qp_registry_level(qp_registry *r, uint32_t level, uint64_t *out, uint64_t *len) {
  if (!r) return QP_ERR_ARG;
  if (!r->tree.n()) return empty_registry(r, "qp_registry_level");
  const qpk::AccLevels &lv = r->tree.lv;
  if (level >= lv.nlevels) {
    r->ctx->err = "qp_registry_level: the tree has " + std::to_string(lv.nlevels) + " levels";
    return QP_ERR_ARG;
  }
  if (len) *len = lv.len[level];
  if (!out) return QP_OK;
  qp_ctx *c = r->ctx;
  QP_HIP_TRY(c, hipSetDevice(c->device));
  const uint64_t *src = r->tree.dig.p + lv.off[level] * 4;
  QP_HIP_TRY(c, hipMemcpyAsync(out, src, lv.len[level] * 32, hipMemcpyDeviceToHost, c->stream));
  QP_HIP_TRY(c, hipStreamSynchronize(c->stream));
  return QP_OK;
}

}  // extern "C"
