// acc_tree.cpp — AccTree (acc_tree.h): allocation, the batched path download, the re-lay of a reserve, an audit's batch of prefix roots.
#include "acc_tree.h"
#include <string.h>
#include <algorithm>
#include "../../include/qpgpu.h"

int AccTree::alloc(AccErr e, uint64_t cap) {
  QP_HIP_TRY(&e, dig.alloc((size_t)qpk::acc_reserved(cap) * 4));
  capacity = cap;
  qpk::acc_levels_reserved(0, cap, lv);
  return QP_OK;
}

int AccTree::paths(AccErr e, hipStream_t s, const uint64_t *idx, uint32_t nidx, uint64_t *siblings,
                   uint32_t *path_bits, uint32_t *depth, uint64_t *leaves) {
  if (!d_idx.p) {
    QP_HIP_TRY(&e, d_idx.alloc(ACC_BATCH));
    QP_HIP_TRY(&e, d_sib.alloc((size_t)ACC_BATCH * qpk::ACC_PATH_SLOTS * 4));
    QP_HIP_TRY(&e, d_bits.alloc(ACC_BATCH / 2));
    QP_HIP_TRY(&e, d_depth.alloc(ACC_BATCH / 2));
    QP_HIP_TRY(&e, d_leaf.alloc((size_t)ACC_BATCH * 4));
  }
  for (uint32_t done = 0; done < nidx;) {
    const uint32_t nb = std::min(ACC_BATCH, nidx - done);
    QP_HIP_TRY(&e, hipMemcpyAsync(d_idx.p, idx + done, (size_t)nb * 8, hipMemcpyHostToDevice, s));
    qpk::acc_paths(dig.p, lv, d_idx.p, nb, d_sib.p, d_bits.as<uint32_t>(), d_depth.as<uint32_t>(),
                   leaves ? d_leaf.p : nullptr, s);
    QP_HIP_TRY(&e, hipGetLastError());
    QP_HIP_TRY(&e, hipMemcpyAsync(siblings + (size_t)done * qpk::ACC_PATH_SLOTS * 4, d_sib.p,
                                  (size_t)nb * qpk::ACC_PATH_SLOTS * 32, hipMemcpyDeviceToHost, s));
    QP_HIP_TRY(&e, hipMemcpyAsync(path_bits + done, d_bits.p, (size_t)nb * 4, hipMemcpyDeviceToHost, s));
    QP_HIP_TRY(&e, hipMemcpyAsync(depth + done, d_depth.p, (size_t)nb * 4, hipMemcpyDeviceToHost, s));
    if (leaves)
      QP_HIP_TRY(&e, hipMemcpyAsync(leaves + (size_t)done * 4, d_leaf.p, (size_t)nb * 32, hipMemcpyDeviceToHost, s));
    QP_HIP_TRY(&e, hipStreamSynchronize(s));
    done += nb;
  }
  return QP_OK;
}

int AccTree::prefix_roots(AccErr e, hipStream_t s, const uint64_t *ms, uint32_t k, uint64_t *roots_out) {
  if (k && d_m.words < ACC_BATCH) {
    QP_HIP_TRY(&e, d_m.alloc(ACC_BATCH));
    QP_HIP_TRY(&e, d_roots.alloc((size_t)ACC_BATCH * 4));
  }
  for (uint32_t done = 0; done < k;) {
    const uint32_t nb = std::min(ACC_BATCH, k - done);
    QP_HIP_TRY(&e, hipMemcpyAsync(d_m.p, ms + done, (size_t)nb * 8, hipMemcpyHostToDevice, s));
    qpk::acc_prefix_roots(dig.p, lv, d_m.p, nb, d_roots.p, s);
    QP_HIP_TRY(&e, hipGetLastError());
    QP_HIP_TRY(&e, hipMemcpyAsync(roots_out + (size_t)done * 4, d_roots.p, (size_t)nb * 32, hipMemcpyDeviceToHost, s));
    QP_HIP_TRY(&e, hipStreamSynchronize(s));
    done += nb;
  }
  return QP_OK;
}

int AccTree::reserve(AccErr e, uint64_t new_capacity, const qpk::AccLevels &nlv, hipStream_t s) {
  DevBuf nd;
  QP_HIP_TRY(&e, nd.alloc((size_t)qpk::acc_reserved(new_capacity) * 4));
  for (uint32_t l = 0; l < nlv.nlevels; l++)
    QP_HIP_TRY(&e, hipMemcpyAsync(nd.p + nlv.off[l] * 4, dig.p + lv.off[l] * 4, nlv.len[l] * 32,
                                  hipMemcpyDeviceToDevice, s));
  QP_HIP_TRY(&e, hipStreamSynchronize(s));
  dig = std::move(nd);
  lv = nlv;
  capacity = new_capacity;
  return QP_OK;
}

void PrefixRootBatch::get(uint32_t i, uint64_t out[4]) {
  if (!asked) {
    asked = true;
    at.assign(k, 0);
    for (uint32_t j = 0; j < k; j++)
      if (ns[j] <= n) {
        at[j] = (uint32_t)ms.size();
        ms.push_back(ns[j]);
      }
    got.assign(ms.size() * 4, 0);
    rc = tree.prefix_roots(e, s, ms.data(), (uint32_t)ms.size(), got.data());
  }
  memcpy(out, &got[(size_t)at[i] * 4], 32);
}
