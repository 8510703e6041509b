// acc_tree.hip — the levels and the Merkle paths of an accumulator tree
// (gfx950; acc_kernels.h has the convention); a path is the siblings of the
// levels where the leaf's node was hashed, compacted, with one side bit each.
// VALU-bound like merkle.hip: one lane per parent, one capacity-zero
// permutation each (merkle_node.h), the state in registers.
#include "acc_kernels.h"
#include "merkle_node.h"
#include "poseidon_coop.h"

namespace qpk {

// one wide level: lane t hashes nodes 2t, 2t+1 of src into node t of dst.  The
// lone last node of an odd src is copied by lane 0 once its own hash is
// stored (a branch around the permutation for that one lane cost every lane
// registers: 84 and 108 VGPRs in two forms against this form's count)
__global__ void __launch_bounds__(256) k_acc_level(const uint64_t *__restrict__ src, uint64_t nsrc,
                                                   uint64_t *__restrict__ dst) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t npair = nsrc / 2;
  if (t >= npair) return;
  const uint64_t *c = src + t * 8;
  uint64_t s[12];
#pragma unroll
  for (int j = 0; j < 8; j++) s[j] = c[j];
  node_digest(s);
  uint64_t *o = dst + t * 4;
#pragma unroll
  for (int j = 0; j < 4; j++) o[j] = s[j];
  if (t == 0 && (nsrc & 1)) {
#pragma unroll
    for (int j = 0; j < 4; j++) dst[npair * 4 + j] = src[(nsrc - 1) * 4 + j];
  }
}

// every level above level l0 (at most ACC_FOLD_MAX nodes) in one wave: the
// nodes fold through LDS level by level, every level written out
__global__ void __launch_bounds__(ACC_FOLD_MAX) k_acc_fold(uint64_t *__restrict__ dig, AccLevels lv, uint32_t l0) {
  __shared__ uint64_t sh[ACC_FOLD_MAX * 4];
  const uint32_t t = threadIdx.x;
  if (t < lv.len[l0]) {
    const uint64_t *c = dig + (lv.off[l0] + t) * 4;
#pragma unroll
    for (int j = 0; j < 4; j++) sh[t * 4 + j] = c[j];
  }
  __syncthreads();
  for (uint32_t l = l0 + 1; l < lv.nlevels; l++) {
    const uint32_t nsrc = (uint32_t)lv.len[l - 1], ndst = (uint32_t)lv.len[l];
    uint64_t s[12];
    if (t < ndst) {
#pragma unroll
      for (int j = 0; j < 4; j++) s[j] = sh[t * 8 + j];
      if (2 * t + 1 < nsrc) {
#pragma unroll
        for (int j = 4; j < 8; j++) s[j] = sh[t * 8 + j];
        node_digest(s);
      }
      uint64_t *o = dig + (lv.off[l] + t) * 4;
#pragma unroll
      for (int j = 0; j < 4; j++) o[j] = s[j];
    }
    __syncthreads();
    if (t < ndst) {
#pragma unroll
      for (int j = 0; j < 4; j++) sh[t * 4 + j] = s[j];
    }
    __syncthreads();
  }
}

// one lane per (leaf of the batch, level): 32 lanes per leaf, two leaves per
// wave.  Lane l marks whether the leaf's node at level l was hashed (it has a
// sibling) or promoted (the shape rule, acc_layout.h's path_levels); the
// leaf's half of the wave ballot is its level mask, so the slot of lane l's
// sibling is the count of hashed levels below l.
// Every one of the leaf's 32 sibling slots is written exactly once: slots
// below the depth by the hashed lanes, slot l >= depth (zero digest) by lane l.
__global__ void __launch_bounds__(256) k_acc_paths(const uint64_t *__restrict__ dig, AccLevels lv,
                                                   const uint64_t *__restrict__ idx, uint32_t nidx,
                                                   uint64_t *__restrict__ siblings, uint32_t *__restrict__ path_bits,
                                                   uint32_t *__restrict__ depth, uint64_t *__restrict__ leaves) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t b = g >> 5, l = g & 31;
  const bool valid = b < nidx;
  const uint64_t i = valid ? idx[b] : 0;
  const uint64_t sib = (i >> l) ^ 1;
  const bool hashed = valid && l + 1 < lv.nlevels && sib < lv.len[l];
  const uint32_t m = (uint32_t)(__ballot(hashed) >> (threadIdx.x & 32));
  if (!valid) return;
  const uint32_t d = __popc(m);
  uint64_t *out = siblings + (uint64_t)b * ACC_PATH_SLOTS * 4;
  if (hashed) {
    const uint64_t *c = dig + (lv.off[l] + sib) * 4;
    uint64_t *o = out + __popc(m & ((1u << l) - 1)) * 4;
#pragma unroll
    for (int j = 0; j < 4; j++) o[j] = c[j];
  }
  if (l >= d) {
#pragma unroll
    for (int j = 0; j < 4; j++) out[l * 4 + j] = 0;
  }
  if (l == 0) {
    uint32_t bits = 0, k = 0;
    for (uint32_t mm = m; mm; mm &= mm - 1, k++) bits |= (uint32_t)((i >> (__ffs(mm) - 1)) & 1) << k;
    path_bits[b] = bits;
    depth[b] = d;
    if (leaves) {
#pragma unroll
      for (int j = 0; j < 4; j++) leaves[(uint64_t)b * 4 + j] = dig[i * 4 + j];
    }
  }
}

// one lane per queried size m[i]: the root the tree had when it held leaves
// [0, m), HostTree::prefix_root's fold (acc_layout.h): at most 31 dependent
// permutations, the running digest in registers.  Read-only; it runs after the
// append that made `lv` on the same stream.  The level counter is uniform, so
// the table is read with scalar loads; a lane whose prefix is finished leaves
// the loop.  m outside 1..n cannot be reached (the host checks before it
// enqueues): such a lane reads nothing and answers the zero digest.
__global__ void __launch_bounds__(256) k_acc_prefix_roots(const uint64_t *__restrict__ dig, AccLevels lv,
                                                          const uint64_t *__restrict__ m, uint32_t k,
                                                          uint64_t *__restrict__ roots) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= k) return;
  const uint64_t mi = m[i];
  uint64_t s[12];
  if (mi == 0 || mi > lv.len[0]) {
#pragma unroll
    for (int j = 0; j < 4; j++) roots[(uint64_t)i * 4 + j] = 0;
    return;
  }
#pragma unroll
  for (int j = 0; j < 4; j++) s[j] = dig[(mi - 1) * 4 + j];
  for (uint32_t l = 0; l + 1 < lv.nlevels; l++) {
    const uint64_t c = (mi + ((uint64_t)1 << l) - 1) >> l;
    if (c <= 1) break;
    if (c & 1) continue;  // the prefix's last node at this level is promoted
    const uint64_t *left = dig + (lv.off[l] + c - 2) * 4;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      s[4 + j] = s[j];
      s[j] = left[j];
    }
    node_digest(s);
  }
#pragma unroll
  for (int j = 0; j < 4; j++) roots[(uint64_t)i * 4 + j] = s[j];
}

// ---- the levels above level 0 after an update (acc_kernels.h).  A node of
// level l is remade from nodes 2j, 2j + 1 of level l - 1, which the previous
// launch (or the owner, for the leaves) left final; a node whose right child
// lies beyond the level's end is a promotion, a copy of the left child.

// the row form of one node: the 16-lane row of lane l16 remakes node j of
// `level`.  The permutation runs for a promoted node too (on the left child
// alone) and is dropped at the store, so no lane leaves the DPP broadcasts.
__device__ __forceinline__ void acc_node_row(uint64_t *__restrict__ dig, const AccLevels &lv, uint32_t level,
                                             uint64_t j, uint32_t l16) {
  const uint64_t *c = dig + (lv.off[level - 1] + 2 * j) * 4;
  const bool pair = 2 * j + 1 < lv.len[level - 1];
  const uint64_t in = l16 < (pair ? 8u : 4u) ? c[l16] : 0;
  const uint64_t x = pc::permute_row(in);
  if (l16 < 4) dig[(lv.off[level] + j) * 4 + l16] = pair ? psd::canon(x) : in;
}

// append, narrow range: nodes [first, first + count) of `level`, one 16-lane
// row per node, 16 nodes per block; rows past the range exit together
__global__ void __launch_bounds__(256) k_acc_range_row(uint64_t *__restrict__ dig, AccLevels lv, uint32_t level,
                                                       uint64_t first, uint32_t count) {
  const uint32_t r = blockIdx.x * 16 + (threadIdx.x >> 4);
  if (r >= count) return;
  acc_node_row(dig, lv, level, first + r, threadIdx.x & 15);
}

// replace, level 0: leaf b of the batch into slot idx[b] (one lane per felt)
__global__ void __launch_bounds__(256) k_acc_put(uint64_t *__restrict__ dig, const uint64_t *__restrict__ idx,
                                                 const uint64_t *__restrict__ leaves, uint32_t k) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (uint64_t)k * 4) return;
  dig[idx[g >> 2] * 4 + (g & 3)] = leaves[g];
}

// replace, one level: the dirty nodes are unique(idx >> level), idx ascending.
// Of the batch entries with the same idx >> level the first owns the node and
// the others leave at once, so every dirty node is written exactly once; its
// children are final because the level below was a launch of its own.  One
// lane per batch entry.
__global__ void __launch_bounds__(256) k_acc_scatter(uint64_t *__restrict__ dig, AccLevels lv, uint32_t level,
                                                     const uint64_t *__restrict__ idx, uint32_t k) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= k) return;
  const uint64_t j = idx[b] >> level;
  if (b && (idx[b - 1] >> level) == j) return;
  const uint64_t *c = dig + (lv.off[level - 1] + 2 * j) * 4;
  const bool pair = 2 * j + 1 < lv.len[level - 1];
  uint64_t s[12];
#pragma unroll
  for (int i = 0; i < 4; i++) s[i] = c[i];
#pragma unroll
  for (int i = 4; i < 8; i++) s[i] = pair ? c[i] : 0;
  node_digest(s);
  if (!pair) {  // promoted: the left child again, unhashed
#pragma unroll
    for (int i = 0; i < 4; i++) s[i] = c[i];
  }
  uint64_t *o = dig + (lv.off[level] + j) * 4;
#pragma unroll
  for (int i = 0; i < 4; i++) o[i] = s[i];
}

// the same in the row form: one 16-lane row per batch entry; the rows that do
// not own their node exit whole (the owner rule of k_acc_scatter)
__global__ void __launch_bounds__(256) k_acc_scatter_row(uint64_t *__restrict__ dig, AccLevels lv, uint32_t level,
                                                         const uint64_t *__restrict__ idx, uint32_t k) {
  const uint32_t b = blockIdx.x * 16 + (threadIdx.x >> 4);
  if (b >= k) return;
  const uint64_t j = idx[b] >> level;
  if (b && (idx[b - 1] >> level) == j) return;
  acc_node_row(dig, lv, level, j, threadIdx.x & 15);
}

void acc_paths(const uint64_t *dig, const AccLevels &lv, const uint64_t *idx, uint32_t nidx, uint64_t *siblings,
               uint32_t *path_bits, uint32_t *depth, uint64_t *leaves, hipStream_t s) {
  if (!nidx) return;
  k_acc_paths<<<(unsigned)(((uint64_t)nidx * ACC_PATH_SLOTS + 255) / 256), 256, 0, s>>>(
      dig, lv, idx, nidx, siblings, path_bits, depth, leaves);
}

void acc_prefix_roots(const uint64_t *dig, const AccLevels &lv, const uint64_t *m, uint32_t k, uint64_t *roots,
                      hipStream_t s) {
  if (!k) return;
  k_acc_prefix_roots<<<(k + 255) / 256, 256, 0, s>>>(dig, lv, m, k, roots);
}

// nodes [a, e) of level l (a even-aligned source: pairs from 2a) from level
// l - 1; true when k_acc_fold finished the tree from level l - 1 up
static bool acc_range(uint64_t *dig, const AccLevels &lv, uint32_t l, uint64_t a, uint64_t e, uint64_t row_max,
                      hipStream_t s) {
  const uint64_t count = e - a;
  if (count < row_max) {
    k_acc_range_row<<<(unsigned)((count + 15) / 16), 256, 0, s>>>(dig, lv, l, a, (uint32_t)count);
    return false;
  }
  if (lv.len[l - 1] <= ACC_FOLD_MAX) {
    k_acc_fold<<<1, ACC_FOLD_MAX, 0, s>>>(dig, lv, l - 1);
    return true;
  }
  // one lane per pair (len > ACC_FOLD_MAX: at least 32 pairs in the whole level)
  const uint64_t *src = dig + (lv.off[l - 1] + 2 * a) * 4;
  uint64_t *dst = dig + (lv.off[l] + a) * 4;
  const uint64_t nsrc = lv.len[l - 1] - 2 * a;
  if (nsrc == 1)  // the range is one promoted node: no pair for k_acc_level's lane 0
    (void)hipMemcpyAsync(dst, src, 32, hipMemcpyDeviceToDevice, s);
  else
    k_acc_level<<<(unsigned)((nsrc / 2 + 255) / 256), 256, 0, s>>>(src, nsrc, dst);
  return false;
}

void acc_append(uint64_t *dig, const AccLevels &lv, uint64_t n_old, uint64_t row_max, hipStream_t s) {
  for (uint32_t l = 1; l < lv.nlevels; l++)
    if (acc_range(dig, lv, l, n_old >> l, lv.len[l], row_max, s)) return;
}

void acc_replace(uint64_t *dig, const AccLevels &lv, const uint64_t *idx, const uint64_t *leaves, uint32_t k,
                 uint64_t row_max, hipStream_t s) {
  if (!k) return;
  k_acc_put<<<(unsigned)(((uint64_t)k * 4 + 255) / 256), 256, 0, s>>>(dig, idx, leaves, k);
  for (uint32_t l = 1; l < lv.nlevels; l++) {
    if (k >= lv.len[l]) {  // no fewer entries than nodes: the whole level, as a range
      if (acc_range(dig, lv, l, 0, lv.len[l], row_max, s)) return;
    } else if (k < row_max) {
      k_acc_scatter_row<<<(k + 15) / 16, 256, 0, s>>>(dig, lv, l, idx, k);
    } else if (lv.len[l - 1] <= ACC_FOLD_MAX) {
      k_acc_fold<<<1, ACC_FOLD_MAX, 0, s>>>(dig, lv, l - 1);
      return;
    } else {
      k_acc_scatter<<<(k + 255) / 256, 256, 0, s>>>(dig, lv, l, idx, k);
    }
  }
}

}  // namespace qpk
