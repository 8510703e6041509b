// fri.hip — the FRI stages on gfx950, batched
// over proofs of one circuit (blockIdx.y = proof index, per-proof strides):
//
//   k_fri_compose / _divide  prove_openings: alpha-reduce + divide by (X - z)
//   k_fri_leaf, k_fold       fri_committed_trees: leaves of 2^a ext, folding
//   k_gather_*               query-round openings
#include "field.h"
#include "poseidon_dev.h"
#include "poseidon_coop.h"
#include "paths.h"
#include "prover_kernels.h"
#include "prover_dev.h"
#include <algorithm>

namespace qpk {

// comp[k] = sum_j alpha^j c_j[k] over the listed oracles (Horner, reverse order)
__global__ void __launch_bounds__(256) k_fri_compose(FriComposeArgs a) {
  const uint32_t n = 1u << a.log_n;
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const uint32_t b = blockIdx.y;
  const uint64_t *ch = a.chal + b * CHAL_STRIDE;
  const ext al{ch[CH_FRI_ALPHA], ch[CH_FRI_ALPHA + 1]};
  ext acc{0, 0};
  for (int o = (int)a.noracles - 1; o >= 0; o--) {
    const uint64_t *base = a.coeffs[o] + b * a.bstride[o] + k;
    for (uint32_t p = a.npolys[o]; p-- > 0;) acc = gl::ext_add(gl::ext_mul(acc, al), ext{base[(uint64_t)p * n], 0});
  }
  ext acc2{0, 0};
  const uint64_t *zb = a.coeffs[2] + b * a.bstride[2] + k;
  for (uint32_t p = a.nnext; p-- > 0;) acc2 = gl::ext_add(gl::ext_mul(acc2, al), ext{zb[(uint64_t)p * n], 0});
  uint64_t *o1 = a.comp + b * (4ull * n);
  o1[k] = acc.c0;
  o1[n + k] = acc.c1;
  o1[2 * n + k] = acc2.c0;
  o1[3 * n + k] = acc2.c1;
}

// suffix-scan form of divide_by_linear: q_{k-1} = sum_{i>=k} c_i z^{i-k}
//   = z^{-k} S_k with S_k = sum_{i>=k} c_i z^i; final = alpha^nc Q1 + Q2
// MAXPER: n / blockDim.x values per thread (16 up to n = 2^14; 64 for the
// degree-2^15/2^16 top aggregation circuits, whose arrays live in scratch)
template <int MAXPER>
__global__ void __launch_bounds__(1024) k_fri_divide(const uint64_t *__restrict__ comp, uint64_t *__restrict__ fin,
                                                     uint32_t log_n, const uint64_t *__restrict__ chal,
                                                     uint64_t f_bstride, uint64_t f_cstride) {
  __shared__ ext sh[1024];
  const uint32_t n = 1u << log_n, b = blockIdx.x;
  const uint64_t *ch = chal + b * CHAL_STRIDE;
  const uint32_t T = blockDim.x, per = n / T;
  const uint32_t lo = threadIdx.x * per;
  ext res[MAXPER];
  for (int pass = 0; pass < 2; pass++) {
    const uint64_t *cc = comp + b * (4ull * n) + (uint64_t)pass * 2 * n;
    const ext z{ch[pass ? CH_ZETA_NEXT : CH_ZETA], ch[(pass ? CH_ZETA_NEXT : CH_ZETA) + 1]};
    const ext zi{ch[pass ? CH_ZETA_NEXT_INV : CH_ZETA_INV], ch[(pass ? CH_ZETA_NEXT_INV : CH_ZETA_INV) + 1]};
    // local suffix sums within [lo, lo+per) of d_i = c_i z^i
    ext zp = gl::ext_pow(z, lo);
    ext d[MAXPER];
    for (uint32_t i = 0; i < per; i++) {
      d[i] = gl::ext_mul(ext{cc[lo + i], cc[n + lo + i]}, zp);
      zp = gl::ext_mul(zp, z);
    }
    ext tot{0, 0};
    for (uint32_t i = per; i-- > 0;) {
      tot = gl::ext_add(tot, d[i]);
      d[i] = tot;
    }
    sh[threadIdx.x] = tot;
    __syncthreads();
    // inclusive suffix scan across threads
    for (uint32_t off = 1; off < T; off <<= 1) {
      ext v = threadIdx.x + off < T ? sh[threadIdx.x + off] : ext{0, 0};
      __syncthreads();
      sh[threadIdx.x] = gl::ext_add(sh[threadIdx.x], v);
      __syncthreads();
    }
    const ext after = threadIdx.x + 1 < T ? sh[threadIdx.x + 1] : ext{0, 0};
    __syncthreads();
    // q_{k-1} = z^{-k} (S_k) for k >= 1; output index m = k-1; q_{n-1} = 0 (padding)
    ext zk = gl::ext_pow(zi, lo);
    for (uint32_t i = 0; i < per; i++) {
      const uint32_t k = lo + i;
      ext q = gl::ext_mul(gl::ext_add(d[i], after), zk);  // S_k z^-k = q_{k-1}
      zk = gl::ext_mul(zk, zi);
      if (pass == 0) {
        res[i] = q;
      } else {
        res[i] = gl::ext_add(res[i], q);
      }
      (void)k;
    }
    if (pass == 0) {
      const ext ap{ch[CH_ALPHA_POW_NC], ch[CH_ALPHA_POW_NC + 1]};
      for (uint32_t i = 0; i < per; i++) res[i] = gl::ext_mul(res[i], ap);
    }
  }
  // res[i] at k = lo+i holds q_{k-1}; shift down by one, q_{n-1} = 0
  uint64_t *o = fin + b * f_bstride;
  for (uint32_t i = 0; i < per; i++) {
    const uint32_t k = lo + i;
    if (k == 0) continue;
    o[k - 1] = res[i].c0;
    o[f_cstride + k - 1] = res[i].c1;
  }
  if (threadIdx.x == T - 1) {
    o[n - 1] = 0;
    o[f_cstride + n - 1] = 0;
  }
}

void fri_initial_poly(const FriComposeArgs &a, uint64_t *fin, uint64_t f_bstride, uint64_t f_cstride, uint32_t nb,
                      hipStream_t s) {
  const uint64_t n = 1ull << a.log_n;
  k_fri_compose<<<dim3(cdiv(n, 256), nb), 256, 0, s>>>(a);
  // k_fri_divide: n / 8 threads up to 1024, n / threads values each (n >= 2^6: at least 8 threads;
  // <16> holds 16 per thread, n <= 2^14; <64> holds 64, n <= 2^16)
  const unsigned T = (unsigned)std::min<uint64_t>(1024, n / 8);
  if (n / T <= 16)
    k_fri_divide<16><<<nb, T, 0, s>>>(a.comp, fin, a.log_n, a.chal, f_bstride, f_cstride);
  else
    k_fri_divide<64><<<nb, 1024, 0, s>>>(a.comp, fin, a.log_n, a.chal, f_bstride, f_cstride);
}

// FRI layer leaves: leaf i = 2^ab consecutive leaf-order ext values, interleaved c0,c1
__global__ void __launch_bounds__(256) k_fri_leaf(const uint64_t *__restrict__ vals, uint64_t *__restrict__ dig,
                                                  uint32_t log_len, uint32_t ab, uint64_t v_bstride, uint64_t d_bstride) {
  const uint32_t nleaves = 1u << (log_len - ab);
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nleaves) return;
  const uint32_t b = blockIdx.y;
  const uint64_t L = 1ull << log_len;
  const uint64_t *c0 = vals + b * v_bstride + ((uint64_t)i << ab);
  const uint64_t *c1 = c0 + L;
  const uint32_t W = 2u << ab;
  uint64_t *o = dig + b * d_bstride + (uint64_t)i * 4;
  if (W <= 4) {  // hash_or_noop: a leaf of <= 4 elements is its own digest (arity 2)
    o[0] = psd::canon(c0[0]); o[1] = psd::canon(c1[0]); o[2] = psd::canon(c0[1]); o[3] = psd::canon(c1[1]);
    return;
  }
  uint64_t s[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (uint32_t off = 0; off < W; off += 8) {
#pragma unroll
    for (uint32_t k = 0; k < 8; k += 2) {
      const uint32_t e = (off + k) >> 1;
      if (off + k < W) {
        s[k] = c0[e];
        s[k + 1] = c1[e];
      }
    }
    psd::permute_nc(s);
  }
  o[0] = psd::canon(s[0]); o[1] = psd::canon(s[1]); o[2] = psd::canon(s[2]); o[3] = psd::canon(s[3]);
}

// k_fri_leaf with one 16-lane row per leaf (pc::permute_row): a layer of few
// leaves (small batches, the upper FRI layers) otherwise costs a one-lane
// permutation's latency per absorbed chunk whatever its width
__global__ void __launch_bounds__(256) k_fri_leaf_row(const uint64_t *__restrict__ vals, uint64_t *__restrict__ dig,
                                                      uint32_t log_len, uint32_t ab, uint64_t v_bstride,
                                                      uint64_t d_bstride) {
  const uint32_t i = blockIdx.x * 16 + (threadIdx.x >> 4), l16 = threadIdx.x & 15;
  if (i >= (1u << (log_len - ab))) return;
  const uint32_t b = blockIdx.y;
  const uint64_t L = 1ull << log_len;
  const uint64_t *c0 = vals + b * v_bstride + ((uint64_t)i << ab);
  const uint32_t W = 2u << ab;  // > 4 (the launcher sends arity 2 to k_fri_leaf)
  uint64_t x = 0;
  for (uint32_t off = 0; off < W; off += 8) {
    const uint32_t e = off + l16;  // element e: c0/c1 of value e >> 1
    if (l16 < 8 && e < W) x = (e & 1 ? c0 + L : c0)[e >> 1];
    x = pc::permute_row(x);
  }
  if (l16 < 4) dig[b * d_bstride + (uint64_t)i * 4 + l16] = psd::canon(x);
}

// leaves of a FRI layer: the row form up to FRI_ROW_MAX leaves over the
// batch (path hook fri_row), the one-lane form above
constexpr long FRI_ROW_MAX = 16384;
void fri_leaf(const uint64_t *vals, uint64_t *dig, uint32_t log_len, uint32_t ab, uint64_t v_bstride,
              uint64_t d_bstride, uint32_t nb, hipStream_t s) {
  const uint64_t lim = (uint64_t)path_opt("fri_row", FRI_ROW_MAX);
  const uint64_t nl = 1ull << (log_len - ab);
  if ((2u << ab) > 4 && nl * nb <= lim)
    k_fri_leaf_row<<<dim3((unsigned)((nl + 15) / 16), nb), 256, 0, s>>>(vals, dig, log_len, ab, v_bstride, d_bstride);
  else
    k_fri_leaf<<<dim3((unsigned)((nl + 255) / 256), nb), 256, 0, s>>>(vals, dig, log_len, ab, v_bstride, d_bstride);
}

void fri_layer_tree(const Twiddles &tw, const uint64_t *coef, uint64_t coef_cstride, uint64_t coef_bstride,
                    uint32_t coef_log, uint64_t *vals, uint64_t *dig, uint32_t log_len, uint32_t ab, uint32_t cap_h,
                    uint64_t shift, uint32_t nb, hipStream_t s) {
  const uint64_t dbs = tree_digest_count(log_len - ab, cap_h) * 4;
  lde(tw, coef, coef_cstride, vals, 1ull << log_len, 2, coef_log, log_len - coef_log, shift, nb, coef_bstride,
      2ull << log_len, s);
  fri_leaf(vals, dig, log_len, ab, 2ull << log_len, dbs, nb, s);
  merkle_tree(dig, log_len - ab, cap_h, nb, dbs, s);
}

// fold: out[k] = sum_{i<2^ab} beta^i c[2^ab k + i]  (coefficients, ext as 2 columns).
// Only the first 2^log_nz input coefficients can be nonzero (the layer-0
// polynomial has degree < n in a length-N buffer): outputs past them are
// written as zeros without reading the zero tail.
__global__ void __launch_bounds__(256) k_fold(const uint64_t *__restrict__ cin, uint64_t *__restrict__ cout,
                                              uint32_t log_len, uint32_t ab, uint32_t layer,
                                              const uint64_t *__restrict__ chal, uint64_t i_bstride,
                                              uint64_t o_bstride, uint32_t log_nz) {
  const uint32_t nout = 1u << (log_len - ab);
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nout) return;
  const uint32_t b = blockIdx.y;
  uint64_t *o = cout + b * o_bstride;
  if (((uint64_t)k << ab) >= (1ull << log_nz)) {
    o[k] = 0;
    o[nout + k] = 0;
    return;
  }
  const uint64_t *ch = chal + b * CHAL_STRIDE;
  const ext beta{ch[CH_FRI_BETA + 2 * layer], ch[CH_FRI_BETA + 2 * layer + 1]};
  const uint64_t L = 1ull << log_len;
  const uint64_t *c0 = cin + b * i_bstride, *c1 = c0 + L;
  ext acc{0, 0};
  for (uint32_t i = 1u << ab; i-- > 0;) {
    const uint64_t idx = ((uint64_t)k << ab) + i;
    acc = gl::ext_add(gl::ext_mul(acc, beta), ext{c0[idx], c1[idx]});
  }
  o[k] = acc.c0;
  o[nout + k] = acc.c1;
}

void fold(const uint64_t *cin, uint64_t *cout, uint32_t log_len, uint32_t ab, uint32_t layer, const uint64_t *chal,
          uint64_t i_bstride, uint64_t o_bstride, uint32_t log_nz, uint32_t nb, hipStream_t s) {
  k_fold<<<dim3(cdiv(1ull << (log_len - ab), 256), nb), 256, 0, s>>>(cin, cout, log_len, ab, layer, chal, i_bstride,
                                                                     o_bstride, log_nz);
}

// ---------------------------------------------------------------- gathers

// out[b][q][c] = cols[b*bstride + c*stride + idx[b][q] >> shift]
__global__ void k_gather_rows_b(const uint64_t *__restrict__ cols, uint64_t stride, uint64_t bstride, uint32_t ncols,
                                const uint32_t *__restrict__ idx, uint32_t nq, uint32_t shift,
                                uint64_t *__restrict__ out, uint64_t o_bstride) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t b = blockIdx.y;
  if (t >= ncols * nq) return;
  const uint32_t q = t / ncols, c = t % ncols;
  out[b * o_bstride + t] = cols[b * bstride + (uint64_t)c * stride + (idx[b * nq + q] >> shift)];
}

// out[b][q][k][4] = sibling digest at level k of leaf idx[b][q] >> shift
__global__ void k_gather_paths_b(const uint64_t *__restrict__ dig, uint64_t d_bstride, uint32_t log_leaves,
                                 uint32_t cap_h, const uint32_t *__restrict__ idx, uint32_t nq, uint32_t shift,
                                 uint64_t *__restrict__ out, uint64_t o_bstride) {
  const uint32_t depth = log_leaves - cap_h;
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t b = blockIdx.y;
  if (t >= nq * depth * 4) return;
  const uint32_t q = t / (depth * 4), r = t % (depth * 4), k = r / 4, e = r % 4;
  uint64_t off = 0;
  for (uint32_t j = 0; j < k; j++) off += (uint64_t)1 << (log_leaves - j);
  const uint64_t leaf = idx[b * nq + q] >> shift;
  const uint64_t sib = (leaf >> k) ^ 1u;
  out[b * o_bstride + t] = dig[b * d_bstride + (off + sib) * 4 + e];
}

// FRI layer leaves for queries: out[b][q][2*arity] interleaved from 2 columns
__global__ void k_gather_fri_leaf(const uint64_t *__restrict__ vals, uint64_t v_bstride, uint32_t log_len, uint32_t ab,
                                  const uint32_t *__restrict__ idx, uint32_t nq, uint32_t shift,
                                  uint64_t *__restrict__ out, uint64_t o_bstride) {
  const uint32_t W = 2u << ab;
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t b = blockIdx.y;
  if (t >= nq * W) return;
  const uint32_t q = t / W, e = t % W;
  const uint64_t leaf = idx[b * nq + q] >> shift;
  const uint64_t L = 1ull << log_len;
  out[b * o_bstride + t] = vals[b * v_bstride + (e & 1) * L + (leaf << ab) + (e >> 1)];
}

void gather_rows(const uint64_t *cols, uint64_t stride, uint64_t bstride, uint32_t ncols, const uint32_t *idx,
                 uint32_t nq, uint32_t shift, uint64_t *out, uint64_t o_bstride, uint32_t nb, hipStream_t s) {
  const uint64_t tot = (uint64_t)ncols * nq;
  if (!tot) return;
  k_gather_rows_b<<<dim3(cdiv(tot, 256), nb), 256, 0, s>>>(cols, stride, bstride, ncols, idx, nq, shift, out, o_bstride);
}

void gather_paths(const uint64_t *dig, uint64_t d_bstride, uint32_t log_leaves, uint32_t cap_h, const uint32_t *idx,
                  uint32_t nq, uint32_t shift, uint64_t *out, uint64_t o_bstride, uint32_t nb, hipStream_t s) {
  const uint64_t tot = (uint64_t)nq * (log_leaves - cap_h) * 4;
  if (!tot) return;
  k_gather_paths_b<<<dim3(cdiv(tot, 256), nb), 256, 0, s>>>(dig, d_bstride, log_leaves, cap_h, idx, nq, shift, out,
                                                            o_bstride);
}

void gather_fri_leaf(const uint64_t *vals, uint64_t v_bstride, uint32_t log_len, uint32_t ab, const uint32_t *idx,
                     uint32_t nq, uint32_t shift, uint64_t *out, uint64_t o_bstride, uint32_t nb, hipStream_t s) {
  const uint64_t tot = (uint64_t)nq * (2u << ab);
  if (!tot) return;
  k_gather_fri_leaf<<<dim3(cdiv(tot, 256), nb), 256, 0, s>>>(vals, v_bstride, log_len, ab, idx, nq, shift, out,
                                                             o_bstride);
}

}  // namespace qpk
