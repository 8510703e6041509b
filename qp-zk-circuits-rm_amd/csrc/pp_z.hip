// pp_z.hip — wires_permutation_partial_products_and_zs (SURVEY.md section 8
// row a9) on gfx950, batched over proofs of one circuit (blockIdx.y = proof
// index, per-proof strides): k_pp_rows / k_pp_rows_t, then k_z_scan.
#include "field.h"
#include "field_nc.h"
#include "ntt16.h"
#include "prover_kernels.h"
#include "prover_dev.h"

namespace qpk {

// per row: P_j = prod_{k<=j} num_k/den_k over chunks of qdf routed wires
__global__ void __launch_bounds__(256) k_pp_rows(const uint64_t *__restrict__ wires, const uint64_t *__restrict__ sigmas,
                                                 const uint64_t *__restrict__ k_is, const uint64_t *__restrict__ chal,
                                                 uint64_t *__restrict__ prods, uint32_t log_n, uint32_t R, uint32_t qdf,
                                                 uint32_t nc, uint64_t w_bstride, uint64_t p_bstride,
                                                 const uint64_t *__restrict__ tw) {
  const uint32_t n = 1u << log_n;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t b = blockIdx.y;
  wires += b * w_bstride;
  prods += b * p_bstride;
  const uint64_t *ch = chal + b * CHAL_STRIDE;
  const uint64_t x = wpow_N(tw, i, log_n);
  const uint32_t nchunks = (R + qdf - 1) / qdf;
  for (uint32_t c = 0; c < nc; c++) {
    const uint64_t beta = ch[CH_BETA + c], gamma = ch[CH_GAMMA + c];
    uint64_t num[16], den[16];
    for (uint32_t k = 0; k < nchunks; k++) {
      uint64_t nn = 1, dd = 1;
      for (uint32_t j = k * qdf; j < (k + 1) * qdf && j < R; j++) {
        uint64_t wv = wires[(uint64_t)j * n + i];
        nn = gl::mul(nn, gl::add(gl::add(wv, gl::mul(beta, gl::mul(k_is[j], x))), gamma));
        dd = gl::mul(dd, gl::add(gl::add(wv, gl::mul(beta, sigmas[(uint64_t)j * n + i])), gamma));
      }
      num[k] = nn;
      den[k] = dd;
    }
    // batch inversion of den[0..nchunks)
    uint64_t pre[16], acc = 1;
    for (uint32_t k = 0; k < nchunks; k++) {
      pre[k] = acc;
      acc = gl::mul(acc, den[k]);
    }
    uint64_t inv = gl::inv(acc);
    for (uint32_t k = nchunks; k-- > 0;) {
      uint64_t t = gl::mul(inv, pre[k]);
      inv = gl::mul(inv, den[k]);
      den[k] = t;
    }
    uint64_t run = 1;
    for (uint32_t k = 0; k < nchunks; k++) {
      run = gl::mul(run, gl::mul(num[k], den[k]));
      prods[((uint64_t)c * nchunks + k) * n + i] = run;
    }
  }
}

// a^(p-2) by the addition chain of p - 2 = (2^32 - 2) 2^32 + (2^32 - 1):
// 63 squarings + 8 products (the generic gl::inv runs a 64-step
// square-and-multiply loop with a product per set bit: 125 products)
__device__ __forceinline__ uint64_t inv_chain(uint64_t x) {
  auto sq = [](uint64_t v, int k) {
#pragma unroll
    for (int i = 0; i < k; i++) v = gfn::mul(v, v);
    return v;
  };
  const uint64_t t1 = x;
  const uint64_t t2 = gfn::mul(sq(t1, 1), t1);   // x^(2^2-1)
  const uint64_t t3 = gfn::mul(sq(t2, 1), t1);   // x^(2^3-1)
  const uint64_t t6 = gfn::mul(sq(t3, 3), t3);   // x^(2^6-1)
  const uint64_t t12 = gfn::mul(sq(t6, 6), t6);  // x^(2^12-1)
  const uint64_t t24 = gfn::mul(sq(t12, 12), t12);
  const uint64_t t30 = gfn::mul(sq(t24, 6), t6);
  const uint64_t t31 = gfn::mul(sq(t30, 1), t1);  // x^(2^31-1)
  const uint64_t t32 = gfn::mul(sq(t31, 1), t1);  // x^(2^32-1)
  // x^(2^32-2) = (x^(2^31-1))^2; then shift up 32 and add 2^32-1
  return gfn::mul(sq(sq(t31, 1), 32), t32);
}

// k_pp_rows for the leaf circuits' shape (R routed wires in chunks of QDF,
// 2 challenges), compile-time so the per-row chunk values stay in registers:
// the numerator term is w + gamma + k_j (beta x) (beta x once per row), and
// the running quotient is kept as a fraction N_k / D_k (prefix products of
// the chunk numerators and denominators), so one inversion of D_last per
// challenge gives every D_k^-1 walking back (D_(k-1)^-1 = D_k^-1 den_k).
// Non-canonical arithmetic inside (field_nc.h), canonical products out.  Same
// values as k_pp_rows (plonky2 wires_permutation_partial_products_and_zs).
template <int R, int QDF>
__global__ void __launch_bounds__(256) k_pp_rows_t(const uint64_t *__restrict__ wires,
                                                   const uint64_t *__restrict__ sigmas,
                                                   const uint64_t *__restrict__ k_is,
                                                   const uint64_t *__restrict__ chal, uint64_t *__restrict__ prods,
                                                   uint32_t log_n, uint64_t w_bstride, uint64_t p_bstride,
                                                   const uint64_t *__restrict__ tw) {
  constexpr int NCH = (R + QDF - 1) / QDF;
  const uint32_t n = 1u << log_n;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t b = blockIdx.y;
  wires += b * w_bstride;
  prods += b * p_bstride;
  const uint64_t *ch = chal + b * CHAL_STRIDE;
  const uint64_t x = wpow_N(tw, i, log_n);
#pragma unroll 1
  for (int c = 0; c < 2; c++) {
    const uint64_t beta = ch[CH_BETA + c], gamma = ch[CH_GAMMA + c];
    const uint64_t bx = gfn::mul(beta, x);
    uint64_t N[NCH], den[NCH], D = 1;
#pragma unroll
    for (int k = 0; k < NCH; k++) {
      uint64_t nn = 1, dd = 1;
#pragma unroll
      for (int jj = 0; jj < QDF; jj++) {
        const int j = k * QDF + jj;
        if (j < R) {
          const uint64_t wg = gfn::add(wires[(uint64_t)j * n + i], gamma);
          const uint64_t nj = gfn::add(wg, gfn::mul(k_is[j], bx));
          const uint64_t dj = gfn::add(wg, gfn::mul(beta, sigmas[(uint64_t)j * n + i]));
          nn = jj ? gfn::mul(nn, nj) : nj;
          dd = jj ? gfn::mul(dd, dj) : dj;
        }
      }
      N[k] = k ? gfn::mul(N[k - 1], nn) : nn;
      den[k] = dd;
      D = k ? gfn::mul(D, dd) : dd;
    }
    uint64_t dinv = inv_chain(D);
    uint64_t *out = prods + (uint64_t)c * NCH * n + i;
#pragma unroll
    for (int k = NCH - 1; k >= 0; k--) {
      out[(uint64_t)k * n] = gfn::canon(gfn::mul(N[k], dinv));
      if (k) dinv = gfn::mul(dinv, den[k]);
    }
  }
}

// exclusive prefix product of the full-row products -> Z; pp_j = Z * P_j.
// The row products go through LDS (coalesced in, each thread's contiguous
// chunk scanned from LDS, Z written back over them), so every HBM access is a
// coalesced row sweep: n reads of the full products, (npp) reads of the
// partial products, (1 + npp) n writes per challenge.
// STAGE = true: the row products are staged in LDS (n <= 2^14); false: read
// from HBM (the degree-2^15/2^16 top aggregation circuits), Z written there
template <bool STAGE>
__global__ void __launch_bounds__(1024) k_z_scan(const uint64_t *__restrict__ prods, uint64_t *__restrict__ zs,
                                                 uint32_t log_n, uint32_t nc, uint32_t nchunks, uint64_t p_bstride,
                                                 uint64_t z_bstride) {
  extern __shared__ __attribute__((aligned(16))) uint64_t zbuf[];  // [lp(n)] rows (STAGE), then [T] partials
  const uint32_t n = 1u << log_n;
  const uint32_t c = blockIdx.x, b = blockIdx.y;
  prods += b * p_bstride + (uint64_t)c * nchunks * n;
  zs += b * z_bstride;
  const uint64_t *full = prods + (uint64_t)(nchunks - 1) * n;
  const uint32_t T = blockDim.x, t = threadIdx.x, per = (n + T - 1) / T;
  uint64_t *part = STAGE ? zbuf + nt::lp(n) : zbuf;
  // staged: row i at zbuf[lp(i)]; unstaged: Z itself is built in zs column c
  uint64_t *zc = zs + (uint64_t)c * n;
  auto row = [&](uint32_t i) -> uint64_t { return STAGE ? zbuf[nt::lp(i)] : full[i]; };
  if constexpr (STAGE) {
    for (uint32_t i = t; i < n; i += T) zbuf[nt::lp(i)] = full[i];
    __syncthreads();
  }
  const uint32_t lo = min(t * per, n), hi = min(lo + per, n);
  uint64_t local = 1;
  for (uint32_t i = lo; i < hi; i++) local = gl::mul(local, row(i));
  part[t] = local;
  __syncthreads();
  // inclusive Hillis-Steele scan over T partial products
  for (uint32_t off = 1; off < T; off <<= 1) {
    uint64_t v = t >= off ? part[t - off] : 1;
    __syncthreads();
    part[t] = gl::mul(part[t], v);
    __syncthreads();
  }
  uint64_t z = t ? part[t - 1] : 1;
  for (uint32_t i = lo; i < hi; i++) {
    const uint64_t f = row(i);
    if constexpr (STAGE) zbuf[nt::lp(i)] = z;
    else zc[i] = z;
    z = gl::mul(z, f);
  }
  __syncthreads();
  const uint32_t npp = nchunks - 1;
  for (uint32_t i = t; i < n; i += T) {
    const uint64_t zi = STAGE ? zbuf[nt::lp(i)] : zc[i];
    if constexpr (STAGE) zc[i] = zi;
    for (uint32_t j = 0; j < npp; j++) zs[((uint64_t)nc + c * npp + j) * n + i] = gl::mul(zi, prods[(uint64_t)j * n + i]);
  }
}

void partial_products_and_zs(const Twiddles &tw, const uint64_t *wires, uint64_t w_bstride, const uint64_t *sigmas,
                             const uint64_t *k_is, const uint64_t *chal, uint64_t *prods, uint64_t *zs,
                             uint64_t z_bstride, uint32_t log_n, uint32_t R, uint32_t qdf, uint32_t nc, uint32_t nb,
                             hipStream_t s) {
  const uint32_t n = 1u << log_n, nchunks = (R + qdf - 1) / qdf;
  const uint64_t pbs = (uint64_t)nc * nchunks * n;
  const dim3 rows(cdiv(n, 256), nb);
  // the leaf circuits' shape takes the compile-time kernel
  if (R == 80 && qdf == 8 && nc == 2)
    k_pp_rows_t<80, 8><<<rows, 256, 0, s>>>(wires, sigmas, k_is, chal, prods, log_n, w_bstride, pbs, tw.fwd);
  else
    k_pp_rows<<<rows, 256, 0, s>>>(wires, sigmas, k_is, chal, prods, log_n, R, qdf, nc, w_bstride, pbs, tw.fwd);
  // LDS: the T = 1024 partial products, after the staged rows
  if (log_n <= LDS_LOG_MAX)
    k_z_scan<true><<<dim3(nc, nb), 1024, 8u * (ntt_lds_words(n) + 1024), s>>>(prods, zs, log_n, nc, nchunks, pbs,
                                                                               z_bstride);
  else
    k_z_scan<false><<<dim3(nc, nb), 1024, 8u * 1024, s>>>(prods, zs, log_n, nc, nchunks, pbs, z_bstride);
}

}  // namespace qpk
