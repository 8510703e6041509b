// openings.hip — OpeningSet::new on gfx950:
// Horner at zeta / g*zeta of every committed polynomial, batched over proofs
// of one circuit (blockIdx.y = proof index, per-proof strides).
#include "field.h"
#include "paths.h"
#include "prover_kernels.h"
#include "prover_dev.h"
#include <algorithm>

namespace qpk {

constexpr int OPEN_PB = 8;  // polys per k_openings block

// value of each coefficient column at an extension point: out[b][poly].
// A block evaluates OPEN_PB polys of one proof: thread t walks k = t + jT with
// one running power z^k shared by the OPEN_PB columns (2 base products per
// coefficient instead of 6), then a tree reduction per poly.  blockDim = T
// (host: 256, or n/4 >= 64 for small circuits so z^t's pow stays amortised).
__global__ void __launch_bounds__(256) k_openings(const uint64_t *__restrict__ coeffs, uint64_t c_bstride,
                                                  uint32_t npolys, uint32_t log_n, const uint64_t *__restrict__ pts,
                                                  uint32_t pt_off, uint64_t *__restrict__ out, uint32_t out_off) {
  __shared__ ext red[OPEN_PB][256];
  const uint32_t n = 1u << log_n, T = blockDim.x, t = threadIdx.x;
  const uint32_t p0 = blockIdx.x * OPEN_PB, b = blockIdx.y;
  const uint32_t np = min((uint32_t)OPEN_PB, npolys - p0);
  const uint64_t *cf = coeffs + b * c_bstride + (uint64_t)p0 * n;
  const ext z = ext{pts[b * CHAL_STRIDE + pt_off], pts[b * CHAL_STRIDE + pt_off + 1]};
  ext zp = gl::ext_pow(z, t);
  const ext zs = gl::ext_pow(z, T);
  ext acc[OPEN_PB];
#pragma unroll
  for (int j = 0; j < OPEN_PB; j++) acc[j] = ext{0, 0};
  for (uint32_t k = t; k < n; k += T) {
#pragma unroll
    for (int j = 0; j < OPEN_PB; j++)
      if ((uint32_t)j < np) acc[j] = gl::ext_add(acc[j], gl::ext_scale(zp, cf[(uint64_t)j * n + k]));
    zp = gl::ext_mul(zp, zs);
  }
#pragma unroll
  for (int j = 0; j < OPEN_PB; j++) red[j][t] = acc[j];
  __syncthreads();
  for (uint32_t o = T / 2; o; o >>= 1) {
    if (t < o)
      for (uint32_t j = 0; j < np; j++) red[j][t] = gl::ext_add(red[j][t], red[j][t + o]);
    __syncthreads();
  }
  if (t < np) {
    uint64_t *dst = out + b * OPEN_STRIDE + 2 * (out_off + p0 + t);
    dst[0] = red[t][0].c0;
    dst[1] = red[t][0].c1;
  }
}

// all of a proof's opening batches in one launch: segment j's polys form
// groups of OPEN_PB from group g0; each group's coefficient range splits into
// S slices of n / S (a small batch otherwise leaves most CUs idle: one proof
// has ~33 groups), whose partial sums k_openings_reduce adds (S > 1)
__global__ void __launch_bounds__(256) k_openings_seg(OpeningsArgs a) {
  __shared__ ext red[OPEN_PB][256];
  const uint32_t n = 1u << a.log_n, T = blockDim.x, t = threadIdx.x;
  const uint32_t g = blockIdx.x / a.S, slice = blockIdx.x % a.S, b = blockIdx.y;
  uint32_t j = 0;
  while (j + 1 < a.nseg && g >= a.seg[j + 1].g0) j++;
  const OpenSeg sg = a.seg[j];
  const uint32_t p0 = (g - sg.g0) * OPEN_PB;
  const uint32_t np = min((uint32_t)OPEN_PB, sg.npolys - p0);
  const uint32_t len = n / a.S, lo = slice * len;
  const uint64_t *cf = sg.coeffs + b * sg.c_bstride + (uint64_t)p0 * n;
  const ext z = ext{a.pts[b * CHAL_STRIDE + sg.pt_off], a.pts[b * CHAL_STRIDE + sg.pt_off + 1]};
  ext zp = gl::ext_pow(z, lo + t);
  const ext zs = gl::ext_pow(z, T);
  ext acc[OPEN_PB];
#pragma unroll
  for (int q = 0; q < OPEN_PB; q++) acc[q] = ext{0, 0};
  for (uint32_t k = lo + t; k < lo + len; k += T) {
#pragma unroll
    for (int q = 0; q < OPEN_PB; q++)
      if ((uint32_t)q < np) acc[q] = gl::ext_add(acc[q], gl::ext_scale(zp, cf[(uint64_t)q * n + k]));
    zp = gl::ext_mul(zp, zs);
  }
#pragma unroll
  for (int q = 0; q < OPEN_PB; q++) red[q][t] = acc[q];
  __syncthreads();
  for (uint32_t o = T / 2; o; o >>= 1) {
    if (t < o)
      for (uint32_t q = 0; q < np; q++) red[q][t] = gl::ext_add(red[q][t], red[q][t + o]);
    __syncthreads();
  }
  if (t < np) {
    const uint32_t idx = sg.out_off + p0 + t;
    uint64_t *dst = a.S == 1 ? a.out + b * OPEN_STRIDE + 2 * idx
                             : a.part + ((uint64_t)(b * a.S + slice) * OPEN_STRIDE + 2 * idx);
    dst[0] = red[t][0].c0;
    dst[1] = red[t][0].c1;
  }
}

__global__ void __launch_bounds__(256) k_openings_reduce(const uint64_t *__restrict__ part, uint64_t *__restrict__ out,
                                                         uint32_t ntot, uint32_t S) {
  const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
  if (idx >= ntot) return;
  ext acc{0, 0};
  for (uint32_t sl = 0; sl < S; sl++) {
    const uint64_t *p = part + (uint64_t)(b * S + sl) * OPEN_STRIDE + 2 * idx;
    acc = gl::ext_add(acc, ext{p[0], p[1]});
  }
  out[b * OPEN_STRIDE + 2 * idx] = acc.c0;
  out[b * OPEN_STRIDE + 2 * idx + 1] = acc.c1;
}

void openings(OpeningsArgs a, uint32_t nb, hipStream_t s) {
  const uint32_t n = 1u << a.log_n;
  const unsigned T = (unsigned)std::min<uint32_t>(256, std::max<uint32_t>(64, n / 4));
  a.ngroups = 0;
  a.ntot = 0;
  for (uint32_t j = 0; j < a.nseg; j++) {
    a.seg[j].g0 = a.ngroups;
    a.ngroups += (a.seg[j].npolys + OPEN_PB - 1) / OPEN_PB;
    a.ntot = std::max(a.ntot, a.seg[j].out_off + a.seg[j].npolys);
  }
  // path hook open_slices=1: one block per group (the shape of the large batches)
  const uint32_t smax = (uint32_t)std::min<long>(std::max<long>(path_opt("open_slices", OPEN_MAX_SLICES), 1),
                                                 OPEN_MAX_SLICES);
  a.S = 1;
  while (a.S * 2 <= smax && a.S * 2 * T * 8 <= n && (uint64_t)a.ngroups * nb * a.S < 1024) a.S *= 2;
  k_openings_seg<<<dim3(a.ngroups * a.S, nb), T, 0, s>>>(a);
  if (a.S > 1) k_openings_reduce<<<dim3((a.ntot + 255) / 256, nb), 256, 0, s>>>(a.part, a.out, a.ntot, a.S);
}

}  // namespace qpk
