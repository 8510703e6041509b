// field_probe.hip — TEST-ONLY probe of the device field arithmetic
// (qp_debug_field_op, include/qpgpu.h).  One lane per element (or per group of
// elements for the 4-wide / K-wide forms) applies one of the functions the
// production kernels call — nt:: (ntt16.h), gfn:: (field_nc.h), pf::
// (poseidon_fast.h), gl:: (field.h) — to a[i], b[i] and stores the raw result,
// not canonicalised, so tests/test_gpu_field_ops.py sees the representation.
// Nothing here restates the arithmetic: the headers are included, not copied.
#include "../../include/qpgpu.h"
#include <algorithm>
#include <string>
#include "ctx.h"
#include "field.h"
#include "field_nc.h"
#include "ntt16.h"
#include "poseidon_fast.h"

namespace {

// elements one lane consumes (0: unknown op / parameter)
uint32_t group_size(uint32_t op, uint32_t param) {
  switch (op) {
    case QP_FOP_NT_ADD4:
    case QP_FOP_NT_SUB4: return param ? 0 : 4;
    case QP_FOP_PF_MULK2: return param ? 0 : 2;
    case QP_FOP_PF_MULK3: return param ? 0 : 3;
    case QP_FOP_NT_MUL_POW2: return (param < 192 && param % 6 == 0) ? 1 : 0;
    case QP_FOP_ACC3: return (param >= 1 && param <= 256) ? param : 0;
    default: return (op < QP_FOP_COUNT && !param) ? 1 : 0;
  }
}

bool unary(uint32_t op) { return op == QP_FOP_PF_SBOX || op == QP_FOP_PF_SBOX_C || op == QP_FOP_NT_MUL_POW2; }

template <int E>
__device__ __forceinline__ uint64_t pow2_e(uint32_t e, uint64_t x) {
  if constexpr (E < 192) {
    if (e == (uint32_t)E) return nt::mul_pow2<E>(x);
    return pow2_e<E + 6>(e, x);
  } else {
    return x;
  }
}

// group g of G elements: a[g G .. g G + G), b likewise; out the same layout
// (QP_FOP_ACC3: one word per group)
template <uint32_t OP>
__global__ void __launch_bounds__(256) k_field_op(const uint64_t *__restrict__ a, const uint64_t *__restrict__ b,
                                                  uint64_t ngroups, uint32_t param, uint64_t *__restrict__ out) {
  for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < ngroups;
       g += (uint64_t)gridDim.x * blockDim.x) {
    if constexpr (OP == QP_FOP_NT_ADD4 || OP == QP_FOP_NT_SUB4) {
      const uint64_t x[4] = {a[4 * g], a[4 * g + 1], a[4 * g + 2], a[4 * g + 3]};
      const uint64_t y[4] = {b[4 * g], b[4 * g + 1], b[4 * g + 2], b[4 * g + 3]};
      uint64_t r[4];
      if constexpr (OP == QP_FOP_NT_ADD4) nt::add4(x, y, r);
      else nt::sub4(x, y, r);
#pragma unroll
      for (int i = 0; i < 4; i++) out[4 * g + i] = r[i];
    } else if constexpr (OP == QP_FOP_PF_MULK2 || OP == QP_FOP_PF_MULK3) {
      constexpr int K = OP == QP_FOP_PF_MULK2 ? 2 : 3;
      uint64_t x[K], y[K], r[K];
#pragma unroll
      for (int i = 0; i < K; i++) {
        x[i] = a[K * g + i];
        y[i] = b[K * g + i];
      }
      gfn::mulk<K>(x, y, r);
#pragma unroll
      for (int i = 0; i < K; i++) out[K * g + i] = r[i];
    } else if constexpr (OP == QP_FOP_ACC3) {
      gfn::Acc3 acc;
      const uint64_t *x = a + g * param, *y = b + g * param;
      for (uint32_t k = 0; k < param; k++) acc.mac(x[k], y[k]);
      acc.add_shifted(x[0], param % 64);
      out[g] = acc.value();
    } else {
      const uint64_t x = a[g], y = b ? b[g] : 0;
      uint64_t r;
      if constexpr (OP == QP_FOP_NT_ADD) r = nt::add(x, y);
      else if constexpr (OP == QP_FOP_GFN_ADD) r = gfn::add(x, y);
      else if constexpr (OP == QP_FOP_GFN_ADD_C) r = gfn::add_c(x, y);
      else if constexpr (OP == QP_FOP_PF_ADD_C) r = pf::add_c(x, y);
      else if constexpr (OP == QP_FOP_GL_ADD) r = gl::add(x, y);
      else if constexpr (OP == QP_FOP_NT_SUB) r = nt::sub(x, y);
      else if constexpr (OP == QP_FOP_GL_SUB) r = gl::sub(x, y);
      else if constexpr (OP == QP_FOP_NT_REDUCE) r = nt::reduce(x, y);
      else if constexpr (OP == QP_FOP_GFN_REDUCE) r = gfn::reduce(x, y);
      else if constexpr (OP == QP_FOP_GL_REDUCE128) r = gl::reduce128(x, y);
      else if constexpr (OP == QP_FOP_PF_REDUCE_ROW) r = pf::reduce_row(x, y);
      else if constexpr (OP == QP_FOP_PF_REDUCE_ROW_C) r = pf::reduce_row_c(x, y);
      else if constexpr (OP == QP_FOP_PF_SUB_SMALL) r = pf::sub_small(x, gfn::lo32(y), gfn::hi32(y));
      else if constexpr (OP == QP_FOP_PF_MUL) r = gfn::mul(x, y);
      else if constexpr (OP == QP_FOP_PF_MUL_C) r = gfn::mul_c(x, y);
      else if constexpr (OP == QP_FOP_GL_MUL) r = gl::mul(x, y);
      else if constexpr (OP == QP_FOP_PF_SBOX) r = pf::sbox(x);
      else if constexpr (OP == QP_FOP_PF_SBOX_C) r = pf::sbox_c(x);
      else if constexpr (OP == QP_FOP_PF_REDUCE_ROW_WIDE) r = pf::reduce_row_wide(x, y);
      else r = pow2_e<0>(param, x);
      out[g] = r;
    }
  }
}

template <uint32_t OP = 0>
void launch(uint32_t op, dim3 grid, hipStream_t s, const uint64_t *a, const uint64_t *b, uint64_t ngroups,
            uint32_t param, uint64_t *out) {
  if constexpr (OP < QP_FOP_COUNT) {
    if (op == OP) k_field_op<OP><<<grid, 256, 0, s>>>(a, b, ngroups, param, out);
    else launch<OP + 1>(op, grid, s, a, b, ngroups, param, out);
  }
}

}  // namespace

extern "C" int qp_debug_field_op(qp_ctx *c, uint32_t op, uint32_t param, const uint64_t *a, const uint64_t *b,
                                 uint64_t n, uint64_t *out) {
  if (!c) return QP_ERR_ARG;
  const uint32_t G = group_size(op, param);
  if (!G) { c->err = "qp_debug_field_op: unknown op or parameter"; return QP_ERR_ARG; }
  if (n % G) { c->err = "qp_debug_field_op: n is not a multiple of the op's group size"; return QP_ERR_ARG; }
  if (n > ((uint64_t)1 << 28)) { c->err = "qp_debug_field_op: more than 2^28 elements"; return QP_ERR_ARG; }
  if (!n) return QP_OK;
  if (!a || !out || (!b && !unary(op))) { c->err = "null argument"; return QP_ERR_ARG; }
  const uint64_t ngroups = n / G, nout = op == QP_FOP_ACC3 ? ngroups : n;
  DevBuf da, db, dout;  // db stays null for a unary op
  hipError_t e = hipSetDevice(c->device);
  if (!e) e = da.alloc(n);
  if (!e && b) e = db.alloc(n);
  if (!e) e = dout.alloc(nout);
  if (!e) e = hipMemcpyAsync(da.p, a, n * 8, hipMemcpyHostToDevice, c->stream);
  if (!e && b) e = hipMemcpyAsync(db.p, b, n * 8, hipMemcpyHostToDevice, c->stream);
  if (!e) {
    const dim3 grid((unsigned)std::min<uint64_t>((ngroups + 255) / 256, 1024));
    launch(op, grid, c->stream, da.p, db.p, ngroups, param, dout.p);
    e = hipGetLastError();
  }
  if (!e) e = hipMemcpyAsync(out, dout.p, nout * 8, hipMemcpyDeviceToHost, c->stream);
  if (!e) e = hipStreamSynchronize(c->stream);
  if (e) {
    c->err = std::string("qp_debug_field_op: ") + hipGetErrorString(e);
    return e == hipErrorOutOfMemory ? QP_ERR_OOM : QP_ERR_HIP;
  }
  return QP_OK;
}
