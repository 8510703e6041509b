// poseidon_probe.hip — TEST-ONLY probe of the device Poseidon forms
// (qp_debug_poseidon_op, include/qpgpu.h).  Each state of 12 words goes through
// one of the forms the production kernels instantiate — pf:: whole
// permutations and their pieces (poseidon_fast.h), pc:: one-wave and 16-lane-row
// forms (poseidon_coop.h) — and comes back as 12 RAW words, not canonicalised,
// so tests/test_gpu_poseidon_forms.py sees the representation.  Nothing here
// restates the arithmetic: the headers are included, not copied.  Two pieces
// have no function of their own in the headers and are called the way their
// kernel calls them: round 0 of permute_nc_capz (8 S-boxes, capz_mds) and the
// witness's rolled partial round (S-box on lane 0, mds_rows_block_dyn).
#include "../../include/qpgpu.h"
#include <algorithm>
#include <string>
#include "ctx.h"
#include "poseidon.h"
#include "poseidon_coop.h"
#include "poseidon_fast.h"

namespace {

constexpr int MDS_NEXT = 27;  // the mds_block<NEXT> instance probed beside mds_block<-1>

bool wave_form(uint32_t f) { return f == QP_PFORM_COOP_PERMUTE || f == QP_PFORM_COOP_MDS; }
bool row_form(uint32_t f) { return f == QP_PFORM_ROW_PERMUTE || f == QP_PFORM_ROW_MDS; }
bool capz_form(uint32_t f) { return f == QP_PFORM_PERMUTE_CAPZ || f == QP_PFORM_CAPZ_ROUND0; }

bool param_ok(uint32_t form, uint32_t param) {
  switch (form) {
    case QP_PFORM_MDS_BLOCK: return param == 0 || param == MDS_NEXT;
    case QP_PFORM_MDS_K:
    case QP_PFORM_FULL_ROUND_DYN:
    case QP_PFORM_PARTIAL_DYN: return param >= 1 && param < (uint32_t)ps::ROUNDS;
    case QP_PFORM_PARTIAL_GROUP: return param <= 20 && param % pf::PF_GROUP == 0;
    case QP_PFORM_DENSE_GROUP: return param < 22 && pfd::GLEN[param] != 0;
    case QP_PFORM_DENSE_GROUP4: return param < 22 && pfd4::GLEN[param] != 0;
    default: return form < QP_PFORM_COUNT && !param;
  }
}

__device__ __forceinline__ void split(const uint64_t s[12], uint32_t lo[12], uint32_t hi[12]) {
#pragma unroll
  for (int i = 0; i < 12; i++) {
    lo[i] = pf::lo32(s[i]);
    hi[i] = pf::hi32(s[i]);
  }
}

// one state per lane.  P: the compile-time parameter of the form (NEXT of
// mds_block, T0 of partial_group and of dense_group over either table); param: the run-time one (the round whose
// constants the dyn forms and mds_k fold)
template <uint32_t FORM, int P>
__global__ void __launch_bounds__(256) k_poseidon_lane(const uint64_t *__restrict__ in, uint64_t nstates,
                                                       uint32_t param, uint64_t *__restrict__ out) {
  for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < nstates;
       g += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t s[12];
#pragma unroll
    for (int i = 0; i < 12; i++) s[i] = in[12 * g + i];
    if constexpr (FORM == QP_PFORM_PERMUTE_NC) {
      pf::permute_nc(s);
    } else if constexpr (FORM == QP_PFORM_PERMUTE_CAPZ) {
      pf::permute_nc_capz<0xFu>(s);
    } else if constexpr (FORM == QP_PFORM_ROUNDS1_L7) {
      pf::rounds<1, 0x80u>(s);
    } else if constexpr (FORM == QP_PFORM_MDS_BLOCK) {
      pf::mds_block<P>(s);
    } else if constexpr (FORM == QP_PFORM_MDS_K) {
      uint64_t k[12];
#pragma unroll
      for (int i = 0; i < 12; i++) k[i] = ps::RC_DEV[param * 12 + i];
      pf::mds_k(s, k);
    } else if constexpr (FORM == QP_PFORM_MDS_MADS) {
      pf::mds_mads(s);
    } else if constexpr (FORM == QP_PFORM_CAPZ_ROUND0) {
      uint32_t lo[12], hi[12];
#pragma unroll
      for (int i = 0; i < 8; i++) {
        s[i] = pf::sbox(pf::add_c(s[i], ps::rc_cx(i)));
        lo[i] = pf::lo32(s[i]);
        hi[i] = pf::hi32(s[i]);
      }
      pf::capz_mds(s, lo, hi);
    } else if constexpr (FORM == QP_PFORM_MDS_INIT_SPARSE) {
      pf::mds_init_sparse(s);
    } else if constexpr (FORM == QP_PFORM_PARTIAL_GROUP) {
      pf::partial_group<P, (22 - P) < pf::PF_GROUP ? (22 - P) : pf::PF_GROUP>(s);
    } else if constexpr (FORM == QP_PFORM_DENSE_GROUP) {
      pf::dense_group<P, pfd::GLEN[P]>(s);
    } else if constexpr (FORM == QP_PFORM_DENSE_GROUP4) {
      pf::dense_group<P, pfd4::GLEN[P], pf::TabG4>(s);
    } else if constexpr (FORM == QP_PFORM_FULL_ROUND_DYN) {
      pf::full_round_dyn(s, ps::RC_DEV + param * 12);
    } else {
      static_assert(FORM == QP_PFORM_PARTIAL_DYN, "one-lane form");
      s[0] = pf::sbox(s[0]);
      uint32_t lo[12], hi[12];
      split(s, lo, hi);
      pf::mds_rows_block_dyn<0>(s, lo, hi, ps::RC_DEV + param * 12);
    }
#pragma unroll
    for (int i = 0; i < 12; i++) out[12 * g + i] = s[i];
  }
}

// one state per 64-lane wave (4 per block) or per 16-lane row (16 per block):
// element i on lane i < 12 of the wave / row, the other lanes hold 0.  Blocks
// are always 256 lanes and a wave / row past nstates exits whole (as
// k_merkle_level_coop / k_merkle_level_row do), so pc::permute sees 64 active
// lanes and the row forms whole rows.
template <uint32_t FORM>
__global__ void __launch_bounds__(256) k_poseidon_coop(const uint64_t *__restrict__ in, uint64_t nstates,
                                                       uint64_t *__restrict__ out) {
  constexpr bool ROW = FORM == QP_PFORM_ROW_PERMUTE || FORM == QP_PFORM_ROW_MDS;
  const uint64_t st = ROW ? (uint64_t)blockIdx.x * 16 + (threadIdx.x >> 4) : (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & (ROW ? 15 : 63);
  if (st >= nstates) return;
  uint64_t x = lane < 12 ? in[12 * st + lane] : 0;
  if constexpr (FORM == QP_PFORM_COOP_PERMUTE) {
    x = pc::permute(x);
  } else if constexpr (FORM == QP_PFORM_ROW_PERMUTE) {
    x = pc::permute_row(x);
  } else {
    uint32_t coef[12];
    pc::mds_coef(lane < 12 ? lane : 0, coef);
    if constexpr (FORM == QP_PFORM_COOP_MDS) x = pc::wave_mds_row(x, coef);
    else x = pc::row_mds(x, coef);
  }
  if (lane < 12) out[12 * st + lane] = x;
}

template <uint32_t FORM, int P>
void lane_launch(dim3 grid, hipStream_t s, const uint64_t *in, uint64_t n, uint32_t param, uint64_t *out) {
  k_poseidon_lane<FORM, P><<<grid, 256, 0, s>>>(in, n, param, out);
}

template <int T0 = 0>
void group_launch(uint32_t t0, dim3 grid, hipStream_t s, const uint64_t *in, uint64_t n, uint64_t *out) {
  if constexpr (T0 < 22) {
    if (t0 == (uint32_t)T0) lane_launch<QP_PFORM_PARTIAL_GROUP, T0>(grid, s, in, n, 0, out);
    else group_launch<T0 + pf::PF_GROUP>(t0, grid, s, in, n, out);
  }
}

template <int T0 = 0>
void dense_launch(uint32_t t0, dim3 grid, hipStream_t s, const uint64_t *in, uint64_t n, uint64_t *out) {
  if constexpr (T0 < 22) {
    if (t0 == (uint32_t)T0) lane_launch<QP_PFORM_DENSE_GROUP, T0>(grid, s, in, n, 0, out);
    else dense_launch<T0 + pfd::GLEN[T0]>(t0, grid, s, in, n, out);
  }
}

template <int T0 = 0>
void dense4_launch(uint32_t t0, dim3 grid, hipStream_t s, const uint64_t *in, uint64_t n, uint64_t *out) {
  if constexpr (T0 < 22) {
    if (t0 == (uint32_t)T0) lane_launch<QP_PFORM_DENSE_GROUP4, T0>(grid, s, in, n, 0, out);
    else dense4_launch<T0 + pfd4::GLEN[T0]>(t0, grid, s, in, n, out);
  }
}

void launch(uint32_t form, uint32_t param, hipStream_t s, const uint64_t *in, uint64_t n, uint64_t *out) {
  if (wave_form(form) || row_form(form)) {
    const dim3 grid((unsigned)((n + (row_form(form) ? 15 : 3)) / (row_form(form) ? 16 : 4)));
    switch (form) {
      case QP_PFORM_COOP_PERMUTE: k_poseidon_coop<QP_PFORM_COOP_PERMUTE><<<grid, 256, 0, s>>>(in, n, out); break;
      case QP_PFORM_ROW_PERMUTE: k_poseidon_coop<QP_PFORM_ROW_PERMUTE><<<grid, 256, 0, s>>>(in, n, out); break;
      case QP_PFORM_COOP_MDS: k_poseidon_coop<QP_PFORM_COOP_MDS><<<grid, 256, 0, s>>>(in, n, out); break;
      default: k_poseidon_coop<QP_PFORM_ROW_MDS><<<grid, 256, 0, s>>>(in, n, out); break;
    }
    return;
  }
  const dim3 grid((unsigned)std::min<uint64_t>((n + 255) / 256, 1024));
  switch (form) {
    case QP_PFORM_PERMUTE_NC: lane_launch<QP_PFORM_PERMUTE_NC, 0>(grid, s, in, n, param, out); break;
    case QP_PFORM_PERMUTE_CAPZ: lane_launch<QP_PFORM_PERMUTE_CAPZ, 0>(grid, s, in, n, param, out); break;
    case QP_PFORM_ROUNDS1_L7: lane_launch<QP_PFORM_ROUNDS1_L7, 0>(grid, s, in, n, param, out); break;
    case QP_PFORM_MDS_BLOCK:
      if (param) lane_launch<QP_PFORM_MDS_BLOCK, MDS_NEXT>(grid, s, in, n, param, out);
      else lane_launch<QP_PFORM_MDS_BLOCK, -1>(grid, s, in, n, param, out);
      break;
    case QP_PFORM_MDS_K: lane_launch<QP_PFORM_MDS_K, 0>(grid, s, in, n, param, out); break;
    case QP_PFORM_MDS_MADS: lane_launch<QP_PFORM_MDS_MADS, 0>(grid, s, in, n, param, out); break;
    case QP_PFORM_CAPZ_ROUND0: lane_launch<QP_PFORM_CAPZ_ROUND0, 0>(grid, s, in, n, param, out); break;
    case QP_PFORM_MDS_INIT_SPARSE: lane_launch<QP_PFORM_MDS_INIT_SPARSE, 0>(grid, s, in, n, param, out); break;
    case QP_PFORM_PARTIAL_GROUP: group_launch(param, grid, s, in, n, out); break;
    case QP_PFORM_DENSE_GROUP: dense_launch(param, grid, s, in, n, out); break;
    case QP_PFORM_DENSE_GROUP4: dense4_launch(param, grid, s, in, n, out); break;
    case QP_PFORM_FULL_ROUND_DYN: lane_launch<QP_PFORM_FULL_ROUND_DYN, 0>(grid, s, in, n, param, out); break;
    default: lane_launch<QP_PFORM_PARTIAL_DYN, 0>(grid, s, in, n, param, out); break;
  }
}

}  // namespace

extern "C" int qp_debug_poseidon_op(qp_ctx *c, uint32_t form, uint32_t param, const uint64_t *states,
                                    uint64_t nstates, uint64_t *out) {
  if (!c) return QP_ERR_ARG;
  if (!param_ok(form, param)) { c->err = "qp_debug_poseidon_op: unknown form or parameter"; return QP_ERR_ARG; }
  if (nstates > ((uint64_t)1 << 20)) { c->err = "qp_debug_poseidon_op: more than 2^20 states"; return QP_ERR_ARG; }
  if (!nstates) return QP_OK;
  if (!states || !out) { c->err = "null argument"; return QP_ERR_ARG; }
  if (capz_form(form))
    for (uint64_t i = 0; i < nstates; i++)
      if (states[12 * i + 8] | states[12 * i + 9] | states[12 * i + 10] | states[12 * i + 11]) {
        c->err = "qp_debug_poseidon_op: lanes 8..11 of a capz state must be 0";
        return QP_ERR_ARG;
      }
  const uint64_t n = nstates * 12;
  DevBuf din, dout;
  hipError_t e = hipSetDevice(c->device);
  if (!e) e = din.alloc(n);
  if (!e) e = dout.alloc(n);
  if (!e) e = hipMemcpyAsync(din.p, states, n * 8, hipMemcpyHostToDevice, c->stream);
  if (!e) {
    launch(form, param, c->stream, din.p, nstates, dout.p);
    e = hipGetLastError();
  }
  if (!e) e = hipMemcpyAsync(out, dout.p, n * 8, hipMemcpyDeviceToHost, c->stream);
  if (!e) e = hipStreamSynchronize(c->stream);
  if (e) {
    c->err = std::string("qp_debug_poseidon_op: ") + hipGetErrorString(e);
    return e == hipErrorOutOfMemory ? QP_ERR_OOM : QP_ERR_HIP;
  }
  return QP_OK;
}
