// verifier.hip — the verifier's query rounds on gfx950 (plonky2
// fri/verifier.rs fri_verifier_query_round over a batch of proofs) and
// qp_merkle_verify.  VALU-bound like the prover's hashing kernels: one lane
// per Merkle path with the 12-element state in registers (the leaf's sponge,
// then one two_to_one per sibling), one lane per query for the arithmetic.
// Each lane reads its own row of the repacked arrays (aligned 64-bit loads).
#include "../../include/qpgpu.h"
#include "ctx.h"
#include "poseidon_dev.h"
#include "verifier.h"

namespace qv {

struct DevHash {
  static __device__ __forceinline__ void permute(uint64_t s[12]) { psd::permute_nc(s); }
  static __device__ __forceinline__ void node(uint64_t s[12]) { psd::permute_nc_node(s); }
};

__global__ void __launch_bounds__(256) k_verify_paths(const PathJob job) {
  uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= job.total) return;
  const uint32_t lane = t;
  uint32_t c = 0;
  while (c + 1 < job.ncls && t >= job.cls[c].n) t -= job.cls[c++].n;
  job.ok[lane] = path_ok<DevHash>(job.cls[c], job.cap_height, t) ? 1 : 0;
}

__global__ void __launch_bounds__(256) k_verify_fri(const FriJob job) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= job.n) return;
  job.code[t] = fri_query(job, t);
}

void launch_paths(const PathJob &job, hipStream_t s) {
  if (!job.total) return;
  k_verify_paths<<<(job.total + 255) / 256, 256, 0, s>>>(job);
}

void launch_fri(const FriJob &job, hipStream_t s) {
  if (!job.n) return;
  k_verify_fri<<<(job.n + 255) / 256, 256, 0, s>>>(job);
}

}  // namespace qv

extern "C" int qp_merkle_verify(qp_ctx *c, const uint64_t *leaves, uint32_t width, const uint32_t *idx,
                                const uint64_t *siblings, uint32_t nsib, const uint64_t *cap, uint32_t cap_height,
                                uint32_t n, uint8_t *ok_out) {
  if (!c) return QP_ERR_ARG;
  if (!n) return QP_OK;
  if (!leaves || !idx || !cap || !ok_out || (nsib && !siblings) || !width || width > (1u << 20) || nsib > 32 ||
      cap_height > 20 || nsib + cap_height > 32) {
    c->err = "qp_merkle_verify: null argument or unsupported shape (width >= 1, nsib + cap_height <= 32)";
    return QP_ERR_ARG;
  }
  QP_HIP_TRY(c, hipSetDevice(c->device));
  const size_t lw = (size_t)n * width, sw = (size_t)n * nsib * 4, cw = (size_t)4 << cap_height;
  const size_t words = lw + sw + cw + (n + 1) / 2;
  DevBuf buf, ok;
  hipError_t e = buf.alloc(words);
  if (!e) e = ok.alloc(((size_t)n + 7) / 8);  // one byte per path
  uint64_t *const d = buf.p;
  uint8_t *const d_ok = ok.as<uint8_t>();
  if (!e) e = hipMemcpyAsync(d, leaves, lw * 8, hipMemcpyHostToDevice, c->stream);
  if (!e && sw) e = hipMemcpyAsync(d + lw, siblings, sw * 8, hipMemcpyHostToDevice, c->stream);
  if (!e) e = hipMemcpyAsync(d + lw + sw, cap, cw * 8, hipMemcpyHostToDevice, c->stream);
  if (!e) e = hipMemcpyAsync(d + lw + sw + cw, idx, (size_t)n * 4, hipMemcpyHostToDevice, c->stream);
  if (!e) {
    qv::PathJob job{};
    job.cls[0] = qv::PathClass{d, d + lw, (const uint32_t *)(d + lw + sw + cw), d + lw + sw, 0, width, nsib, 1, n};
    job.ncls = 1;
    job.cap_height = cap_height;
    job.total = n;
    job.ok = d_ok;
    qv::launch_paths(job, c->stream);
    e = hipGetLastError();
  }
  if (!e) e = hipMemcpyAsync(ok_out, d_ok, n, hipMemcpyDeviceToHost, c->stream);
  if (!e) e = hipStreamSynchronize(c->stream);
  QP_HIP_TRY(c, e);
  return QP_OK;
}
