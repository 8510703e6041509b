// ballot_device.h — what the ballot box's kernel files share (ballot.hip's
// table, tally and log kernels, ballot_audit.hip's audit of a published log):
// the values of a slot word and of a flags byte, the field's modulus, and the
// block-wide predicate count.  Device code for blocks of 256 lanes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace qpk {

constexpr uint32_t BALLOT_EMPTY = 0xFFFFFFFFu;    // a slot that holds no seq
constexpr uint32_t BALLOT_NO_SLOT = 0xFFFFFFFFu;  // stay[] of a lane whose probe ran out (defensive)
constexpr uint8_t BALLOT_VOTE = 1, BALLOT_COUNTED = 2;  // the bits of a log entry's flags byte
constexpr uint64_t BALLOT_P = 0xFFFFFFFF00000001ull;    // the Goldilocks modulus: a felt is canonical below it

// adds N per-lane predicates over the block into N 64-bit counters: a wave
// ballot and popcount each, the waves' counts through LDS, one integer atomic
// per counter and block (integer sums are order-independent).  Every lane of
// the block calls it.
template <int N>
__device__ __forceinline__ void block_count(const bool (&pred)[N], unsigned long long *const (&dst)[N]) {
  __shared__ uint32_t sh[4][N];
  const uint32_t wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < N; j++) {
    const uint32_t n = __popcll(__ballot(pred[j]));
    if ((threadIdx.x & 63) == 0) sh[wave][j] = n;
  }
  __syncthreads();
  if (threadIdx.x < N) {
    const uint32_t t = sh[0][threadIdx.x] + sh[1][threadIdx.x] + sh[2][threadIdx.x] + sh[3][threadIdx.x];
    if (t) atomicAdd(dst[threadIdx.x], (unsigned long long)t);
  }
}

}  // namespace qpk
