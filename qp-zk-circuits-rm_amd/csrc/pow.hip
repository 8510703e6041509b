// pow.hip — fri_proof_of_work on gfx950: the
// minimal witness of every proof of a batch, one launch (k_pow_scan).
#include "poseidon.h"
#include "poseidon_dev.h"
#include "prover_kernels.h"
#include <algorithm>

namespace qpk {

// Minimal witness, one launch for all proofs.  Candidates of proof b are
// claimed in blocks of 256 from a per-proof counter (next[b], increasing), so
// every block below the best hit is claimed while that hit is still unknown
// and gets tested: the final found[b] is the minimal witness.  A workgroup
// keeps claiming blocks of one proof until the claimed block starts at or
// above found[b] (or at limit), then moves to the next proof, so the stragglers
// of the geometric search get every workgroup of the grid.  limit bounds every
// loop (16 PoW bits: no hit below 2^36 has probability exp(-2^20)).
__device__ __forceinline__ bool pow_hit(const uint64_t *__restrict__ pre, uint32_t pos, uint64_t cand, uint32_t bits) {
  const uint64_t y = pf::sbox(pf::add_c(cand, ps::RC_DEV[pos]));
  const uint32_t y0 = pf::lo32(y), y1 = pf::hi32(y);
  uint64_t s[12];
#pragma unroll
  for (int r = 0; r < 12; r++) {
    const uint32_t c = (uint32_t)pre[12 + r];
    s[r] = pf::reduce_row((uint64_t)y0 * c + (pre[r] & pf::EPS), (uint64_t)y1 * c + (pre[r] >> 32));
  }
  pf::rounds<1, 0x80u>(s);  // only lane 7 is read
  return (psd::canon(s[7]) >> (64 - bits)) == 0;
}

// one candidate per thread per claimed block of 256 (2 or 4 per thread and
// per-wave claims measured no better: profiles/r05_ab_pow_cpt.log,
// r05_ab_pow_wave.log)
__global__ void __launch_bounds__(256) k_pow_scan(const uint64_t *__restrict__ states, const uint32_t *__restrict__ pos,
                                                  uint64_t *__restrict__ found, uint64_t *__restrict__ next, uint32_t nb,
                                                  uint32_t bits, uint64_t limit) {
  constexpr uint64_t BLK = 256;
  __shared__ uint64_t blk;
  __shared__ uint32_t done;
  for (uint32_t i = 0; i < nb; i++) {
    const uint32_t b = (blockIdx.x + i) % nb;
    const uint64_t *pre = states + b * 24;
    for (;;) {
      if (threadIdx.x == 0) {
        const uint64_t k = atomicAdd((unsigned long long *)(next + b), 1ull);
        blk = k;
        done = k * BLK >= limit || k * BLK >= *(const volatile uint64_t *)(found + b);
      }
      __syncthreads();
      const uint64_t k = blk;
      const uint32_t d = done;
      __syncthreads();  // every lane has read blk / done before lane 0 rewrites them
      if (d) break;
      const uint64_t cand = k * BLK + threadIdx.x;
      if (pow_hit(pre, pos[b], cand, bits)) atomicMin((unsigned long long *)(found + b), (unsigned long long)cand);
    }
  }
}

// 2048 workgroups claim 256-candidate blocks from per-proof counters, moving
// on to the next proof once theirs has a hit below the claimed block (per-wave
// claims and 2-4 candidates per thread measured no better:
// profiles/r05_ab_pow_wave.log, r05_ab_pow_cpt.log; a windowed loop with a
// host check per window was the round-1 form)
hipError_t pow_search(const uint64_t *states, const uint32_t *pos, uint64_t *found, uint64_t *next, uint32_t nb,
                      uint32_t bits, hipStream_t s) {
  hipError_t e = hipMemsetAsync(found, 0xFF, (size_t)nb * 8, s);
  if (!e) e = hipMemsetAsync(next, 0, (size_t)nb * 8, s);
  if (e) return e;
  const uint64_t limit = 1ull << std::min<uint32_t>(bits + 20, 62);
  k_pow_scan<<<2048, 256, 0, s>>>(states, pos, found, next, nb, bits, limit);
  return hipGetLastError();
}

}  // namespace qpk
