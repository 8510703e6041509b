// claims.hip — the payout claims commitment on the device (gfx950;
// claims_kernels.h has the layouts, claims.h the definitions).  The leaves are
// VALU-bound: one lane per sorted position reads its record (36 bytes), follows
// astay[entry] to the view's slot, reads the four limb sums, normalises them
// and runs the two permutations of the 11-felt leaf in registers (the forms
// ledger.hip's log leaf uses).  The grand total and the gather are
// latency-bound reads.  Blocks of 256 lanes.  Every index a lane follows is
// compared with a count the host computed before it is used.
#include "claims_kernels.h"
#include "claims.h"
#include "poseidon_dev.h"
#include "slot_table_device.h"

namespace qpk {

namespace {
// the slot of the account that owns range entry `entry`, or NO_SLOT with *err set
__device__ __forceinline__ uint32_t owner_slot(const LedgerDev &v, uint32_t entry, uint32_t k, uint32_t *err) {
  if (entry >= k) {
    atomicOr(err, CLAIMS_ERR_ENTRY);
    return NO_SLOT;
  }
  const uint32_t at = v.astay[entry];
  if (at == NO_SLOT || (uint64_t)at > v.mask) {  // NO_SLOT: the entry was not credited (mask reaches 2^32 - 1 past 2^30 entries)
    atomicOr(err, CLAIMS_ERR_SLOT);
    return NO_SLOT;
  }
  return at;
}
}  // namespace

__global__ void __launch_bounds__(256) k_claims_leaves(NsetRecs r, uint32_t a, LedgerDev v, uint32_t k, uint64_t m0,
                                                       uint32_t *__restrict__ totals, uint64_t *__restrict__ dig,
                                                       uint32_t *__restrict__ err) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= a) return;
  const uint32_t entry = r.seq[j];
  const uint32_t at = owner_slot(v, entry, k, err);
  if (at == NO_SLOT) return;
  uint64_t sums[4];
  load_key(reinterpret_cast<const uint64_t *>(v.sum) + (uint64_t)at * 4, sums);
  uint32_t t[5];
  qcl::normalise(sums, t);
#pragma unroll
  for (int i = 0; i < 5; i++) totals[(uint64_t)j * 5 + i] = t[i];
  uint64_t s[12];
  load_key(r.key + (uint64_t)j * 4, s);
#pragma unroll
  for (int i = 0; i < 4; i++) s[4 + i] = t[i];
  s[8] = s[9] = s[10] = s[11] = 0;
  pf::permute_nc_capz<0xFFFu>(s);
  s[0] = t[4];
  s[1] = m0 + entry;
  s[2] = qcl::LEAF_TAG;
#pragma unroll
  for (int i = 0; i < 12; i++) s[i] = pf::add_c(s[i], ps::rc_cx(i));
  pf::rounds<0, 0xFu>(s);
  ulonglong2 *o = reinterpret_cast<ulonglong2 *>(dig + (uint64_t)j * 4);
  o[0] = make_ulonglong2(psd::canon(s[0]), psd::canon(s[1]));
  o[1] = make_ulonglong2(psd::canon(s[2]), psd::canon(s[3]));
}

// A block's limb sums in LDS, then one integer atomic per block and limb (integer addition is
// order-free).  A 64-bit word holds every partial sum: the rows of a range own disjoint sets of its
// credited entries, so any sum of distinct rows' limb-i sums is at most the sum of limb i over all
// credited entries of the range, at most 2^31 (2^32 - 1) < 2^63 (DESIGN §17 has the derivation).
__global__ void __launch_bounds__(256) k_claims_total(const uint32_t *__restrict__ entry, uint32_t a, LedgerDev v,
                                                      uint32_t k, unsigned long long *__restrict__ out,
                                                      uint32_t *__restrict__ err) {
  __shared__ unsigned long long sh[4][256];
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  uint64_t sums[4] = {0, 0, 0, 0};
  if (j < a) {
    const uint32_t at = owner_slot(v, entry[j], k, err);
    if (at != NO_SLOT) load_key(reinterpret_cast<const uint64_t *>(v.sum) + (uint64_t)at * 4, sums);
  }
#pragma unroll
  for (int i = 0; i < 4; i++) sh[i][threadIdx.x] = sums[i];
  __syncthreads();
  for (uint32_t off = 128; off; off >>= 1) {
    if (threadIdx.x < off)
#pragma unroll
      for (int i = 0; i < 4; i++) sh[i][threadIdx.x] += sh[i][threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x < 4 && sh[threadIdx.x][0]) atomicAdd(out + threadIdx.x, sh[threadIdx.x][0]);
}

__global__ void __launch_bounds__(256) k_claims_gather_totals(const uint32_t *__restrict__ totals,
                                                              const uint64_t *__restrict__ idx, uint32_t n,
                                                              uint32_t *__restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t j = idx[i];
#pragma unroll
  for (int f = 0; f < 5; f++) out[(uint64_t)i * 5 + f] = totals[j * 5 + f];
}

void claims_leaves(const NsetRecs &recs, uint32_t a, const LedgerDev &v, uint32_t k, uint64_t m0, uint32_t *totals,
                   uint64_t *dig, uint32_t *err, hipStream_t s) {
  if (a) k_claims_leaves<<<ledger_blocks(a), LEDGER_BLOCK, 0, s>>>(recs, a, v, k, m0, totals, dig, err);
}

void claims_total(const uint32_t *entry, uint32_t a, const LedgerDev &v, uint32_t k, unsigned long long *out,
                  uint32_t *err, hipStream_t s) {
  if (a) k_claims_total<<<ledger_blocks(a), LEDGER_BLOCK, 0, s>>>(entry, a, v, k, out, err);
}

void claims_gather_totals(const uint32_t *totals, const uint64_t *idx, uint32_t n, uint32_t *out, hipStream_t s) {
  if (n) k_claims_gather_totals<<<ledger_blocks(n), LEDGER_BLOCK, 0, s>>>(totals, idx, n, out);
}

}  // namespace qpk
