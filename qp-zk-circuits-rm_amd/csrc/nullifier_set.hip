// nullifier_set.hip — the sorted nullifier set of a log on the device (gfx950;
// nullifier_set_kernels.h has the layouts and the form of the sort,
// nullifier_set.h the definitions).  The select is the payouts' compaction
// (count per block, scan, write).  The tile sort is LDS-bound: 55 bitonic steps
// over 1024 records, each lane two compare-exchanges per step.  A merge pass is
// latency-bound: per output element a binary search of at most 32 dependent
// pairs of 32-byte key reads, then one coalesced 36-byte write.  The leaves are
// VALU-bound, one permutation per lane (merkle_node.h).  Blocks of 256 lanes.
#include "nullifier_set_kernels.h"
#include "ledger_kernels.h"
#include "merkle_node.h"
#include "nullifier_set.h"
#include "slot_table_device.h"

namespace qpk {

namespace {
__device__ __forceinline__ void store_key(uint64_t *p, const uint64_t k[4]) {
  reinterpret_cast<ulonglong2 *>(p)[0] = make_ulonglong2(k[0], k[1]);
  reinterpret_cast<ulonglong2 *>(p)[1] = make_ulonglong2(k[2], k[3]);
}
}  // namespace

__global__ void __launch_bounds__(256) k_nset_select_count(const uint8_t *__restrict__ flags, uint32_t n, uint8_t mask,
                                                           uint32_t *__restrict__ blk) {
  const uint32_t seq = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t total;
  block_rank(seq < n && (flags[seq] & mask), &total);
  if (threadIdx.x == 0) blk[blockIdx.x] = total;
}

__global__ void __launch_bounds__(256) k_nset_select_write(const uint8_t *__restrict__ flags, uint32_t n, uint8_t mask,
                                                           const uint32_t *__restrict__ blk,
                                                           uint32_t *__restrict__ sel) {
  const uint32_t seq = blockIdx.x * blockDim.x + threadIdx.x;
  const bool member = seq < n && (flags[seq] & mask);
  uint32_t total;
  const uint32_t rank = block_rank(member, &total);
  if (member) sel[blk[blockIdx.x] + rank] = seq;  // below the members' count <= n: the caller sized sel[] for n
}

// One tile per workgroup, the records in LDS as five columns (a lane's 8-byte and 4-byte accesses at
// consecutive indices are conflict-free).  Positions past m hold the padding record (all-ones key,
// seq 0xFFFFFFFF), which the order puts after every record of a log (a seq is below 2^31), so the
// tile's own records end up in front and only they are written out.  Compare-exchange t of a step
// with distance j touches i = t with a zero bit inserted at j, and i | j; ascending where (i & k2)
// is zero.  Equal records (padding only) are never swapped.
__global__ void __launch_bounds__(256) k_nset_tile_sort(const uint64_t *__restrict__ nullifier,
                                                        const uint32_t *__restrict__ sel, uint32_t m, NsetRecs out) {
  __shared__ uint64_t sk[4][NSET_TILE];
  __shared__ uint32_t ss[NSET_TILE];
  const uint32_t base = blockIdx.x * NSET_TILE;
  for (uint32_t i = threadIdx.x; i < NSET_TILE; i += 256) {
    uint64_t k[4] = {~0ull, ~0ull, ~0ull, ~0ull};
    uint32_t seq = NSET_NO_SEQ;
    if (base + i < m) {
      seq = sel[base + i];
      load_key(nullifier + (uint64_t)seq * 4, k);
    }
#pragma unroll
    for (int f = 0; f < 4; f++) sk[f][i] = k[f];
    ss[i] = seq;
  }
  __syncthreads();
  for (uint32_t k2 = 2; k2 <= NSET_TILE; k2 <<= 1)
    for (uint32_t j = k2 >> 1; j; j >>= 1) {
#pragma unroll
      for (uint32_t t = threadIdx.x; t < NSET_TILE / 2; t += 256) {
        const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
        uint64_t a[4], b[4];
#pragma unroll
        for (int f = 0; f < 4; f++) a[f] = sk[f][i], b[f] = sk[f][p];
        const uint32_t sa = ss[i], sb = ss[p];
        const bool up = !(i & k2);
        if (up ? qns::rec_less(b, sb, a, sa) : qns::rec_less(a, sa, b, sb)) {
#pragma unroll
          for (int f = 0; f < 4; f++) sk[f][i] = b[f], sk[f][p] = a[f];
          ss[i] = sb, ss[p] = sa;
        }
      }
      __syncthreads();
    }
  for (uint32_t i = threadIdx.x; i < NSET_TILE && base + i < m; i += 256) {
    uint64_t k[4];
#pragma unroll
    for (int f = 0; f < 4; f++) k[f] = sk[f][i];
    store_key(out.key + (uint64_t)(base + i) * 4, k);
    out.seq[base + i] = ss[i];
  }
}

// One lane per output element i < m.  Its pair of runs starts at s0 = (i / 2 run) 2 run: A = [s0, s0 +
// la), B = [s0 + run, s0 + run + lb), la = min(run, m - s0) >= 1, lb = what is left of run records
// past A (0: the unpaired last run, copied).  d = i - s0 outputs precede element i; a = the number of
// them that come from A is the least a in [max(0, d - lb), min(d, la)] with A[a] > B[d - a - 1] (or
// the upper end): the search reads A[mid], mid < min(d, la), and B[d - mid - 1], 0 <= d - mid - 1 <
// lb, and halves at most 32 times.  Element i is the smaller of A[a] and B[d - a] where both exist.
__global__ void __launch_bounds__(256) k_nset_merge(NsetRecs src, NsetRecs dst, uint32_t m, uint32_t run) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const uint32_t s0 = i / (2 * run) * (2 * run), d = i - s0;
  const uint32_t la = min(run, m - s0), lb = la < run ? 0 : min(run, m - s0 - run);
  uint32_t from = i;
  if (lb) {
    const uint64_t *ka = src.key + (uint64_t)s0 * 4, *kb = src.key + (uint64_t)(s0 + run) * 4;
    const uint32_t *sa = src.seq + s0, *sb = src.seq + s0 + run;
    uint32_t lo = d > lb ? d - lb : 0, hi = min(d, la);
    for (int it = 0; it < 32 && lo < hi; it++) {
      const uint32_t mid = lo + (hi - lo) / 2, b = d - mid - 1;
      uint64_t x[4], y[4];
      load_key(ka + (uint64_t)mid * 4, x);
      load_key(kb + (uint64_t)b * 4, y);
      if (qns::rec_less(x, sa[mid], y, sb[b])) lo = mid + 1;
      else hi = mid;
    }
    const uint32_t a = lo, b = d - lo;  // a <= la, b <= lb, a + b = d < la + lb: one of them is inside its run
    bool take_a = b >= lb;
    if (a < la && b < lb) {
      uint64_t x[4], y[4];
      load_key(ka + (uint64_t)a * 4, x);
      load_key(kb + (uint64_t)b * 4, y);
      take_a = qns::rec_less(x, sa[a], y, sb[b]);
    }
    from = take_a ? s0 + a : s0 + run + b;
  }
  uint64_t k[4];
  load_key(src.key + (uint64_t)from * 4, k);
  store_key(dst.key + (uint64_t)i * 4, k);
  dst.seq[i] = src.seq[from];
}

// sorted records: position j >= 1 whose predecessor has an equal key is a duplicate member; equal keys
// lie in seq order, so it is never the lowest seq of its key.  A log of a handle has none; one
// integer atomic per offender (the minimum does not depend on the order they arrive in).
__global__ void __launch_bounds__(256) k_nset_duplicates(NsetRecs r, uint32_t m, uint32_t *__restrict__ dup) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j == 0 || j >= m) return;
  uint64_t a[4], b[4];
  load_key(r.key + (uint64_t)(j - 1) * 4, a);
  load_key(r.key + (uint64_t)j * 4, b);
  if (qst::key_equal(a, b)) atomicMin(dup, r.seq[j]);
}

// set leaf j = hash_no_pad([K_j[0..4], seq_j, 2]) into level 0 of the digest buffer, one lane per position
__global__ void __launch_bounds__(256) k_nset_leaves(NsetRecs r, uint32_t m, uint64_t *__restrict__ dig) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  uint64_t s[12];
  load_key(r.key + (uint64_t)j * 4, s);
  s[4] = r.seq[j];
  s[5] = qns::LEAF_TAG;
  s[6] = s[7] = 0;
  node_digest(s);
  store_key(dig + (uint64_t)j * 4, s);
}

// one lane per query key: the lower bound over the sorted keys (qns::lower_bound: at most 32 halvings)
__global__ void __launch_bounds__(256) k_nset_search(NsetRecs r, uint32_t m, const uint64_t *__restrict__ q, uint32_t k,
                                                     uint32_t *__restrict__ pos, uint32_t *__restrict__ found) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= k) return;
  uint64_t x[4];
  load_key(q + (uint64_t)i * 4, x);
  const uint32_t at = (uint32_t)qns::lower_bound(r.key, m, x);
  pos[i] = at;
  found[i] = at < m && qst::key_equal(r.key + (uint64_t)at * 4, x);
}

__global__ void __launch_bounds__(256) k_nset_gather(NsetRecs r, const uint64_t *__restrict__ idx, uint32_t k,
                                                     uint64_t *__restrict__ key_out, uint64_t *__restrict__ seq_out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= k) return;
  const uint64_t j = idx[i];
  uint64_t x[4];
  load_key(r.key + j * 4, x);
  store_key(key_out + (uint64_t)i * 4, x);
  seq_out[i] = r.seq[j];
}

static unsigned nset_blocks(uint64_t n) { return (unsigned)((n + 255) / 256); }

void nset_select_count(const uint8_t *flags, uint32_t n, uint8_t mask, uint32_t *blk, hipStream_t s) {
  if (n) k_nset_select_count<<<ledger_blocks(n), LEDGER_BLOCK, 0, s>>>(flags, n, mask, blk);
}

void nset_select_write(const uint8_t *flags, uint32_t n, uint8_t mask, const uint32_t *blk, uint32_t *sel,
                       hipStream_t s) {
  if (n) k_nset_select_write<<<ledger_blocks(n), LEDGER_BLOCK, 0, s>>>(flags, n, mask, blk, sel);
}

void nset_tile_sort(const uint64_t *nullifier, const uint32_t *sel, uint32_t m, const NsetRecs &out, hipStream_t s) {
  if (m) k_nset_tile_sort<<<(m + NSET_TILE - 1) / NSET_TILE, 256, 0, s>>>(nullifier, sel, m, out);
}

void nset_merge(const NsetRecs &src, const NsetRecs &dst, uint32_t m, uint32_t run, hipStream_t s) {
  if (m) k_nset_merge<<<nset_blocks(m), 256, 0, s>>>(src, dst, m, run);
}

void nset_duplicates(const NsetRecs &recs, uint32_t m, uint32_t *dup, hipStream_t s) {
  if (m > 1) k_nset_duplicates<<<nset_blocks(m), 256, 0, s>>>(recs, m, dup);
}

void nset_leaves(const NsetRecs &recs, uint32_t m, uint64_t *dig, hipStream_t s) {
  if (m) k_nset_leaves<<<nset_blocks(m), 256, 0, s>>>(recs, m, dig);
}

void nset_search(const NsetRecs &recs, uint32_t m, const uint64_t *q, uint32_t k, uint32_t *pos, uint32_t *found,
                 hipStream_t s) {
  if (k) k_nset_search<<<nset_blocks(k), 256, 0, s>>>(recs, m, q, k, pos, found);
}

void nset_gather(const NsetRecs &recs, const uint64_t *idx, uint32_t k, uint64_t *key_out, uint64_t *seq_out,
                 hipStream_t s) {
  if (k) k_nset_gather<<<nset_blocks(k), 256, 0, s>>>(recs, idx, k, key_out, seq_out);
}

}  // namespace qpk
