// ledger.hip — the transfer ledger on the device (gfx950): the screen of the
// public inputs, the stable pack of a batch's admitted transfers into the log,
// the nullifier table, the account table with its limb sums, the payouts'
// compaction and the read-only lookups.  Layouts and the home-slot rules:
// ledger_kernels.h.  Memory-latency-bound throughout: a lane reads 128 bytes of
// public inputs or does a few dependent slot atomics and 32-byte key reads.
// Blocks of 256 lanes (LEDGER_BLOCK).
#include "ballot_device.h"
#include "ledger_kernels.h"
#include "ledger_table.h"

namespace qpk {

namespace {
constexpr uint32_t LEDGER_EMPTY = 0xFFFFFFFFu;    // a slot that holds no seq
constexpr uint32_t LEDGER_NO_SLOT = 0xFFFFFFFFu;  // stay[] / astay[] of a lane whose probe ran out (defensive)
constexpr uint8_t LEDGER_CREDITED = ql::FLAG_CREDITED;

// one table: slot words over keys[seq][4] that live in the log
struct SlotTable {
  const uint64_t *keys;
  uint32_t *slot;
  uint64_t mask;
};

__device__ __forceinline__ void load_key(const uint64_t *p, uint64_t k[4]) {
  const ulonglong2 a = reinterpret_cast<const ulonglong2 *>(p)[0], b = reinterpret_cast<const ulonglong2 *>(p)[1];
  k[0] = a.x, k[1] = a.y, k[2] = b.x, k[3] = b.y;
}

// The probe of log entry seq's key (only seqs below `limit` are ever stored): returns the slot
// where it stays, LEDGER_NO_SLOT if S slots were tried; *claimed = this lane took an empty slot.
// It is the ballot box's probe (ballot.hip) over either table, and that file's facts 1-4 carry over
// word for word with "nullifier" read as "key":
// 1. A claimed slot's key never changes: the only later write is an atomicMin by a lane whose own
//    key equals the slot entry's, so all entries of one key stop at one slot whatever the
//    interleaving, and the word ends at the minimum of their seqs.  seq is monotone in the
//    transfer number (the pack is stable), so that is the lowest number.
// 2. The keys compared against were written by k_ledger_pack, a launch before this one; of what a
//    lane of the same launch writes only the slot word is read, and only through agent-scope
//    atomics.  No fences, no flags, no spinning.
// 3. count + k <= C <= S / 2 (the host checks before it launches), so an empty slot ends the loop;
//    it is bounded by S all the same, and running out sets the error word.
// 4. The lookups take no atomics and run in launches of their own after everything that writes.
__device__ __forceinline__ uint32_t table_probe(const SlotTable &t, uint32_t seq, uint32_t limit, bool *claimed) {
  uint64_t k[4];
  load_key(t.keys + (uint64_t)seq * 4, k);
  *claimed = false;
  uint64_t at = k[0] & t.mask;
  for (uint64_t tried = 0; tried <= t.mask; tried++, at = (at + 1) & t.mask) {
    uint32_t cur = __hip_atomic_load(t.slot + at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == LEDGER_EMPTY) {
      cur = atomicCAS(t.slot + at, LEDGER_EMPTY, seq);
      if (cur == LEDGER_EMPTY) {
        *claimed = true;
        return (uint32_t)at;
      }
    }
    if (cur == seq) return (uint32_t)at;
    if (cur >= limit) break;  // not a log entry: cannot be reached
    uint64_t o[4];
    load_key(t.keys + (uint64_t)cur * 4, o);  // cur < limit <= C, written before the launch
    if (ql::key_equal(o, k)) {
      atomicMin(t.slot + at, seq);
      return (uint32_t)at;
    }
  }
  return LEDGER_NO_SLOT;
}

// the read-only probe (fact 4) of key k in a table whose log holds `count` entries: the slot that
// holds an entry with that key, or LEDGER_NO_SLOT; a slot word at or beyond count sets *bad
__device__ __forceinline__ uint32_t table_lookup(const SlotTable &t, const uint64_t k[4], uint32_t count, bool *bad) {
  uint64_t at = k[0] & t.mask;
  for (uint64_t tried = 0; tried <= t.mask; tried++, at = (at + 1) & t.mask) {
    const uint32_t cur = t.slot[at];
    if (cur == LEDGER_EMPTY) break;
    if (cur >= count) {
      *bad = true;
      break;
    }
    uint64_t o[4];
    load_key(t.keys + (uint64_t)cur * 4, o);
    if (ql::key_equal(o, k)) return (uint32_t)at;
  }
  return LEDGER_NO_SLOT;
}

__device__ __forceinline__ SlotTable nullifier_table(const LedgerDev &d) { return {d.nullifier, d.nslot, d.mask}; }
__device__ __forceinline__ SlotTable account_table(const LedgerDev &d) { return {d.account, d.aslot, d.mask}; }

// the lane's rank among the block's lanes with pred, in lane order; *total = how many there are.
// Every lane of the block calls it, once per kernel.
__device__ __forceinline__ uint32_t block_rank(bool pred, uint32_t *total) {
  __shared__ uint32_t wave_n[4];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long b = __ballot(pred);
  if (lane == 0) wave_n[wave] = __popcll(b);
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (uint32_t w = 0; w < 4; w++) {
    const uint32_t n = wave_n[w];
    all += n;
    before += w < wave ? n : 0;
  }
  *total = all;
  return before + __popcll(b & ((1ull << lane) - 1));
}

// a credited entry into the account table, its limbs onto the account's sums.  The sums are indexed
// by the slot the key stays at, which fact 1 fixes for the key whatever the interleaving; integer
// addition commutes, so the sums are exact in any order.  Nothing reads a sum in this launch.
__device__ __forceinline__ bool credit_entry(const LedgerDev &d, uint32_t seq, uint32_t limit, bool *claimed) {
  const uint32_t at = table_probe(account_table(d), seq, limit, claimed);
  d.astay[seq] = at;
  if (at == LEDGER_NO_SLOT) return false;
  const uint4 a = reinterpret_cast<const uint4 *>(d.amount)[seq];
  unsigned long long *s = d.sum + (uint64_t)at * 4;
  atomicAdd(s + 0, (unsigned long long)a.x);
  atomicAdd(s + 1, (unsigned long long)a.y);
  atomicAdd(s + 2, (unsigned long long)a.z);
  atomicAdd(s + 3, (unsigned long long)a.w);
  return true;
}

__device__ __forceinline__ bool owns_account(const LedgerDev &d, uint32_t seq) {
  if (!(d.flags[seq] & LEDGER_CREDITED)) return false;
  const uint32_t at = d.astay[seq];
  return at != LEDGER_NO_SLOT && d.aslot[at] == seq;
}
}  // namespace

// one lane per transfer: the five checks, the result, the block's admitted count
__global__ void __launch_bounds__(256) k_ledger_screen(LedgerScreen sc, const uint64_t *__restrict__ pis,
                                                       const uint32_t *__restrict__ verdicts, uint32_t n,
                                                       uint64_t first_number, LedgerResult *__restrict__ res,
                                                       uint32_t *__restrict__ blk) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  bool admitted = false;
  if (i < n) {
    uint64_t pi[16];
    const ulonglong2 *src = reinterpret_cast<const ulonglong2 *>(pis + (uint64_t)i * 16);
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const ulonglong2 v = src[j];
      pi[2 * j] = v.x, pi[2 * j + 1] = v.y;
    }
    const uint32_t verdict = verdicts ? verdicts[i] : 0;
    const uint32_t st = ql::screen_check(pi, verdict, sc.roots, sc.nroots, sc.has_padding ? sc.padding : nullptr);
    const uint64_t num = first_number + i;
    res[i] = LedgerResult{st, verdict, num, num};
    admitted = st == ql::CREDITED;
  }
  uint32_t total;
  block_rank(admitted, &total);
  if (threadIdx.x == 0) blk[blockIdx.x] = total;
}

// one block: blk[nb] to exclusive prefix sums, a contiguous run per lane, the lanes' runs through LDS
__global__ void __launch_bounds__(256) k_ledger_scan(uint32_t *__restrict__ blk, uint32_t nb, uint32_t *total) {
  __shared__ uint32_t part[256];
  const uint32_t per = (nb + 255) / 256;
  const uint64_t lo = min((uint64_t)threadIdx.x * per, (uint64_t)nb), hi = min(lo + per, (uint64_t)nb);
  uint32_t mine = 0;
  for (uint64_t i = lo; i < hi; i++) mine += blk[i];
  part[threadIdx.x] = mine;
  __syncthreads();
  for (uint32_t off = 1; off < 256; off <<= 1) {
    const uint32_t v = threadIdx.x >= off ? part[threadIdx.x - off] : 0;
    __syncthreads();
    part[threadIdx.x] += v;
    __syncthreads();
  }
  uint32_t run = part[threadIdx.x] - mine;
  for (uint64_t i = lo; i < hi; i++) {
    const uint32_t v = blk[i];
    blk[i] = run;
    run += v;
  }
  if (threadIdx.x == 255) *total = part[255];
}

// one lane per transfer: an admitted one writes its log entry at first_seq + (admitted before it)
__global__ void __launch_bounds__(256) k_ledger_pack(LedgerDev d, const uint64_t *__restrict__ pis,
                                                     const LedgerResult *__restrict__ res,
                                                     const uint32_t *__restrict__ blk, uint32_t n, uint32_t first_seq,
                                                     uint32_t *__restrict__ pos) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool admitted = i < n && res[i].status == ql::CREDITED;
  uint32_t total;
  const uint32_t rank = block_rank(admitted, &total);
  if (!admitted) return;
  const uint32_t j = blk[blockIdx.x] + rank;
  const uint64_t seq = (uint64_t)first_seq + j;  // < first_seq + k <= C: the host checked k before this launch
  const ulonglong2 *src = reinterpret_cast<const ulonglong2 *>(pis + (uint64_t)i * 16);
  ulonglong2 *nul = reinterpret_cast<ulonglong2 *>(d.nullifier + seq * 4);
  ulonglong2 *acc = reinterpret_cast<ulonglong2 *>(d.account + seq * 4);
  nul[0] = src[ql::PI_NULLIFIER / 2], nul[1] = src[ql::PI_NULLIFIER / 2 + 1];
  acc[0] = src[ql::PI_ACCOUNT / 2], acc[1] = src[ql::PI_ACCOUNT / 2 + 1];
  const ulonglong2 hi = src[ql::PI_AMOUNT / 2], lo = src[ql::PI_AMOUNT / 2 + 1];
  reinterpret_cast<uint4 *>(d.amount)[seq] = make_uint4((uint32_t)hi.x, (uint32_t)hi.y, (uint32_t)lo.x, (uint32_t)lo.y);
  d.number[seq] = res[i].number;
  d.flags[seq] = 0;
  d.astay[seq] = LEDGER_NO_SLOT;
  pos[j] = i;
}

// one lane per admitted transfer of the batch
__global__ void __launch_bounds__(256) k_ledger_insert(LedgerDev d, uint32_t first_seq, uint32_t k,
                                                       uint32_t *__restrict__ stay, uint32_t *__restrict__ err) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= k) return;
  bool claimed;
  const uint32_t at = table_probe(nullifier_table(d), first_seq + j, first_seq + k, &claimed);
  stay[j] = at;
  if (at == LEDGER_NO_SLOT) atomicOr(err, 1u);
}

// a launch after the insert: every nullifier slot word is final.  One lane per admitted transfer of
// the batch; the lanes past k only take part in the block's counts.
__global__ void __launch_bounds__(256) k_ledger_resolve(LedgerDev d, uint32_t first_seq, uint32_t k,
                                                        const uint32_t *__restrict__ stay,
                                                        const uint32_t *__restrict__ pos, LedgerResult *res,
                                                        LedgerCounters *ctr) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  bool credited = false, claimed = false;
  if (j < k) {
    const uint32_t seq = first_seq + j, at = stay[j];
    const uint32_t owner = at == LEDGER_NO_SLOT ? LEDGER_EMPTY : d.nslot[at];
    LedgerResult *r = res + pos[j];
    if (owner > seq) {  // a slot holds the minimum of its nullifier's seqs: defensive, as the probe's bound
      atomicOr(&ctr->err, 2u);
      r->first = ~0ull;
    } else if (owner == seq) {
      d.flags[seq] = LEDGER_CREDITED;
      credited = true;
      if (!credit_entry(d, seq, first_seq + k, &claimed)) atomicOr(&ctr->err, 4u);
    } else {
      r->first = d.number[owner];
      r->status = ql::DOUBLE_SPEND;
    }
  }
  const bool pred[2] = {credited, claimed};
  unsigned long long *const dst[2] = {&ctr->credited, &ctr->accounts};
  block_count(pred, dst);
}

// reserve: the credited entries of the copied log into the new, empty tables.  Credited entries have
// distinct nullifiers, so each claims a nullifier slot; the account table and the sums as in a cast.
__global__ void __launch_bounds__(256) k_ledger_rebuild(LedgerDev d, uint32_t count, uint32_t *__restrict__ err) {
  const uint32_t seq = blockIdx.x * blockDim.x + threadIdx.x;
  if (seq >= count || !(d.flags[seq] & LEDGER_CREDITED)) return;
  bool claimed;
  if (table_probe(nullifier_table(d), seq, count, &claimed) == LEDGER_NO_SLOT) atomicOr(err, 1u);
  if (!credit_entry(d, seq, count, &claimed)) atomicOr(err, 4u);
}

// one lane per queried nullifier q[i][4]
__global__ void __launch_bounds__(256) k_ledger_find(LedgerDev d, uint32_t count, const uint64_t *__restrict__ q,
                                                     uint32_t k, uint32_t *__restrict__ seq_out,
                                                     uint32_t *__restrict__ err) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= k) return;
  uint64_t key[4];
  load_key(q + (uint64_t)i * 4, key);
  bool bad = false;
  const uint32_t at = table_lookup(nullifier_table(d), key, count, &bad);
  if (bad) atomicOr(err, 8u);
  seq_out[i] = at == LEDGER_NO_SLOT ? LEDGER_EMPTY : d.nslot[at];
}

// one lane per queried account q[i][4]
__global__ void __launch_bounds__(256) k_ledger_totals(LedgerDev d, uint32_t count, const uint64_t *__restrict__ q,
                                                       uint32_t k, unsigned long long *__restrict__ sums,
                                                       uint32_t *__restrict__ found, uint32_t *__restrict__ err) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= k) return;
  uint64_t key[4];
  load_key(q + (uint64_t)i * 4, key);
  bool bad = false;
  const uint32_t at = table_lookup(account_table(d), key, count, &bad);
  if (bad) atomicOr(err, 8u);
  found[i] = at != LEDGER_NO_SLOT;
#pragma unroll
  for (int j = 0; j < 4; j++) sums[(uint64_t)i * 4 + j] = at == LEDGER_NO_SLOT ? 0 : d.sum[(uint64_t)at * 4 + j];
}

// the payouts: the entries that own their account slot, compacted in log order (= the order of each
// account's first credited entry, with no sort): count per block, scan, write
__global__ void __launch_bounds__(256) k_ledger_payee_count(LedgerDev d, uint32_t count, uint32_t *__restrict__ blk) {
  const uint32_t seq = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t total;
  block_rank(seq < count && owns_account(d, seq), &total);
  if (threadIdx.x == 0) blk[blockIdx.x] = total;
}

__global__ void __launch_bounds__(256) k_ledger_payee_write(LedgerDev d, uint32_t count,
                                                            const uint32_t *__restrict__ blk,
                                                            uint32_t *__restrict__ payee) {
  const uint32_t seq = blockIdx.x * blockDim.x + threadIdx.x;
  const bool owns = seq < count && owns_account(d, seq);
  uint32_t total;
  const uint32_t rank = block_rank(owns, &total);
  if (owns) payee[blk[blockIdx.x] + rank] = seq;  // below the accounts' count <= count: the caller sized payee[] for count
}

__global__ void __launch_bounds__(256) k_ledger_payouts(LedgerDev d, const uint32_t *__restrict__ payee, uint32_t k,
                                                        uint64_t *__restrict__ accounts,
                                                        unsigned long long *__restrict__ sums,
                                                        uint64_t *__restrict__ first_seq) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= k) return;
  const uint32_t seq = payee[i];
  const uint64_t at = d.astay[seq];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    accounts[(uint64_t)i * 4 + j] = d.account[(uint64_t)seq * 4 + j];
    sums[(uint64_t)i * 4 + j] = d.sum[at * 4 + j];
  }
  first_seq[i] = seq;
}

// the audit: credited, admitted and the four limb sums from the log alone.  A block's limbs summed in
// LDS (256 limbs below 2^32: below 2^40), one integer atomic per figure and block.
__global__ void __launch_bounds__(256) k_ledger_recount(LedgerDev d, uint32_t count, unsigned long long *out) {
  __shared__ unsigned long long sh[4][256];
  const uint32_t seq = blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = seq < count;
  const bool credited = in && (d.flags[seq] & LEDGER_CREDITED);
  uint4 a = make_uint4(0, 0, 0, 0);
  if (credited) a = reinterpret_cast<const uint4 *>(d.amount)[seq];
  sh[0][threadIdx.x] = a.x, sh[1][threadIdx.x] = a.y, sh[2][threadIdx.x] = a.z, sh[3][threadIdx.x] = a.w;
  __syncthreads();
  for (uint32_t off = 128; off; off >>= 1) {
    if (threadIdx.x < off)
#pragma unroll
      for (int j = 0; j < 4; j++) sh[j][threadIdx.x] += sh[j][threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x < 4 && sh[threadIdx.x][0]) atomicAdd(out + 2 + threadIdx.x, sh[threadIdx.x][0]);
  const bool pred[2] = {credited, in};
  unsigned long long *const dst[2] = {out, out + 1};
  block_count(pred, dst);
}

void ledger_screen(const LedgerScreen &sc, const uint64_t *pis, const uint32_t *verdicts, uint32_t n,
                   uint64_t first_number, LedgerResult *res, uint32_t *blk, hipStream_t s) {
  if (!n) return;
  k_ledger_screen<<<ledger_blocks(n), LEDGER_BLOCK, 0, s>>>(sc, pis, verdicts, n, first_number, res, blk);
}

void ledger_scan(uint32_t *blk, uint32_t nb, uint32_t *total, hipStream_t s) {
  k_ledger_scan<<<1, 256, 0, s>>>(blk, nb, total);
}

void ledger_pack(const LedgerDev &d, const uint64_t *pis, const LedgerResult *res, const uint32_t *blk, uint32_t n,
                 uint32_t first_seq, uint32_t *pos, hipStream_t s) {
  if (!n) return;
  k_ledger_pack<<<ledger_blocks(n), LEDGER_BLOCK, 0, s>>>(d, pis, res, blk, n, first_seq, pos);
}

void ledger_insert(const LedgerDev &d, uint32_t first_seq, uint32_t k, uint32_t *stay, LedgerCounters *ctr,
                   hipStream_t s) {
  if (!k) return;
  k_ledger_insert<<<ledger_blocks(k), LEDGER_BLOCK, 0, s>>>(d, first_seq, k, stay, &ctr->err);
}

void ledger_resolve(const LedgerDev &d, uint32_t first_seq, uint32_t k, const uint32_t *stay, const uint32_t *pos,
                    LedgerResult *res, LedgerCounters *ctr, hipStream_t s) {
  if (!k) return;
  k_ledger_resolve<<<ledger_blocks(k), LEDGER_BLOCK, 0, s>>>(d, first_seq, k, stay, pos, res, ctr);
}

void ledger_rebuild(const LedgerDev &d, uint32_t count, LedgerCounters *ctr, hipStream_t s) {
  if (!count) return;
  k_ledger_rebuild<<<ledger_blocks(count), LEDGER_BLOCK, 0, s>>>(d, count, &ctr->err);
}

void ledger_find(const LedgerDev &d, uint32_t count, const uint64_t *q, uint32_t k, uint32_t *seq_out,
                 LedgerCounters *ctr, hipStream_t s) {
  if (!k) return;
  k_ledger_find<<<ledger_blocks(k), LEDGER_BLOCK, 0, s>>>(d, count, q, k, seq_out, &ctr->err);
}

void ledger_totals(const LedgerDev &d, uint32_t count, const uint64_t *q, uint32_t k, unsigned long long *sums,
                   uint32_t *found, LedgerCounters *ctr, hipStream_t s) {
  if (!k) return;
  k_ledger_totals<<<ledger_blocks(k), LEDGER_BLOCK, 0, s>>>(d, count, q, k, sums, found, &ctr->err);
}

void ledger_payee_count(const LedgerDev &d, uint32_t count, uint32_t *blk, hipStream_t s) {
  if (!count) return;
  k_ledger_payee_count<<<ledger_blocks(count), LEDGER_BLOCK, 0, s>>>(d, count, blk);
}

void ledger_payee_write(const LedgerDev &d, uint32_t count, const uint32_t *blk, uint32_t *payee, hipStream_t s) {
  if (!count) return;
  k_ledger_payee_write<<<ledger_blocks(count), LEDGER_BLOCK, 0, s>>>(d, count, blk, payee);
}

void ledger_payouts(const LedgerDev &d, const uint32_t *payee, uint32_t k, uint64_t *accounts,
                    unsigned long long *sums, uint64_t *first_seq, hipStream_t s) {
  if (!k) return;
  k_ledger_payouts<<<ledger_blocks(k), LEDGER_BLOCK, 0, s>>>(d, payee, k, accounts, sums, first_seq);
}

void ledger_recount(const LedgerDev &d, uint32_t count, unsigned long long *out, hipStream_t s) {
  if (!count) return;
  k_ledger_recount<<<ledger_blocks(count), LEDGER_BLOCK, 0, s>>>(d, count, out);
}

}  // namespace qpk
