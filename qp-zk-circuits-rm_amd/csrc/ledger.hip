// ledger.hip — the transfer ledger on the device (gfx950): the screen of the
// public inputs, the stable pack of a batch's admitted transfers into the log,
// the nullifier table, the account table with its limb sums, the payouts'
// compaction and the read-only lookups.  Layouts and the home-slot rules:
// ledger_kernels.h.  Memory-latency-bound throughout: a lane reads 128 bytes of
// public inputs or does a few dependent slot atomics and 32-byte key reads.
// Blocks of 256 lanes (LEDGER_BLOCK).  The log commitment's leaf kernel is the
// exception: VALU-bound, two permutations per lane (poseidon_dev.h).  The audit
// of a published log reuses the insert, the probes, the recount and the payees'
// compaction over a table of the audit's own; a restore runs the audit's screen,
// insert and resolve over the new ledger's tables; a payout round credits a
// range of the log into a scratch account table and reuses the same compaction.
#include "ledger_kernels.h"
#include "ledger_rounds.h"
#include "ledger_table.h"
#include "poseidon_dev.h"
#include "slot_table_device.h"

namespace qpk {

namespace {
constexpr uint8_t LEDGER_CREDITED = ql::FLAG_CREDITED;

__device__ __forceinline__ SlotTable nullifier_table(const LedgerDev &d) { return {d.nullifier, d.nslot, d.mask}; }
__device__ __forceinline__ SlotTable account_table(const LedgerDev &d) { return {d.account, d.aslot, d.mask}; }

// a credited entry into the account table, its limbs onto the account's sums.  The sums are indexed
// by the slot the key stays at, which fact 1 fixes for the key whatever the interleaving; integer
// addition commutes, so the sums are exact in any order.  Nothing reads a sum in this launch.
__device__ __forceinline__ bool credit_entry(const LedgerDev &d, uint32_t seq, uint32_t limit, bool *claimed) {
  const uint32_t at = table_probe(account_table(d), seq, limit, claimed);
  d.astay[seq] = at;
  if (at == NO_SLOT) return false;
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
  return at != NO_SLOT && d.aslot[at] == seq;
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
  d.astay[seq] = NO_SLOT;
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
  if (at == NO_SLOT) atomicOr(err, 1u);
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
    const uint32_t owner = at == NO_SLOT ? SLOT_EMPTY : d.nslot[at];
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
  if (table_probe(nullifier_table(d), seq, count, &claimed) == NO_SLOT) atomicOr(err, 1u);
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
  seq_out[i] = at == NO_SLOT ? SLOT_EMPTY : d.nslot[at];
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
  found[i] = at != NO_SLOT;
#pragma unroll
  for (int j = 0; j < 4; j++) sums[(uint64_t)i * 4 + j] = at == NO_SLOT ? 0 : d.sum[(uint64_t)at * 4 + j];
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

// ---- the log commitment (ledger_kernels.h, ledger_log.h): leaves, gather

// log leaf seq = hash_no_pad of the entry's 14 felts into level 0 of the digest buffer: one lane per
// entry of [first, end).  The overwrite sponge takes two permutations: felts 0..7 (nullifier, number,
// amount limbs 0..2) over a zero state, then felts 8..13 (amount limb 3, account, flags) over lanes
// 0..5 with lanes 6..11 as the first permutation left them.  Both are poseidon_fast.h's forms: the
// zero-capacity one with all twelve lanes out (what node_digest runs with four), then the general one
// with lanes 0..3 out.  The state stays non-canonical in between (permute_nc takes any 64-bit lanes);
// canon on the four lanes stored.  VALU-bound, registers only: no LDS, no scratch.  A number >= p
// cannot be reached (numbers count transfers); it is not hashed and sets the error word.
__global__ void __launch_bounds__(256) k_ledger_leaves(LedgerDev d, uint32_t first, uint32_t end,
                                                       uint64_t *__restrict__ dig, uint32_t *__restrict__ err) {
  const uint64_t seq = (uint64_t)first + blockIdx.x * blockDim.x + threadIdx.x;
  if (seq >= end) return;
  uint64_t s[12], acc[4];
  load_key(d.nullifier + seq * 4, s);
  s[4] = d.number[seq];
  const uint4 a = reinterpret_cast<const uint4 *>(d.amount)[seq];
  s[5] = a.x, s[6] = a.y, s[7] = a.z;
  if (s[4] >= ql::P) {
    atomicOr(err, LEDGER_ERR_NUMBER);
    return;
  }
  s[8] = s[9] = s[10] = s[11] = 0;
  pf::permute_nc_capz<0xFFFu>(s);
  load_key(d.account + seq * 4, acc);
  s[0] = a.w;
#pragma unroll
  for (int j = 0; j < 4; j++) s[1 + j] = acc[j];
  s[5] = d.flags[seq];
#pragma unroll
  for (int j = 0; j < 12; j++) s[j] = pf::add_c(s[j], ps::rc_cx(j));
  pf::rounds<0, 0xFu>(s);
  ulonglong2 *o = reinterpret_cast<ulonglong2 *>(dig + seq * 4);
  o[0] = make_ulonglong2(psd::canon(s[0]), psd::canon(s[1]));
  o[1] = make_ulonglong2(psd::canon(s[2]), psd::canon(s[3]));
}

// log entries seq[i] < count (the caller checks) into dense arrays: one lane per entry
__global__ void __launch_bounds__(256) k_ledger_gather(LedgerDev d, const uint64_t *__restrict__ seq, uint32_t k,
                                                       uint64_t *__restrict__ nullifier, uint64_t *__restrict__ number,
                                                       uint32_t *__restrict__ amount, uint64_t *__restrict__ account,
                                                       uint8_t *__restrict__ flags) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= k) return;
  const uint64_t at = seq[i];
  const ulonglong2 *nul = reinterpret_cast<const ulonglong2 *>(d.nullifier + at * 4);
  const ulonglong2 *acc = reinterpret_cast<const ulonglong2 *>(d.account + at * 4);
  ulonglong2 *onul = reinterpret_cast<ulonglong2 *>(nullifier + (uint64_t)i * 4);
  ulonglong2 *oacc = reinterpret_cast<ulonglong2 *>(account + (uint64_t)i * 4);
  onul[0] = nul[0], onul[1] = nul[1];
  oacc[0] = acc[0], oacc[1] = acc[1];
  reinterpret_cast<uint4 *>(amount)[i] = reinterpret_cast<const uint4 *>(d.amount)[at];
  number[i] = d.number[at];
  flags[i] = d.flags[at];
}

// ---- the audit of a published log (ledger_audit.h has the rules).  Seqs are consecutive across a
// wave, so each reason's lowest offender goes out by lowest_offender's one atomicMin per wave.

// one lane per entry.  number[seq - 1] is a plain load of uploaded data, across a block edge as inside one.
__global__ void __launch_bounds__(256) k_ledger_audit_screen(LedgerDev d, uint32_t n, LedgerAuditDev *rep) {
  const uint32_t seq = blockIdx.x * blockDim.x + threadIdx.x;
  bool bad = false, unordered = false;
  if (seq < n) {
    uint64_t nul[4], acc[4];
    load_key(d.nullifier + (uint64_t)seq * 4, nul);
    load_key(d.account + (uint64_t)seq * 4, acc);
    const uint64_t num = d.number[seq];
    bad = num >= ql::P || d.flags[seq] > LEDGER_CREDITED;
#pragma unroll
    for (int j = 0; j < 4; j++) bad = bad || nul[j] >= ql::P || acc[j] >= ql::P;
    unordered = seq && num <= d.number[seq - 1];
  }
  if (lowest_offender(bad)) atomicMin(&rep->non_canonical, seq);
  if (lowest_offender(unordered)) atomicMin(&rep->order, seq);
}

// a launch after the whole-log insert: every nullifier slot word is final (facts 1-3 of table_probe:
// the slot of a nullifier ends at the lowest seq that carries it, whatever the scheduling), so owner ==
// seq says "no earlier entry has this nullifier".  One lane per entry; the lanes past n only take part
// in the wave's ballots and the block's counts.  The flags are read and never written; an entry whose
// flag says credited goes into the account table and onto its sums, as in k_ledger_resolve.
__global__ void __launch_bounds__(256) k_ledger_audit_resolve(LedgerDev d, uint32_t n,
                                                              const uint32_t *__restrict__ stay,
                                                              LedgerAuditDev *rep) {
  const uint32_t seq = blockIdx.x * blockDim.x + threadIdx.x;
  bool credited = false, claimed = false, broken = false;
  uint32_t owner = SLOT_EMPTY;
  if (seq < n) {
    const uint32_t at = stay[seq];
    if (at != NO_SLOT) owner = d.nslot[at];
    credited = d.flags[seq] & LEDGER_CREDITED;
    if (owner > seq)  // a slot holds the minimum of its nullifier's seqs: defensive, as the probe's bound
      atomicOr(&rep->ctr.err, 2u);
    else
      broken = credited != (owner == seq);
    d.astay[seq] = NO_SLOT;
    if (credited && !credit_entry(d, seq, n, &claimed)) atomicOr(&rep->ctr.err, 4u);
  }
  if (lowest_offender(broken)) atomicMin(&rep->credit_rule, (unsigned long long)seq << 32 | owner);
  const bool pred[2] = {credited, claimed};
  unsigned long long *const dst[2] = {&rep->ctr.credited, &rep->ctr.accounts};
  block_count(pred, dst);
}

// one lane per claimed payout i < k <= the payees: the account, the four limb sums and first_seq
// against payee i.  The sums were added by k_ledger_audit_resolve, launches ago.
__global__ void __launch_bounds__(256) k_ledger_audit_payouts(LedgerDev d, const uint32_t *__restrict__ payee,
                                                              uint32_t k, const uint64_t *__restrict__ accounts,
                                                              const uint64_t *__restrict__ sums,
                                                              const uint64_t *__restrict__ first_seq,
                                                              LedgerAuditDev *rep) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  bool differs = false;
  if (i < k) {
    const uint32_t seq = payee[i];
    const uint64_t at = d.astay[seq];
    uint64_t want[4], got[4], ws[4], ls[4];
    load_key(d.account + (uint64_t)seq * 4, want);
    load_key(accounts + (uint64_t)i * 4, got);
    load_key(sums + (uint64_t)i * 4, ws);
    load_key(reinterpret_cast<const uint64_t *>(d.sum) + at * 4, ls);
    differs = !ql::key_equal(want, got) || first_seq[i] != seq || !ql::sums_equal(ws, ls);
  }
  if (lowest_offender(differs)) atomicMin(&rep->payout, i);
}

// ---- payout rounds (ledger_rounds.h has the rule).  v is a view of log entries [m0, m1) with a
// scratch account table of the call's own: v.account, v.amount and v.flags point at entry m0 and are
// only read; v.aslot (all empty), v.sum (zero) and v.astay belong to the call; a lane's index j = seq -
// m0 is what the slot words hold.  One lane per entry of the range.  A credited lane is credit_entry
// over the view: the ledger's probe (facts 1-3 of table_probe with limit = k <= S / 2, so the slot of an
// account ends at the lowest j credited to it in the range, by an agent-scope atomicMin), then four
// 64-bit atomicAdds onto the sums of the slot where the key stays.  Nothing reads a slot word or a sum
// in this launch: the owners are compacted by k_ledger_payee_count / k_ledger_scan /
// k_ledger_payee_write over the view and gathered by k_ledger_payouts, launches later.
__global__ void __launch_bounds__(256) k_ledger_round_credit(LedgerDev v, uint32_t k, uint32_t *__restrict__ err) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= k) return;
  bool claimed;
  if (!ql::round_credits(v.flags[j]))
    v.astay[j] = NO_SLOT;
  else if (!credit_entry(v, j, k, &claimed))
    atomicOr(err, 4u);  // the probe ran out of slots: cannot be reached
}

void ledger_round_credit(const LedgerDev &v, uint32_t k, uint32_t *err, hipStream_t s) {
  if (!k) return;
  k_ledger_round_credit<<<ledger_blocks(k), LEDGER_BLOCK, 0, s>>>(v, k, err);
}

void ledger_leaves(const LedgerDev &d, uint32_t first, uint32_t end, uint64_t *dig, LedgerCounters *ctr,
                   hipStream_t s) {
  if (first >= end) return;
  k_ledger_leaves<<<ledger_blocks(end - first), LEDGER_BLOCK, 0, s>>>(d, first, end, dig, &ctr->err);
}

void ledger_gather(const LedgerDev &d, const uint64_t *seq, uint32_t k, uint64_t *nullifier, uint64_t *number,
                   uint32_t *amount, uint64_t *account, uint8_t *flags, hipStream_t s) {
  if (!k) return;
  k_ledger_gather<<<ledger_blocks(k), LEDGER_BLOCK, 0, s>>>(d, seq, k, nullifier, number, amount, account, flags);
}

void ledger_audit_screen(const LedgerDev &d, uint32_t n, LedgerAuditDev *rep, hipStream_t s) {
  if (!n) return;
  k_ledger_audit_screen<<<ledger_blocks(n), LEDGER_BLOCK, 0, s>>>(d, n, rep);
}

void ledger_audit_resolve(const LedgerDev &d, uint32_t n, const uint32_t *stay, LedgerAuditDev *rep, hipStream_t s) {
  if (!n) return;
  k_ledger_audit_resolve<<<ledger_blocks(n), LEDGER_BLOCK, 0, s>>>(d, n, stay, rep);
}

void ledger_audit_payouts(const LedgerDev &d, const uint32_t *payee, uint32_t k, const uint64_t *accounts,
                          const uint64_t *sums, const uint64_t *first_seq, LedgerAuditDev *rep, hipStream_t s) {
  if (!k) return;
  k_ledger_audit_payouts<<<ledger_blocks(k), LEDGER_BLOCK, 0, s>>>(d, payee, k, accounts, sums, first_seq, rep);
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
