// ballot.hip — the ballot box's nullifier table and tally (gfx950).  Layout
// and the home-slot rule: ballot_kernels.h.  Memory-latency-bound: a lane does
// one or a few dependent slot atomics and 32-byte key reads; no arithmetic to
// speak of.  The log commitment's leaf kernel is the exception: VALU-bound, one
// permutation per lane (merkle_node.h), like registry.hip's.
#include "ballot_kernels.h"
#include "merkle_node.h"
#include "slot_table_device.h"

namespace qpk {

namespace {
__device__ __forceinline__ SlotTable nullifier_table(const BallotDev &d) { return {d.nullifier, d.slot, d.mask}; }
}  // namespace

// one lane per admitted ballot of the batch
__global__ void __launch_bounds__(256) k_ballot_insert(BallotDev d, uint32_t first_seq, uint32_t k,
                                                       uint32_t *__restrict__ stay, uint32_t *__restrict__ err) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= k) return;
  bool claimed;
  const uint32_t at = table_probe(nullifier_table(d), first_seq + i, first_seq + k, &claimed);
  stay[i] = at;
  if (at == NO_SLOT) atomicOr(err, 1u);
}

// a launch after the insert: every slot word is final.  One lane per admitted
// ballot of the batch; the lanes past k only take part in the block's count.
__global__ void __launch_bounds__(256) k_ballot_resolve(BallotDev d, uint32_t first_seq, uint32_t k,
                                                        const uint32_t *__restrict__ stay,
                                                        uint64_t *__restrict__ first_out, BallotCounters *ctr) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  bool yes = false, no = false;
  if (i < k) {
    const uint32_t seq = first_seq + i, at = stay[i];
    const uint32_t owner = at == NO_SLOT ? SLOT_EMPTY : d.slot[at];
    if (owner > seq) {  // an entry's slot holds the minimum of its nullifier's seqs: defensive, as the probe's bound
      atomicOr(&ctr->err, 2u);
      first_out[i] = ~0ull;
    } else {
      first_out[i] = d.number[owner];
      if (owner == seq) {
        const uint8_t f = d.flags[seq];
        d.flags[seq] = f | BALLOT_COUNTED;
        yes = f & BALLOT_VOTE;
        no = !yes;
      }
    }
  }
  const bool pred[2] = {yes, no};
  unsigned long long *const dst[2] = {&ctr->yes, &ctr->no};
  block_count(pred, dst);
}

// reserve: the counted entries of the copied log into the new, empty table
// with the insert's probe.  Counted entries have distinct nullifiers, so each
// claims a slot; the minimum rule makes the order irrelevant.
__global__ void __launch_bounds__(256) k_ballot_rebuild(BallotDev d, uint32_t count, uint32_t *__restrict__ err) {
  const uint32_t seq = blockIdx.x * blockDim.x + threadIdx.x;
  if (seq >= count || !(d.flags[seq] & BALLOT_COUNTED)) return;
  bool claimed;
  if (table_probe(nullifier_table(d), seq, count, &claimed) == NO_SLOT) atomicOr(err, 1u);
}

// the audit: yes, no, counted and admitted from the flags alone
__global__ void __launch_bounds__(256) k_ballot_recount(const uint8_t *__restrict__ flags, uint32_t count,
                                                        unsigned long long *out) {
  const uint32_t seq = blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = seq < count;
  const uint8_t f = in ? flags[seq] : 0;
  const bool counted = f & BALLOT_COUNTED, vote = f & BALLOT_VOTE;
  const bool pred[4] = {counted && vote, counted && !vote, counted, in};
  unsigned long long *const dst[4] = {out, out + 1, out + 2, out + 3};
  block_count(pred, dst);
}

// ---- the log commitment (ballot_kernels.h): leaves, lookup, gather

// log leaf seq = hash_no_pad([nullifier[0..4], number, flags]) into level 0 of
// the digest buffer: one lane per entry of [first, end), the registry leaf
// kernel's permutation form.  A number >= p cannot be reached (numbers count
// ballots); it is not hashed and sets the error word.
__global__ void __launch_bounds__(256) k_ballot_leaves(BallotDev d, uint32_t first, uint32_t end,
                                                       uint64_t *__restrict__ dig, uint32_t *__restrict__ err) {
  const uint64_t seq = (uint64_t)first + blockIdx.x * blockDim.x + threadIdx.x;
  if (seq >= end) return;
  const uint64_t *key = d.nullifier + seq * 4;
  uint64_t s[12];
#pragma unroll
  for (int j = 0; j < 4; j++) s[j] = key[j];
  s[4] = d.number[seq];
  s[5] = d.flags[seq];
  s[6] = s[7] = 0;
  if (s[4] >= qst::P) {
    atomicOr(err, 4u);
    return;
  }
  node_digest(s);
  uint64_t *o = dig + seq * 4;
#pragma unroll
  for (int j = 0; j < 4; j++) o[j] = s[j];
}

// one lane per queried nullifier q[i][4]: the read-only probe (fact 4).
// seq_out[i] = the log index of the counted entry with that nullifier, or
// 0xFFFFFFFF.  count: the log's entries; a slot word at or beyond it is not a
// log entry (cannot be reached): nothing is read through it, the error word is set.
__global__ void __launch_bounds__(256) k_ballot_find(BallotDev d, uint32_t count, const uint64_t *__restrict__ q,
                                                     uint32_t k, uint32_t *__restrict__ seq_out,
                                                     uint32_t *__restrict__ err) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= k) return;
  uint64_t key[4];
  load_key(q + (uint64_t)i * 4, key);
  bool bad = false;
  const uint32_t at = table_lookup(nullifier_table(d), key, count, &bad);
  if (bad) atomicOr(err, 8u);
  seq_out[i] = at == NO_SLOT ? SLOT_EMPTY : d.slot[at];
}

// log entries seq[i] < count (the caller checks) into dense arrays: one lane per entry
__global__ void __launch_bounds__(256) k_ballot_gather(BallotDev d, const uint64_t *__restrict__ seq, uint32_t k,
                                                       uint64_t *__restrict__ nullifier, uint64_t *__restrict__ number,
                                                       uint8_t *__restrict__ flags) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= k) return;
  const uint64_t at = seq[i];
#pragma unroll
  for (int j = 0; j < 4; j++) nullifier[(uint64_t)i * 4 + j] = d.nullifier[at * 4 + j];
  number[i] = d.number[at];
  flags[i] = d.flags[at];
}

static unsigned ballot_blocks(uint32_t n) { return (unsigned)(((uint64_t)n + 255) / 256); }

void ballot_insert(const BallotDev &d, uint32_t first_seq, uint32_t k, uint32_t *stay, BallotCounters *ctr,
                   hipStream_t s) {
  if (!k) return;
  k_ballot_insert<<<ballot_blocks(k), 256, 0, s>>>(d, first_seq, k, stay, &ctr->err);
}

void ballot_resolve(const BallotDev &d, uint32_t first_seq, uint32_t k, const uint32_t *stay, uint64_t *first_out,
                    BallotCounters *ctr, hipStream_t s) {
  if (!k) return;
  k_ballot_resolve<<<ballot_blocks(k), 256, 0, s>>>(d, first_seq, k, stay, first_out, ctr);
}

void ballot_rebuild(const BallotDev &d, uint32_t count, BallotCounters *ctr, hipStream_t s) {
  if (!count) return;
  k_ballot_rebuild<<<ballot_blocks(count), 256, 0, s>>>(d, count, &ctr->err);
}

void ballot_recount(const uint8_t *flags, uint32_t count, unsigned long long *out, hipStream_t s) {
  if (!count) return;
  k_ballot_recount<<<ballot_blocks(count), 256, 0, s>>>(flags, count, out);
}

void ballot_leaves(const BallotDev &d, uint32_t first, uint32_t end, uint64_t *dig, BallotCounters *ctr,
                   hipStream_t s) {
  if (first >= end) return;
  k_ballot_leaves<<<ballot_blocks(end - first), 256, 0, s>>>(d, first, end, dig, &ctr->err);
}

void ballot_find(const BallotDev &d, uint32_t count, const uint64_t *q, uint32_t k, uint32_t *seq_out,
                 BallotCounters *ctr, hipStream_t s) {
  if (!k) return;
  k_ballot_find<<<ballot_blocks(k), 256, 0, s>>>(d, count, q, k, seq_out, &ctr->err);
}

void ballot_gather(const BallotDev &d, const uint64_t *seq, uint32_t k, uint64_t *nullifier, uint64_t *number,
                   uint8_t *flags, hipStream_t s) {
  if (!k) return;
  k_ballot_gather<<<ballot_blocks(k), 256, 0, s>>>(d, seq, k, nullifier, number, flags);
}

}  // namespace qpk
