// ballot.hip — the ballot box's nullifier table and tally (gfx950).  Layout
// and the home-slot rule: ballot_kernels.h.  Memory-latency-bound: a lane does
// one or a few dependent slot atomics and 32-byte key reads; no arithmetic to
// speak of.  The log commitment's leaf kernel is the exception: VALU-bound, one
// permutation per lane (merkle_node.h), like registry.hip's.
#include "ballot_device.h"
#include "ballot_kernels.h"
#include "merkle_node.h"

namespace qpk {

namespace {
// The probe of log entry seq (the log holds `limit` entries): returns the slot
// where it stays, BALLOT_NO_SLOT if S slots were tried (see fact 3 below).
//
// Why the table is correct:
// 1. A slot's nullifier never changes once the slot is claimed: a claimed slot
//    holds a seq, and the only later write to it is an atomicMin by a lane
//    whose own nullifier equals log[seq]'s, so the word only ever moves to
//    another entry with the same nullifier.  A lane passes a slot only if the
//    nullifier there differs from its own, which therefore stays true.  So all
//    entries with one nullifier probe the same chain and stop at the same slot
//    whatever the interleaving, and the slot ends at the minimum of their
//    seqs: the lowest ballot number, since seq is monotone in the number.
// 2. The keys a lane compares against are in the log, which the host uploaded
//    before this launch (entries of this batch included).  A lane reads nothing
//    that a lane of the same launch wrote, except the slot word, and that only
//    through agent-scope atomics (load, compare-and-swap, min), which are
//    performed at the device's coherence point and not in an XCD's own L2.
//    That is why the key is not stored in the slot: a plain load does not see
//    another XCD's plain store of the same launch.  No fences, no flags, no
//    spin: no lane waits on another lane.
// 3. The host keeps count + k <= C <= S / 2 before it launches, so an empty
//    slot exists and the loop ends at it at the latest.  The loop is bounded by
//    S all the same; running out cannot be reached and is reported through the
//    error word, after which the box refuses further casts.
// 4. The lookup (k_ballot_find) takes no atomics and writes no slot.  It runs
//    on the box's stream in a launch of its own after every insert, resolve
//    and rebuild has completed, and nothing runs beside it: the slot words and
//    the log it reads were final before it started, and a kernel boundary on
//    one stream makes them visible to plain loads on every XCD.  Nothing is
//    ever removed, so a chain has no gap and an empty slot ends it.
__device__ __forceinline__ uint32_t ballot_probe(const BallotDev &d, uint32_t seq, uint32_t limit) {
  const uint64_t *key = d.nullifier + (uint64_t)seq * 4;
  const uint64_t k0 = key[0], k1 = key[1], k2 = key[2], k3 = key[3];
  uint64_t at = k0 & d.mask;
  for (uint64_t tried = 0; tried <= d.mask; tried++, at = (at + 1) & d.mask) {
    uint32_t cur = __hip_atomic_load(d.slot + at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == BALLOT_EMPTY) {
      cur = atomicCAS(d.slot + at, BALLOT_EMPTY, seq);
      if (cur == BALLOT_EMPTY) return (uint32_t)at;  // claimed
    }
    if (cur == seq) return (uint32_t)at;
    if (cur >= limit) break;  // not a log entry: cannot be reached (only seqs below the limit are ever stored)
    const uint64_t *o = d.nullifier + (uint64_t)cur * 4;  // cur < limit = count + k <= C, written before the launch
    if (o[0] == k0 && o[1] == k1 && o[2] == k2 && o[3] == k3) {
      atomicMin(d.slot + at, seq);
      return (uint32_t)at;
    }
  }
  return BALLOT_NO_SLOT;
}
}  // namespace

// one lane per admitted ballot of the batch
__global__ void __launch_bounds__(256) k_ballot_insert(BallotDev d, uint32_t first_seq, uint32_t k,
                                                       uint32_t *__restrict__ stay, uint32_t *__restrict__ err) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= k) return;
  const uint32_t at = ballot_probe(d, first_seq + i, first_seq + k);
  stay[i] = at;
  if (at == BALLOT_NO_SLOT) atomicOr(err, 1u);
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
    const uint32_t owner = at == BALLOT_NO_SLOT ? BALLOT_EMPTY : d.slot[at];
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
  if (ballot_probe(d, seq, count) == BALLOT_NO_SLOT) atomicOr(err, 1u);
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
  if (s[4] >= BALLOT_P) {
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
  const uint64_t *key = q + (uint64_t)i * 4;
  const uint64_t k0 = key[0], k1 = key[1], k2 = key[2], k3 = key[3];
  uint32_t found = BALLOT_EMPTY;
  uint64_t at = k0 & d.mask;
  for (uint64_t tried = 0; tried <= d.mask; tried++, at = (at + 1) & d.mask) {
    const uint32_t cur = d.slot[at];
    if (cur == BALLOT_EMPTY) break;
    if (cur >= count) {
      atomicOr(err, 8u);
      break;
    }
    const uint64_t *o = d.nullifier + (uint64_t)cur * 4;
    if (o[0] == k0 && o[1] == k1 && o[2] == k2 && o[3] == k3) {
      found = cur;
      break;
    }
  }
  seq_out[i] = found;
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
