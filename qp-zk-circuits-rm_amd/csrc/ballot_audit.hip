// ballot_audit.hip — the audit of a published ballot log on the device
// (gfx950; ballot_audit.h has the definitions, ballot_kernels.h the report's
// layout).  Memory-bound like ballot.hip's table kernels: a lane reads its
// entry (41 bytes) and, in the second pass, one slot word.  The table pass
// between the two is ballot.hip's own k_ballot_insert over the whole log; the
// root is k_ballot_leaves and the accumulator tree's append, as commit_log.
//
// Why the whole-log insert decides the count rule (facts 1-3 of ballot.hip's
// probe): the host uploaded all n entries before the launch (fact 2), the
// table is fresh and holds S >= 2 n slots (fact 3), and whatever the
// scheduling the slot of a nullifier ends at the minimum seq of the entries
// that carry it (fact 1).  k_audit_resolve is a launch of its own after the
// insert on the same stream, so every slot word is final and visible to plain
// loads: owner == seq says "no earlier entry has this nullifier".
//
// The lowest offender: seqs are consecutive across a wave, so the lowest
// offending lane of a wave's ballot holds the wave's lowest seq and alone
// sends it, one atomicMin per wave and reason at the most; the minimum over
// the waves does not depend on the order they arrive in.
#include "ballot_device.h"
#include "ballot_kernels.h"

namespace qpk {

namespace {
// true in the lowest lane of the wave whose `bad` is set; every lane of the wave calls it
__device__ __forceinline__ bool lowest_offender(bool bad) {
  const uint64_t m = __ballot(bad);
  return bad && (threadIdx.x & 63) == (uint32_t)(__ffsll((unsigned long long)m) - 1);
}
}  // namespace

// one lane per entry.  The neighbour number[seq - 1] is a plain load of
// uploaded data, across a block edge as inside one.
__global__ void __launch_bounds__(256) k_audit_screen(BallotDev d, uint32_t n, BallotAuditDev *rep) {
  const uint32_t seq = blockIdx.x * blockDim.x + threadIdx.x;
  bool bad = false, unordered = false;
  if (seq < n) {
    const uint64_t *key = d.nullifier + (uint64_t)seq * 4;
    const uint64_t num = d.number[seq];
    bad = key[0] >= BALLOT_P || key[1] >= BALLOT_P || key[2] >= BALLOT_P || key[3] >= BALLOT_P || num >= BALLOT_P ||
          d.flags[seq] > (BALLOT_VOTE | BALLOT_COUNTED);
    unordered = seq && num <= d.number[seq - 1];
  }
  if (lowest_offender(bad)) atomicMin(&rep->non_canonical, seq);
  if (lowest_offender(unordered)) atomicMin(&rep->order, seq);
}

// a launch after the whole-log insert: every slot word is final.  One lane per
// entry; the lanes past n only take part in the wave's ballots and the block's
// count.  Reads the flags, writes none.
__global__ void __launch_bounds__(256) k_audit_resolve(BallotDev d, uint32_t n, const uint32_t *__restrict__ stay,
                                                       BallotAuditDev *rep) {
  const uint32_t seq = blockIdx.x * blockDim.x + threadIdx.x;
  bool yes = false, no = false, counted = false, broken = false;
  uint32_t owner = BALLOT_EMPTY;
  if (seq < n) {
    const uint32_t at = stay[seq];
    if (at != BALLOT_NO_SLOT) owner = d.slot[at];
    const uint8_t f = d.flags[seq];
    counted = f & BALLOT_COUNTED;
    yes = counted && (f & BALLOT_VOTE);
    no = counted && !(f & BALLOT_VOTE);
    if (owner > seq)  // an entry's slot holds the minimum of its nullifier's seqs: defensive, as the probe's bound
      atomicOr(&rep->ctr.err, 2u);
    else
      broken = counted != (owner == seq);
  }
  if (lowest_offender(broken)) atomicMin(&rep->count_rule, (unsigned long long)seq << 32 | owner);
  const bool pred[3] = {yes, no, counted};
  unsigned long long *const dst[3] = {&rep->ctr.yes, &rep->ctr.no, &rep->counted};
  block_count(pred, dst);
}

static unsigned audit_blocks(uint32_t n) { return (unsigned)(((uint64_t)n + 255) / 256); }

void ballot_audit_screen(const BallotDev &d, uint32_t n, BallotAuditDev *rep, hipStream_t s) {
  if (!n) return;
  k_audit_screen<<<audit_blocks(n), 256, 0, s>>>(d, n, rep);
}

void ballot_audit_resolve(const BallotDev &d, uint32_t n, const uint32_t *stay, BallotAuditDev *rep, hipStream_t s) {
  if (!n) return;
  k_audit_resolve<<<audit_blocks(n), 256, 0, s>>>(d, n, stay, rep);
}

}  // namespace qpk
