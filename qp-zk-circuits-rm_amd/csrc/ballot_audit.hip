// ballot_audit.hip — the audit of a published ballot log on the device
// (gfx950; ballot_audit.h has the definitions, ballot_kernels.h the report's
// layout).  Memory-bound like ballot.hip's table kernels: a lane reads its
// entry (41 bytes) and, in the second pass, one slot word.  The table pass
// between the two is ballot.hip's own k_ballot_insert over the whole log; the
// root is k_ballot_leaves and the accumulator tree's append, as commit_log.
//
// Why the whole-log insert decides the count rule (facts 1-3 of table_probe,
// slot_table_device.h): the host uploaded all n entries before the launch
// (fact 2), the table is fresh and holds S >= 2 n slots (fact 3), and whatever the
// scheduling the slot of a nullifier ends at the minimum seq of the entries
// that carry it (fact 1).  k_audit_resolve is a launch of its own after the
// insert on the same stream, so every slot word is final and visible to plain
// loads: owner == seq says "no earlier entry has this nullifier".
//
// Seqs are consecutive across a wave, so each reason's lowest offender goes out
// by lowest_offender's one atomicMin per wave.
#include "ballot_kernels.h"
#include "slot_table_device.h"

namespace qpk {

// one lane per entry.  The neighbour number[seq - 1] is a plain load of
// uploaded data, across a block edge as inside one.
__global__ void __launch_bounds__(256) k_audit_screen(BallotDev d, uint32_t n, BallotAuditDev *rep) {
  const uint32_t seq = blockIdx.x * blockDim.x + threadIdx.x;
  bool bad = false, unordered = false;
  if (seq < n) {
    const uint64_t *key = d.nullifier + (uint64_t)seq * 4;
    const uint64_t num = d.number[seq];
    bad = key[0] >= qst::P || key[1] >= qst::P || key[2] >= qst::P || key[3] >= qst::P || num >= qst::P ||
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
  uint32_t owner = SLOT_EMPTY;
  if (seq < n) {
    const uint32_t at = stay[seq];
    if (at != NO_SLOT) owner = d.slot[at];
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
