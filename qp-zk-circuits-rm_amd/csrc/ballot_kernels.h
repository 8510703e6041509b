// ballot_kernels.h — argument layouts and launchers of ballot.hip: the ballot
// box's nullifier table and tally on the device.  One launcher per step; the
// launcher owns the grid and block sizes.
//
// The log (dense, indexed by admission sequence seq, written by the host's
// upload before any launch that reads it):
//   nullifier[C][4]   number[C]   flags[C] (bit 0 the vote, bit 1 counted)
// The table: a slot table (slot_table.h has the layout and the home-slot rule,
// slot_table_device.h the probes) of S = the power of two >= 2 C slots, keyed
// by the nullifier.
//
// The log commitment (ballot_log.h has the definitions): the log tree is an
// accumulator tree (acc_tree.h) laid out for the box's capacity.
// k_ballot_leaves writes its level 0; the levels above and the paths are the
// tree's own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace qpk {

struct BallotDev {
  uint64_t *nullifier;  // [C][4]
  uint64_t *number;     // [C]
  uint8_t *flags;       // [C]
  uint32_t *slot;       // [mask + 1]
  uint64_t mask;        // S - 1
};

constexpr uint8_t BALLOT_VOTE = 1, BALLOT_COUNTED = 2;  // the bits of a log entry's flags byte

// the box's device counters: the running tally and the defensive error word
struct BallotCounters {
  unsigned long long yes, no;
  uint32_t err, pad;
};

__global__ void k_ballot_insert(BallotDev d, uint32_t first_seq, uint32_t k, uint32_t *stay, uint32_t *err);
__global__ void k_ballot_resolve(BallotDev d, uint32_t first_seq, uint32_t k, const uint32_t *stay, uint64_t *first_out,
                                 BallotCounters *ctr);
__global__ void k_ballot_rebuild(BallotDev d, uint32_t count, uint32_t *err);
__global__ void k_ballot_recount(const uint8_t *flags, uint32_t count, unsigned long long *out);
__global__ void k_ballot_leaves(BallotDev d, uint32_t first, uint32_t end, uint64_t *dig, uint32_t *err);
__global__ void k_ballot_find(BallotDev d, uint32_t count, const uint64_t *q, uint32_t k, uint32_t *seq_out,
                              uint32_t *err);
__global__ void k_ballot_gather(BallotDev d, const uint64_t *seq, uint32_t k, uint64_t *nullifier, uint64_t *number,
                                uint8_t *flags);

// log entries [first_seq, first_seq + k) (already uploaded) into the table;
// stay[i] = the slot entry first_seq + i stopped at.  The caller keeps
// first_seq + k <= C.
void ballot_insert(const BallotDev &d, uint32_t first_seq, uint32_t k, uint32_t *stay, BallotCounters *ctr,
                   hipStream_t s);
// after ballot_insert, a launch of its own: first_out[i] = the number of the
// entry that owns stay[i]'s slot (entry i's own: counted, its flag set and its
// vote added to ctr)
void ballot_resolve(const BallotDev &d, uint32_t first_seq, uint32_t k, const uint32_t *stay, uint64_t *first_out,
                    BallotCounters *ctr, hipStream_t s);
// the counted entries of log [0, count) into a fresh (all-empty) table
void ballot_rebuild(const BallotDev &d, uint32_t count, BallotCounters *ctr, hipStream_t s);
// out[4] (zeroed by the caller) += yes, no, counted, admitted of flags [0, count)
void ballot_recount(const uint8_t *flags, uint32_t count, unsigned long long *out, hipStream_t s);
// the log leaves of entries [first, end) into dig[seq][4] (level 0 of the log tree); end <= C
void ballot_leaves(const BallotDev &d, uint32_t first, uint32_t end, uint64_t *dig, BallotCounters *ctr,
                   hipStream_t s);
// seq_out[i] = the log index of the counted entry with nullifier q[i][4] (device), or 0xFFFFFFFF;
// count = the log's entries.  After every insert and resolve on the same stream; read-only.
void ballot_find(const BallotDev &d, uint32_t count, const uint64_t *q, uint32_t k, uint32_t *seq_out,
                 BallotCounters *ctr, hipStream_t s);
// the log entries seq[i] (device; each below the log's count, the caller checks) into dense arrays
void ballot_gather(const BallotDev &d, const uint64_t *seq, uint32_t k, uint64_t *nullifier, uint64_t *number,
                   uint8_t *flags, hipStream_t s);

// ---- the audit of a published log (ballot_audit.hip; ballot_audit.h has the definitions).  The
// log is uploaded whole, a fresh all-empty table takes it in one ballot_insert (first_seq = 0,
// k = n), and the audit writes nothing but its report.
constexpr uint32_t AUDIT_NO_SEQ = 0xFFFFFFFFu;  // no offender (seqs stay below 2^31)

// the device half of a report; the host sets the three offender words to all-ones, the rest to zero
struct BallotAuditDev {
  BallotCounters ctr;             // yes, no of the counted flags; the defensive error word of insert and leaves
  unsigned long long counted;     // entries with the counted bit
  unsigned long long count_rule;  // the lowest (seq << 32 | owner) whose counted bit != (owner == seq)
  uint32_t non_canonical, order;  // the lowest offending seq of each
};

__global__ void k_audit_screen(BallotDev d, uint32_t n, BallotAuditDev *rep);
__global__ void k_audit_resolve(BallotDev d, uint32_t n, const uint32_t *stay, BallotAuditDev *rep);

// one lane per entry of [0, n): the canonical checks and number[seq] > number[seq - 1]
void ballot_audit_screen(const BallotDev &d, uint32_t n, BallotAuditDev *rep, hipStream_t s);
// after ballot_insert(d, 0, n, stay, &rep->ctr, s) into a fresh table, a launch of its own: the count
// rule per entry from stay[] and the final slot words, and the counts of the flags.  Writes no flag.
void ballot_audit_resolve(const BallotDev &d, uint32_t n, const uint32_t *stay, BallotAuditDev *rep, hipStream_t s);

}  // namespace qpk
