// ledger_kernels.h — argument layouts and launchers of ledger.hip: the transfer
// ledger's screen, pack, two tables and account sums on the device.  One
// launcher per step; the launcher owns the grid and block sizes.
//
// The log (dense, indexed by admission sequence seq, written by k_ledger_pack in
// a launch before any launch that reads it):
//   nullifier[C][4] number[C] amount[C][4] (u32 limbs, most significant first)
//   account[C][4]   flags[C] (bit 0 credited)   astay[C] (a credited entry's account slot)
// The tables: two slot tables (slot_table.h has the layout and the home-slot
// rule, slot_table_device.h the probes) of S = the power of two >= 2 C slots
// each: nslot keyed by the nullifier, aslot by the exit account, with sum[S][4]
// beside it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace qpk {

struct LedgerDev {
  uint64_t *nullifier;      // [C][4]
  uint64_t *number;         // [C]
  uint32_t *amount;         // [C][4]
  uint64_t *account;        // [C][4]
  uint8_t *flags;           // [C]
  uint32_t *astay;          // [C]
  uint32_t *nslot, *aslot;  // [mask + 1] each
  unsigned long long *sum;  // [mask + 1][4]
  uint64_t mask;            // S - 1
};

// what the screen compares against: the accepted roots (device, sorted as ledger_table.h sorts them)
// and the padding inputs
struct LedgerScreen {
  const uint64_t *roots;  // [nroots][4]
  uint32_t nroots, has_padding;
  uint64_t padding[16];
};

// the ledger's device counters: credited entries, accounts, the defensive error word
struct LedgerCounters {
  unsigned long long credited, accounts;
  uint32_t err, pad;
};

// qp_transfer_result as the kernels write it
struct LedgerResult {
  uint32_t status, verify_status;
  uint64_t number, first;
};

constexpr uint32_t LEDGER_BLOCK = 256;
inline uint32_t ledger_blocks(uint64_t n) { return (uint32_t)((n + LEDGER_BLOCK - 1) / LEDGER_BLOCK); }

// transfers pis[n][16], verdicts[n] (null: all verified): res[i] = the screen's result, numbered from
// first_number; blk[b] = the admitted of block b, b < ledger_blocks(n)
void ledger_screen(const LedgerScreen &sc, const uint64_t *pis, const uint32_t *verdicts, uint32_t n,
                   uint64_t first_number, LedgerResult *res, uint32_t *blk, hipStream_t s);
// blk[nb] into its exclusive prefix sums in place; *total = the sum.  One block.
void ledger_scan(uint32_t *blk, uint32_t nb, uint32_t *total, hipStream_t s);
// after screen and scan: the admitted transfers, in number order, into log [first_seq, first_seq + k), k =
// the scan's total (the caller read it back and keeps first_seq + k <= C); pos[j] = the batch position
// of entry first_seq + j
void ledger_pack(const LedgerDev &d, const uint64_t *pis, const LedgerResult *res, const uint32_t *blk, uint32_t n,
                 uint32_t first_seq, uint32_t *pos, hipStream_t s);
// log entries [first_seq, first_seq + k) into the nullifier table; stay[j] = the slot entry first_seq + j stopped at
void ledger_insert(const LedgerDev &d, uint32_t first_seq, uint32_t k, uint32_t *stay, LedgerCounters *ctr,
                   hipStream_t s);
// after ledger_insert, a launch of its own: res[pos[j]].first = the number of the entry that owns stay[j]'s
// slot; an owner is credited (flag, account table, limb sums, ctr), the others become double spends
void ledger_resolve(const LedgerDev &d, uint32_t first_seq, uint32_t k, const uint32_t *stay, const uint32_t *pos,
                    LedgerResult *res, LedgerCounters *ctr, hipStream_t s);
// reserve: the credited entries of the copied log [0, count) into fresh (all-empty, zero-sum) tables
void ledger_rebuild(const LedgerDev &d, uint32_t count, LedgerCounters *ctr, hipStream_t s);
// seq_out[i] = the log index of the credited entry with nullifier q[i][4] (device), or 0xFFFFFFFF.  Read-only;
// after every insert, resolve and rebuild on the same stream.
void ledger_find(const LedgerDev &d, uint32_t count, const uint64_t *q, uint32_t k, uint32_t *seq_out,
                 LedgerCounters *ctr, hipStream_t s);
// sums[i][4], found[i] of account q[i][4] (device).  Read-only, as ledger_find.
void ledger_totals(const LedgerDev &d, uint32_t count, const uint64_t *q, uint32_t k, unsigned long long *sums,
                   uint32_t *found, LedgerCounters *ctr, hipStream_t s);
// the payees: blk[b] = the entries of block b of log [0, count) that own their account slot
void ledger_payee_count(const LedgerDev &d, uint32_t count, uint32_t *blk, hipStream_t s);
// after ledger_payee_count and ledger_scan: payee[a] = the log index of the a-th such entry, in log order
void ledger_payee_write(const LedgerDev &d, uint32_t count, const uint32_t *blk, uint32_t *payee, hipStream_t s);
// payees [first, first + k) into dense arrays: the account, its sums, the log index
void ledger_payouts(const LedgerDev &d, const uint32_t *payee, uint32_t k, uint64_t *accounts,
                    unsigned long long *sums, uint64_t *first_seq, hipStream_t s);
// out[6] (zeroed by the caller) += credited, admitted, the four limb sums over the credited of log [0, count)
void ledger_recount(const LedgerDev &d, uint32_t count, unsigned long long *out, hipStream_t s);

// ---- the log commitment (ledger_log.h has the definitions): the leaves and the gather.  The levels
// above level 0, the paths and the prefix roots are the accumulator tree's (acc_kernels.h).
// bit of the error word: a number >= p in the log (cannot be reached; the leaf is not hashed)
constexpr uint32_t LEDGER_ERR_NUMBER = 16;
// log leaves [first, end) into level 0 of the digest buffer dig[seq][4]: leaf seq =
// hash_no_pad([nullifier[0..4], number, amount[0..4], account[0..4], flags]), 14 felts, two permutations
void ledger_leaves(const LedgerDev &d, uint32_t first, uint32_t end, uint64_t *dig, LedgerCounters *ctr,
                   hipStream_t s);
// log entries seq[i] < count (device; the caller checks the bound) into dense arrays [k][4], [k], [k][4],
// [k][4], [k]
void ledger_gather(const LedgerDev &d, const uint64_t *seq, uint32_t k, uint64_t *nullifier, uint64_t *number,
                   uint32_t *amount, uint64_t *account, uint8_t *flags, hipStream_t s);

// ---- the audit of a published log (ledger_audit.h has the rules).  The log is uploaded into a
// LedgerDev of its own with fresh tables; the whole-log insert is ledger_insert(d, 0, n, ...), the
// limb totals ledger_recount, the payees ledger_payee_count / ledger_scan / ledger_payee_write.
constexpr uint32_t LEDGER_AUDIT_NO_SEQ = 0xFFFFFFFFu;
struct LedgerAuditDev {
  unsigned long long credit_rule;  // the lowest offender << 32 | the lowest seq of its nullifier; ~0: none
  uint32_t non_canonical, order;   // the lowest offender; LEDGER_AUDIT_NO_SEQ: none
  uint32_t payout, pad;            // the lowest claimed payout that differs; LEDGER_AUDIT_NO_SEQ: none
  LedgerCounters ctr;              // entries with the credited bit, accounts they claim, the error word
};
// canonical felts, flags <= 1, numbers strictly increasing: the lowest offenders into rep
void ledger_audit_screen(const LedgerDev &d, uint32_t n, LedgerAuditDev *rep, hipStream_t s);
// after the whole-log insert, a launch of its own: the credit rule's lowest offender; every entry with the
// credited bit goes into the account table and adds its limbs to the account's sums
void ledger_audit_resolve(const LedgerDev &d, uint32_t n, const uint32_t *stay, LedgerAuditDev *rep, hipStream_t s);
// after ledger_payee_write, so a launch later than the one that adds the sums: claimed payout i < k
// (accounts [k][4], sums [k][4], first_seq [k], device) against payee[i]
void ledger_audit_payouts(const LedgerDev &d, const uint32_t *payee, uint32_t k, const uint64_t *accounts,
                          const uint64_t *sums, const uint64_t *first_seq, LedgerAuditDev *rep, hipStream_t s);
// A restore (ledger_audit.h) is the audit's launches over the new ledger's own LedgerDev, whose tables
// are sized for its capacity: ledger_audit_screen, ledger_insert(d, 0, n, ...), ledger_audit_resolve.
// What they leave (both tables, astay, the sums, rep->ctr's counts) is a live ledger's state.

// ---- payout rounds (ledger_rounds.h has the rule): the accounts credited by log entries [m0, m1).
// A round's view v: account, amount and flags point at entry m0 of a log (read only); aslot [mask + 1]
// (all empty), sum [mask + 1][4] (zero) and astay [k] are scratch of the call, mask + 1 = the power of
// two >= 2 k; nullifier, number and nslot are null and never touched.  Indices are j = seq - m0.
// every credited entry j < k into the view's account table, its limbs onto the slot's sums; *err |= 4 if
// a probe found no slot.  The owners and the rows come from ledger_payee_count / ledger_scan /
// ledger_payee_write / ledger_payouts over the same view, in later launches.
void ledger_round_credit(const LedgerDev &v, uint32_t k, uint32_t *err, hipStream_t s);

}  // namespace qpk
