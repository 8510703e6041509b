// claims_kernels.h — argument layouts and launchers of claims.hip: the leaves,
// the grand total and the totals' gather of a payout claims commitment on the
// device (claims.h has the definitions).  One launcher per step; the launcher
// owns the grid and block sizes.  The credit of the range and the owners'
// compaction are the payout round's (ledger_kernels.h), the sort, the search
// and the record gather the nullifier set's (nullifier_set_kernels.h) with the
// log's account column as the key column: a record is (account, j), j = seq -
// m0 the local index of the account's first credited entry of the range.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ledger_kernels.h"
#include "nullifier_set_kernels.h"

namespace qpk {

// bits of the claims' defensive error word (cannot be reached): a record names an entry outside the
// range; an entry's astay names no slot of the view's table
constexpr uint32_t CLAIMS_ERR_ENTRY = 1, CLAIMS_ERR_SLOT = 2;

// Sorted records [0, a) of the view v (a payout round's, credited: v.astay [k], v.sum [mask + 1][4]):
// totals[j][5] = the five-limb total of record j's account, and claim leaf j =
// hash_no_pad([account[0..4], t[0..5], m0 + j_entry, 3]) into dig[j][4] (level 0 of the claims tree).
// An index out of its bound sets *err and writes nothing.
void claims_leaves(const NsetRecs &recs, uint32_t a, const LedgerDev &v, uint32_t k, uint64_t m0, uint32_t *totals,
                   uint64_t *dig, uint32_t *err, hipStream_t s);
// out[4] (zeroed by the caller) += the four limb sums of the accounts that own entries entry[0..a)
// (each below k); an index out of its bound sets *err and adds nothing
void claims_total(const uint32_t *entry, uint32_t a, const LedgerDev &v, uint32_t k, unsigned long long *out,
                  uint32_t *err, hipStream_t s);
// out[i][5] = totals[idx[i]][5], idx[i] < a (device; the caller checks the bound), i < n
void claims_gather_totals(const uint32_t *totals, const uint64_t *idx, uint32_t n, uint32_t *out, hipStream_t s);

}  // namespace qpk
