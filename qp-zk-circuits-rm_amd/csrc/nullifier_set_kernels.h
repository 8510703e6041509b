// nullifier_set_kernels.h — argument layouts and launchers of
// nullifier_set.hip: the sorted nullifier set of a log on the device
// (nullifier_set.h has the definitions).  One launcher per step; the launcher
// owns the grid and block sizes.
//
// A record is 36 bytes, kept as two columns: key[m][4] (the nullifier) and
// seq[m] (the log index, below 2^31).  The order is qns::rec_less, the full
// five-word order, in every kernel.
//
// The sort: NSET_TILE records per workgroup are sorted in LDS (bitonic), then
// ceil(log2(runs)) merge passes ping-pong between two record buffers.  In a
// merge pass every output element finds its own co-ranks (a merge-path search
// over the two runs of its pair, bounded by 32 halvings); the runs of a pair
// are disjoint and (key, seq) is unique, so there are no ties.  An unpaired
// last run is copied.  Every index comes from counts the host computed: n, m
// and the run length.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace qpk {

// records per tile: 36 KiB of LDS per workgroup of 256 lanes, so four workgroups (16 waves, 4 per
// SIMD) share a CU's 160 KiB
constexpr uint32_t NSET_TILE = 1024;
constexpr uint32_t NSET_NO_SEQ = 0xFFFFFFFFu;  // no duplicate (seqs stay below 2^31)

// one record buffer: m records
struct NsetRecs {
  uint64_t *key;  // [m][4]
  uint32_t *seq;  // [m]
};

// the members of log [0, n): blk[b] = the entries of block b with flags[seq] & mask, b < ledger_blocks(n)
void nset_select_count(const uint8_t *flags, uint32_t n, uint8_t mask, uint32_t *blk, hipStream_t s);
// after nset_select_count and ledger_scan: sel[a] = the log index of the a-th member, in log order
// (the caller sized sel[] for n)
void nset_select_write(const uint8_t *flags, uint32_t n, uint8_t mask, const uint32_t *blk, uint32_t *sel,
                       hipStream_t s);
// out[j], j < m: the records (nullifier[sel[j]], sel[j]), each tile of NSET_TILE sorted
void nset_tile_sort(const uint64_t *nullifier, const uint32_t *sel, uint32_t m, const NsetRecs &out, hipStream_t s);
// one merge pass: src holds sorted runs of `run` records (the last may be shorter); dst[0, m) = the
// runs merged in pairs, an unpaired last run copied
void nset_merge(const NsetRecs &src, const NsetRecs &dst, uint32_t m, uint32_t run, hipStream_t s);
// recs sorted: *dup (set to NSET_NO_SEQ by the caller) = the lowest seq whose predecessor has an equal key
void nset_duplicates(const NsetRecs &recs, uint32_t m, uint32_t *dup, hipStream_t s);
// the set leaves of positions [0, m) into dig[j][4] (level 0 of the set tree)
void nset_leaves(const NsetRecs &recs, uint32_t m, uint64_t *dig, hipStream_t s);
// per query key q[i][4] (device), i < k: pos[i] = the number of keys below it, found[i] = the key at pos[i] equals it
void nset_search(const NsetRecs &recs, uint32_t m, const uint64_t *q, uint32_t k, uint32_t *pos, uint32_t *found,
                 hipStream_t s);
// the records at positions idx[i] < m (device; the caller checks the bound), i < k, into key_out [k][4], seq_out [k]
void nset_gather(const NsetRecs &recs, const uint64_t *idx, uint32_t k, uint64_t *key_out, uint64_t *seq_out,
                 hipStream_t s);

}  // namespace qpk
