// slot_table_device.h — the slot table (slot_table.h has the layout and the
// home-slot rule) on the device, as the ballot box's and the transfer ledger's
// kernel files share it: the claiming probe, the read-only probe, and the
// block- and wave-wide helpers of their kernels.  Device code for blocks of 256
// lanes (gfx950).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "field.h"
#include "slot_table.h"

namespace qpk {

static_assert(qst::P == gl::P, "one modulus");
constexpr uint32_t SLOT_EMPTY = qst::EMPTY;  // a slot that holds no seq
constexpr uint32_t NO_SLOT = 0xFFFFFFFFu;    // stay[] of a lane whose probe ran out (defensive)

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

// The probe of log entry seq's key (the log holds `limit` entries; only seqs below it are ever
// stored): returns the slot where it stays, NO_SLOT if S slots were tried (see fact 3 below);
// *claimed = this lane took an empty slot.
//
// Why the table is correct:
// 1. A slot's key never changes once the slot is claimed: a claimed slot holds a seq, and the only
//    later write to it is an atomicMin by a lane whose own key equals keys[seq], so the word only
//    ever moves to another entry with the same key.  A lane passes a slot only if the key there
//    differs from its own, which therefore stays true.  So all entries with one key probe the same
//    chain and stop at the same slot whatever the interleaving, and the slot ends at the minimum of
//    their seqs: the lowest ballot or transfer number, since seq is monotone in the number.
// 2. The keys a lane compares against are in the log, which was written before this launch (by the
//    host's upload or by a pack kernel; entries of this batch included).  A lane reads nothing that
//    a lane of the same launch wrote, except the slot word, and that only through agent-scope
//    atomics (load, compare-and-swap, min), which are performed at the device's coherence point and
//    not in an XCD's own L2.  That is why the key is not stored in the slot: a plain load does not
//    see another XCD's plain store of the same launch.  No fences, no flags, no spin: no lane waits
//    on another lane.
// 3. The host keeps count + k <= C <= S / 2 before it launches, so an empty slot exists and the loop
//    ends at it at the latest.  The loop is bounded by S all the same; running out cannot be reached
//    and is reported through the error word, after which the owner refuses further casts.
// 4. The lookup (table_lookup) takes no atomics and writes no slot.  It runs on the owner's stream
//    in a launch of its own after every insert, resolve and rebuild has completed, and nothing runs
//    beside it: the slot words and the log it reads were final before it started, and a kernel
//    boundary on one stream makes them visible to plain loads on every XCD.  Nothing is ever
//    removed, so a chain has no gap and an empty slot ends it.
__device__ __forceinline__ uint32_t table_probe(const SlotTable &t, uint32_t seq, uint32_t limit, bool *claimed) {
  uint64_t k[4];
  load_key(t.keys + (uint64_t)seq * 4, k);
  *claimed = false;
  uint64_t at = k[0] & t.mask;
  for (uint64_t tried = 0; tried <= t.mask; tried++, at = (at + 1) & t.mask) {
    uint32_t cur = __hip_atomic_load(t.slot + at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == SLOT_EMPTY) {
      cur = atomicCAS(t.slot + at, SLOT_EMPTY, seq);
      if (cur == SLOT_EMPTY) {
        *claimed = true;
        return (uint32_t)at;
      }
    }
    if (cur == seq) return (uint32_t)at;
    if (cur >= limit) break;  // not a log entry: cannot be reached
    uint64_t o[4];
    load_key(t.keys + (uint64_t)cur * 4, o);  // cur < limit <= C, written before the launch
    if (qst::key_equal(o, k)) {
      atomicMin(t.slot + at, seq);
      return (uint32_t)at;
    }
  }
  return NO_SLOT;
}

// the read-only probe (fact 4) of key k in a table whose log holds `count` entries: the slot that
// holds an entry with that key, or NO_SLOT; a slot word at or beyond count sets *bad
__device__ __forceinline__ uint32_t table_lookup(const SlotTable &t, const uint64_t k[4], uint32_t count, bool *bad) {
  uint64_t at = k[0] & t.mask;
  for (uint64_t tried = 0; tried <= t.mask; tried++, at = (at + 1) & t.mask) {
    const uint32_t cur = t.slot[at];
    if (cur == SLOT_EMPTY) break;
    if (cur >= count) {
      *bad = true;
      break;
    }
    uint64_t o[4];
    load_key(t.keys + (uint64_t)cur * 4, o);
    if (qst::key_equal(o, k)) return (uint32_t)at;
  }
  return NO_SLOT;
}

// adds N per-lane predicates over the block into N 64-bit counters: a wave
// ballot and popcount each, the waves' counts through LDS, one integer atomic
// per counter and block (integer sums are order-independent).  Every lane of
// the block calls it.
template <int N>
__device__ __forceinline__ void block_count(const bool (&pred)[N], unsigned long long *const (&dst)[N]) {
  __shared__ uint32_t sh[4][N];
  const uint32_t wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < N; j++) {
    const uint32_t n = __popcll(__ballot(pred[j]));
    if ((threadIdx.x & 63) == 0) sh[wave][j] = n;
  }
  __syncthreads();
  if (threadIdx.x < N) {
    const uint32_t t = sh[0][threadIdx.x] + sh[1][threadIdx.x] + sh[2][threadIdx.x] + sh[3][threadIdx.x];
    if (t) atomicAdd(dst[threadIdx.x], (unsigned long long)t);
  }
}

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

// true in the lowest lane of the wave whose `bad` is set; every lane of the wave calls it.  Where
// seqs are consecutive across a wave, that lane holds the wave's lowest offending seq and alone
// sends it: one atomicMin per wave and reason at the most, and the minimum over the waves does not
// depend on the order they arrive in.
__device__ __forceinline__ bool lowest_offender(bool bad) {
  const uint64_t m = __ballot(bad);
  return bad && (threadIdx.x & 63) == (uint32_t)(__ffsll((unsigned long long)m) - 1);
}

}  // namespace qpk
