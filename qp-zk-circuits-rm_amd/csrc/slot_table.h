// slot_table.h — the table the ballot box and the transfer ledger both stand
// on, in plain C++ (no HIP): its layout, the home-slot rule and the sequential
// table of the host paths.  slot_table_device.h has the concurrent probes over
// the same layout and the argument why they are correct.
//
// The table: open addressing, linear probing, S = table_slots(C) slots for a
// capacity of C log entries, S the power of two >= 2 C.  A slot is a uint32_t:
// the log index `seq` of an entry, or EMPTY.  The key, four felts, is not in the
// slot: it is keys[seq][4], a column of the log (a ballot's nullifier; a
// transfer's nullifier or its exit account).
//   HOME SLOT = key[0] & (S - 1)
// and the probe goes to slot + 1, wrapping.  All entries of one key stop at one
// slot, and the slot ends at the lowest seq among them.  Nothing is ever
// removed, so a chain has no gap and an empty slot ends it.  A key is a Poseidon
// output, so nobody chooses theirs; tests craft colliding ones from this rule.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define QST_HD __host__ __device__
#else
#define QST_HD
#endif

namespace qst {

constexpr uint64_t P = 0xFFFFFFFF00000001ull;  // the Goldilocks modulus (slot_table_device.h holds it equal to gl::P)
constexpr uint64_t MAX_CAPACITY = 1ull << 31;
constexpr uint32_t EMPTY = 0xFFFFFFFFu;
constexpr uint64_t NOT_FOUND = ~0ull;

inline uint64_t table_slots(uint64_t capacity) {
  uint64_t s = 2;
  while (s < 2 * capacity) s <<= 1;
  return s;
}
inline bool canonical(const uint64_t *v, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (v[i] >= P) return false;
  return true;
}
QST_HD inline bool key_equal(const uint64_t *a, const uint64_t *b) {
  return a[0] == b[0] && a[1] == b[1] && a[2] == b[2] && a[3] == b[3];
}

// The host paths' table: a view of slot words and the key column they index.  Entries arrive in seq
// order, so the first of a key claims its slot and every later one finds it: the lowest seq owns the
// slot by construction.  The view holds raw pointers: make one per use, never across a push_back.
struct SlotTable {
  uint32_t *slot;        // [mask + 1]
  uint64_t mask;         // S - 1
  const uint64_t *keys;  // [count][4]

  // the slot of entry seq's key: its own (claimed now) or an equal earlier entry's
  uint64_t probe(uint32_t seq) const {
    const uint64_t *k = keys + (size_t)seq * 4;
    for (uint64_t at = k[0] & mask;; at = (at + 1) & mask) {  // count <= C <= S / 2: an empty slot exists
      if (slot[at] == EMPTY) slot[at] = seq;
      if (slot[at] == seq || !memcmp(keys + (size_t)slot[at] * 4, k, 32)) return at;
    }
  }
  // the read-only probe: the entry that key k's chain holds (*at_out = its slot), or EMPTY.  Bounded by S.
  uint32_t lookup(const uint64_t k[4], uint64_t *at_out = nullptr) const {
    uint64_t at = k[0] & mask;
    for (uint64_t tried = 0; tried <= mask; tried++, at = (at + 1) & mask) {
      const uint32_t cur = slot[at];
      if (cur == EMPTY) return EMPTY;
      if (!memcmp(keys + (size_t)cur * 4, k, 32)) {
        if (at_out) *at_out = at;
        return cur;
      }
    }
    return EMPTY;
  }
};

}  // namespace qst
