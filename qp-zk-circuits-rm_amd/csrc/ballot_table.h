// ballot_table.h — the ballot box's semantics in plain C++ (no HIP): the
// public-input screen, the packing of a batch's admitted ballots, and the host
// path's nullifier table.  Included by ballot.cpp (both paths screen and pack
// with it; ctx == NULL counts with HostBox) and by the stand-alone check
// tools/ballot_host_check.cpp.
//
// A voting proof's 13 public inputs (voting/src/lib.rs:55-62):
//   proposal[0:4] root[4:8] vote[8] nullifier[9:13]
//
// The table (both paths): a slot table (slot_table.h) for a capacity of C
// admitted ballots; seq is a ballot's admission sequence number, the key
// log.nullifier[seq].
#pragma once
#include <stdint.h>
#include <string.h>
#include <vector>
#include "slot_table.h"

namespace qb {

using qst::canonical, qst::EMPTY, qst::MAX_CAPACITY, qst::NOT_FOUND, qst::P, qst::SlotTable, qst::table_slots;
constexpr uint32_t NPI = 13, PI_ROOT = 4, PI_VOTE = 8, PI_NULLIFIER = 9;
constexpr uint32_t MAX_ROOTS = 64;
constexpr uint8_t FLAG_VOTE = 1, FLAG_COUNTED = 2;

// qp_ballot_status (qpgpu.h), in the order of the checks
enum : uint32_t { COUNTED = 0, PROOF_REJECTED = 1, MALFORMED = 2, WRONG_PROPOSAL = 3, UNKNOWN_ROOT = 4, BAD_VOTE = 5,
                  DOUBLE_VOTE = 6 };

// qp_ballot_result
struct Result {
  uint32_t status, verify_status;
  uint64_t number, first;
};

// what a box accepts: one proposal, the published roots [nroots][4]
struct Screen {
  uint64_t proposal[4] = {0, 0, 0, 0};
  std::vector<uint64_t> roots;
  bool has_root(const uint64_t r[4]) const {
    for (size_t i = 0; i < roots.size(); i += 4)
      if (!memcmp(&roots[i], r, 32)) return true;
    return false;
  }
  // the first five checks, in order; COUNTED = admitted (the table decides the sixth)
  uint32_t check(const uint64_t pi[NPI], uint32_t verdict) const {
    if (verdict) return PROOF_REJECTED;
    if (!canonical(pi, NPI)) return MALFORMED;
    if (memcmp(pi, proposal, 32)) return WRONG_PROPOSAL;
    if (!has_root(pi + PI_ROOT)) return UNKNOWN_ROOT;
    if (pi[PI_VOTE] > 1) return BAD_VOTE;
    return COUNTED;
  }
};

// the admitted ballots of one batch, dense, in ballot-number order: what goes
// to log[count, count + k)
struct Packed {
  std::vector<uint64_t> nullifier, number;  // [k][4], [k]
  std::vector<uint8_t> flags;               // [k]: the vote bit
  std::vector<uint32_t> pos;                // [k]: position in the batch
  size_t size() const { return number.size(); }
};

// screens ballots pis[n][13] (verdicts may be null: all verified), numbers
// them from first_number, writes every result (an admitted one as COUNTED with
// first = its own number, for the table to settle) and packs the admitted
inline void screen_and_pack(const Screen &sc, const uint64_t *pis, const uint32_t *verdicts, uint32_t n,
                            uint64_t first_number, Result *out, Packed &pk) {
  pk.nullifier.clear();
  pk.number.clear();
  pk.flags.clear();
  pk.pos.clear();
  for (uint32_t i = 0; i < n; i++) {
    const uint64_t *pi = pis + (size_t)i * NPI;
    const uint32_t verdict = verdicts ? verdicts[i] : 0;
    const uint64_t num = first_number + i;
    out[i] = Result{sc.check(pi, verdict), verdict, num, num};
    if (out[i].status != COUNTED) continue;
    pk.nullifier.insert(pk.nullifier.end(), pi + PI_NULLIFIER, pi + PI_NULLIFIER + 4);
    pk.number.push_back(num);
    pk.flags.push_back(pi[PI_VOTE] ? FLAG_VOTE : 0);
    pk.pos.push_back(i);
  }
}

// The host path's box: the log and a sequential table of the layout above.
// Ballots arrive in number order, so the first of a nullifier claims its slot
// and every later one finds it: the lowest number wins by construction.
struct HostBox {
  uint64_t capacity = 0, mask = 0, yes = 0, no = 0;
  std::vector<uint32_t> slot;
  std::vector<uint64_t> nullifier, number;  // the log: [count][4], [count]
  std::vector<uint8_t> flags;               // [count]

  uint64_t count() const { return number.size(); }
  void open(uint64_t cap) {
    slot.assign(table_slots(cap), EMPTY);
    capacity = cap;
    mask = slot.size() - 1;
  }
  // the table over the log as it stands; a const box's is for lookup, which writes no slot
  SlotTable table() const { return {const_cast<uint32_t *>(slot.data()), mask, nullifier.data()}; }
  // one admitted ballot (the caller keeps count() < capacity): true if counted; *first as qp_ballot_result's
  bool admit(const uint64_t nul[4], uint64_t num, uint8_t vote_flag, uint64_t *first) {
    const uint32_t seq = (uint32_t)count();
    nullifier.insert(nullifier.end(), nul, nul + 4);
    number.push_back(num);
    flags.push_back(vote_flag);
    const uint32_t owner = slot[table().probe(seq)];
    *first = number[owner];
    if (owner != seq) return false;
    flags[seq] |= FLAG_COUNTED;
    (vote_flag & FLAG_VOTE ? yes : no)++;
    return true;
  }
  // settles a packed batch into out[] (screen_and_pack wrote the rest)
  void admit_packed(const Packed &pk, Result *out) {
    for (size_t j = 0; j < pk.size(); j++) {
      Result &r = out[pk.pos[j]];
      if (!admit(&pk.nullifier[j * 4], pk.number[j], pk.flags[j], &r.first)) r.status = DOUBLE_VOTE;
    }
  }
  // a table for new_capacity >= count(): the counted entries again (each nullifier has exactly one)
  void reserve(uint64_t new_capacity) {
    std::vector<uint32_t> fresh(table_slots(new_capacity), EMPTY);
    slot.swap(fresh);
    capacity = new_capacity;
    mask = slot.size() - 1;
    for (uint64_t seq = 0; seq < count(); seq++)
      if (flags[seq] & FLAG_COUNTED) table().probe((uint32_t)seq);
  }
  // the log index of the counted entry with nullifier q, NOT_FOUND if none
  uint64_t find(const uint64_t q[4]) const {
    const uint32_t seq = table().lookup(q);
    return seq == EMPTY ? NOT_FOUND : seq;
  }
  // yes, no, counted, admitted from the log's flags alone
  void recount(uint64_t out[4]) const {
    out[0] = out[1] = out[2] = 0;
    out[3] = count();
    for (uint8_t f : flags)
      if (f & FLAG_COUNTED) {
        out[f & FLAG_VOTE ? 0 : 1]++;
        out[2]++;
      }
  }
};

}  // namespace qb
