// ledger_table.h — the transfer ledger's semantics in plain C++: the screen of
// a Wormhole proof's public inputs, the packing of a batch's admitted
// transfers, and the host path's two tables and account sums.  Included by
// ledger.cpp (ctx == NULL settles with HostLedger), by ledger.hip (the device
// screen calls screen_check and root_index, so both paths run one statement of
// the checks) and by the stand-alone check tools/ledger_host_check.cpp.
//
// A Wormhole proof's 16 public inputs (wormhole/circuit/src/inputs.rs:12-19,92-97):
//   nullifier[0:4] root_hash[4:8] funding_amount[8:12] exit_account[12:16]
// funding_amount is four 32-bit limbs, most significant first (felts_to_u128).
//
// Two slot tables (slot_table.h; both paths), each for a capacity of C admitted
// transfers.  The nullifier table takes every admitted entry and its slot ends
// at the lowest seq of that nullifier: the credited one.  The account table
// takes the credited entries and its slot ends at the lowest seq credited to
// that account; sum[slot][4] holds the account's four limb sums.
#pragma once
#include <stdint.h>
#include <string.h>
#include <vector>
#include "slot_table.h"

#define QL_HD QST_HD

namespace ql {

using qst::canonical, qst::EMPTY, qst::key_equal, qst::MAX_CAPACITY, qst::NOT_FOUND, qst::P, qst::SlotTable,
    qst::table_slots;
constexpr uint32_t NPI = 16, PI_NULLIFIER = 0, PI_ROOT = 4, PI_AMOUNT = 8, PI_ACCOUNT = 12;
constexpr uint32_t MAX_ROOTS = 4096;
constexpr uint32_t MAX_BATCH = 1u << 22;  // transfers per cast call
constexpr uint8_t FLAG_CREDITED = 1;

// qp_transfer_status (qpgpu.h), in the order of the checks
enum : uint32_t { CREDITED = 0, PROOF_REJECTED = 1, MALFORMED = 2, PADDING = 3, BAD_AMOUNT = 4, UNKNOWN_ROOT = 5,
                  DOUBLE_SPEND = 6 };

// qp_transfer_result
struct Result {
  uint32_t status, verify_status;
  uint64_t number, first;
};

// four felts as a key: the order the accepted roots are sorted in (felt 0 first)
QL_HD inline int key_compare(const uint64_t *a, const uint64_t *b) {
  for (int i = 0; i < 4; i++)
    if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
  return 0;
}
// Four limb sums name the total sum of s[i] << (96 - 32 i).  Two sets name one total iff their
// carry-propagated forms are equal: limbs 3..1 reduced to 32 bits, the carries moved up, and the top
// word with its carry-out.  The audit compares claimed sums with the log's this way, so a claim may
// give an exact total in any split.
QL_HD inline bool sums_equal(const uint64_t *a, const uint64_t *b) {
  uint64_t ca = 0, cb = 0;
  for (int i = 3; i >= 1; i--) {
    const uint64_t ta = a[i] + ca, tb = b[i] + cb;  // a carry is below 2^34: t < carry iff the sum wrapped
    if ((ta & 0xFFFFFFFFull) != (tb & 0xFFFFFFFFull)) return false;
    ca = (ta >> 32) | ((uint64_t)(ta < ca) << 32);
    cb = (tb >> 32) | ((uint64_t)(tb < cb) << 32);
  }
  const uint64_t ta = a[0] + ca, tb = b[0] + cb;
  return ta == tb && (ta < ca) == (tb < cb);
}
// roots [n][4] sorted by key_compare, each held once: the position of r, or of the first root above it
QL_HD inline uint32_t root_lower_bound(const uint64_t *roots, uint32_t n, const uint64_t *r) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (key_compare(roots + (size_t)mid * 4, r) < 0) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}
QL_HD inline bool has_root(const uint64_t *roots, uint32_t n, const uint64_t *r) {
  const uint32_t at = root_lower_bound(roots, n, r);
  return at < n && key_equal(roots + (size_t)at * 4, r);
}

// the first five checks, in order; CREDITED = admitted (the nullifier table decides the sixth).
// padding: the ledger's 16 padding inputs, or null
QL_HD inline uint32_t screen_check(const uint64_t *pi, uint32_t verdict, const uint64_t *roots, uint32_t nroots,
                                   const uint64_t *padding) {
  if (verdict) return PROOF_REJECTED;
  for (uint32_t i = 0; i < NPI; i++)
    if (pi[i] >= P) return MALFORMED;
  if (padding) {
    bool same = true;
    for (uint32_t i = 0; i < NPI; i++) same = same && pi[i] == padding[i];
    if (same) return PADDING;
  }
  for (uint32_t i = 0; i < 4; i++)
    if (pi[PI_AMOUNT + i] >> 32) return BAD_AMOUNT;
  if (!has_root(roots, nroots, pi + PI_ROOT)) return UNKNOWN_ROOT;
  return CREDITED;
}

// what a ledger accepts: the known storage roots (sorted, the form the device searches), the padding inputs
struct Screen {
  std::vector<uint64_t> roots;  // [nroots][4], sorted by key_compare
  bool has_padding = false;
  uint64_t padding[NPI] = {};
  uint32_t nroots() const { return (uint32_t)(roots.size() / 4); }
  bool accepts(const uint64_t r[4]) const { return has_root(roots.data(), nroots(), r); }
  void add_root(const uint64_t r[4]) {  // the caller checked !accepts(r)
    const uint32_t at = root_lower_bound(roots.data(), nroots(), r);
    roots.insert(roots.begin() + (size_t)at * 4, r, r + 4);
  }
  uint32_t check(const uint64_t pi[NPI], uint32_t verdict) const {
    return screen_check(pi, verdict, roots.data(), nroots(), has_padding ? padding : nullptr);
  }
};

// the admitted transfers of one batch, dense, in number order: what goes to log[count, count + k)
struct Packed {
  std::vector<uint64_t> nullifier, number, account;  // [k][4], [k], [k][4]
  std::vector<uint32_t> amount;                      // [k][4]: the limbs, most significant first
  std::vector<uint32_t> pos;                         // [k]: position in the batch
  size_t size() const { return number.size(); }
  void clear() {
    nullifier.clear(), number.clear(), account.clear(), amount.clear(), pos.clear();
  }
};

// screens transfers pis[n][16] (verdicts may be null: all verified), numbers them from first_number,
// writes every result (an admitted one as CREDITED with first = its own number, for the table to
// settle) and packs the admitted
inline void screen_and_pack(const Screen &sc, const uint64_t *pis, const uint32_t *verdicts, uint32_t n,
                            uint64_t first_number, Result *out, Packed &pk) {
  pk.clear();
  for (uint32_t i = 0; i < n; i++) {
    const uint64_t *pi = pis + (size_t)i * NPI;
    const uint32_t verdict = verdicts ? verdicts[i] : 0;
    const uint64_t num = first_number + i;
    out[i] = Result{sc.check(pi, verdict), verdict, num, num};
    if (out[i].status != CREDITED) continue;
    pk.nullifier.insert(pk.nullifier.end(), pi + PI_NULLIFIER, pi + PI_NULLIFIER + 4);
    pk.account.insert(pk.account.end(), pi + PI_ACCOUNT, pi + PI_ACCOUNT + 4);
    for (uint32_t j = 0; j < 4; j++) pk.amount.push_back((uint32_t)pi[PI_AMOUNT + j]);
    pk.number.push_back(num);
    pk.pos.push_back(i);
  }
}

// The host path's ledger: the log, the two sequential tables, the account sums.  Transfers arrive in
// number order, so the first of a nullifier claims its slot and every later one finds it: the lowest
// number is credited by construction, and an account's slot is claimed by its first credited entry.
struct HostLedger {
  uint64_t capacity = 0, mask = 0, credited = 0;
  std::vector<uint32_t> nslot, aslot;  // [S]: the nullifier table, the account table
  std::vector<uint64_t> sum;           // [S][4]: limb sums of the account whose slot it is
  // the log: [count][4], [count], [count][4], [count][4], [count]
  std::vector<uint64_t> nullifier, number, account;
  std::vector<uint32_t> amount;
  std::vector<uint8_t> flags;
  std::vector<uint32_t> astay;  // [count]: the account slot of a credited entry
  std::vector<uint32_t> payee;  // the entries that own an account slot, in log order: one per account

  uint64_t count() const { return number.size(); }
  uint64_t accounts() const { return payee.size(); }
  void open(uint64_t cap) {
    const uint64_t S = table_slots(cap);
    nslot.assign(S, EMPTY);
    aslot.assign(S, EMPTY);
    sum.assign(S * 4, 0);
    capacity = cap;
    mask = S - 1;
  }
  // the two tables over the log as it stands; a const ledger's are for lookup, which writes no slot
  SlotTable ntable() const { return {const_cast<uint32_t *>(nslot.data()), mask, nullifier.data()}; }
  SlotTable atable() const { return {const_cast<uint32_t *>(aslot.data()), mask, account.data()}; }
  void credit(uint32_t seq) {
    const uint64_t at = atable().probe(seq);
    astay[seq] = (uint32_t)at;
    for (int j = 0; j < 4; j++) sum[at * 4 + j] += amount[(size_t)seq * 4 + j];
  }
  // one admitted transfer (the caller keeps count() < capacity): true if credited; *first as qp_transfer_result's
  bool admit(const uint64_t nul[4], uint64_t num, const uint32_t amt[4], const uint64_t acc[4], uint64_t *first) {
    const uint32_t seq = (uint32_t)count();
    nullifier.insert(nullifier.end(), nul, nul + 4);
    account.insert(account.end(), acc, acc + 4);
    amount.insert(amount.end(), amt, amt + 4);
    number.push_back(num);
    flags.push_back(0);
    astay.push_back(EMPTY);
    const uint32_t owner = nslot[ntable().probe(seq)];
    *first = number[owner];
    if (owner != seq) return false;
    flags[seq] |= FLAG_CREDITED;
    credited++;
    credit(seq);
    if (aslot[astay[seq]] == seq) payee.push_back(seq);
    return true;
  }
  // settles a packed batch into out[] (screen_and_pack wrote the rest)
  void admit_packed(const Packed &pk, Result *out) {
    for (size_t j = 0; j < pk.size(); j++) {
      Result &r = out[pk.pos[j]];
      if (!admit(&pk.nullifier[j * 4], pk.number[j], &pk.amount[j * 4], &pk.account[j * 4], &r.first))
        r.status = DOUBLE_SPEND;
    }
  }
  // tables for new_capacity >= count(): both tables and the sums again from the credited entries
  void reserve(uint64_t new_capacity) {
    const uint64_t S = table_slots(new_capacity);
    std::vector<uint32_t> n2(S, EMPTY), a2(S, EMPTY);
    std::vector<uint64_t> s2(S * 4, 0);
    nslot.swap(n2);
    aslot.swap(a2);
    sum.swap(s2);
    capacity = new_capacity;
    mask = S - 1;
    for (uint64_t seq = 0; seq < count(); seq++)
      if (flags[seq] & FLAG_CREDITED) {
        ntable().probe((uint32_t)seq);
        credit((uint32_t)seq);
      }
  }
  uint64_t find(const uint64_t nul[4]) const {
    const uint32_t seq = ntable().lookup(nul);
    return seq == EMPTY ? NOT_FOUND : seq;
  }
  bool total_for(const uint64_t acc[4], uint64_t sums[4]) const {
    uint64_t at = 0;
    const bool found = atable().lookup(acc, &at) != EMPTY;
    for (int j = 0; j < 4; j++) sums[j] = found ? sum[at * 4 + j] : 0;
    return found;
  }
  // credited, admitted and the four limb sums over the credited entries, from the log alone
  void recount(uint64_t out[6]) const {
    memset(out, 0, 48);
    out[1] = count();
    for (uint64_t seq = 0; seq < count(); seq++)
      if (flags[seq] & FLAG_CREDITED) {
        out[0]++;
        for (int j = 0; j < 4; j++) out[2 + j] += amount[seq * 4 + j];
      }
  }
};

}  // namespace ql
