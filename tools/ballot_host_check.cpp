// ballot_host_check.cpp — the ballot box's host-only code (csrc/ballot_table.h:
// the screen, the pack step, the host table and its reserve) under the
// sanitizers, against a brute-force scan of the list of admitted ballots: the
// test streams' shapes (one nullifier, colliding home slots, a chain that
// wraps, felt-3-only differences, shuffled copies, screened ballots, growth)
// under several batchings, and capacities at both edges (1, exactly full, the
// slot count of 2^31).  A stand-alone CPU program; device code runs under no
// sanitizer.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/ballot_host_check.cpp -o ballot_host_check && ./ballot_host_check
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <array>
#include <random>
#include "../qp-zk-circuits-rm_amd/csrc/ballot_table.h"

using namespace qb;

#define CHECK(x)                                                     \
  do {                                                               \
    if (!(x)) {                                                      \
      fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #x); \
      exit(1);                                                       \
    }                                                                \
  } while (0)

typedef std::array<uint64_t, NPI> Pi;
struct Cast {
  Pi pi;
  uint32_t verdict;
};

static const uint64_t PROPOSAL[4] = {42, 1, 2, 3}, ROOT_A[4] = {11, 12, 13, P - 1}, ROOT_B[4] = {21, 22, 23, 24};

static Cast ballot(const uint64_t nul[4], uint64_t vote, const uint64_t *proposal = PROPOSAL,
                   const uint64_t *root = ROOT_A, uint32_t verdict = 0) {
  Cast c;
  for (int i = 0; i < 4; i++) {
    c.pi[i] = proposal[i];
    c.pi[PI_ROOT + i] = root[i];
    c.pi[PI_NULLIFIER + i] = nul[i];
  }
  c.pi[PI_VOTE] = vote;
  c.verdict = verdict;
  return c;
}

// the semantics by brute force: a scan of every earlier admitted ballot
struct Brute {
  Screen sc;
  std::vector<Result> results;
  std::vector<Pi> admitted;
  std::vector<uint64_t> number;
  std::vector<bool> counted;
  uint64_t yes = 0, no = 0;
  void cast(const Cast &c) {
    const uint64_t num = results.size();
    Result r{COUNTED, c.verdict, num, num};
    if (c.verdict) r.status = PROOF_REJECTED;
    else if (std::any_of(c.pi.begin(), c.pi.end(), [](uint64_t x) { return x >= P; })) r.status = MALFORMED;
    else if (!std::equal(PROPOSAL, PROPOSAL + 4, c.pi.begin())) r.status = WRONG_PROPOSAL;
    else if (!sc.has_root(&c.pi[PI_ROOT])) r.status = UNKNOWN_ROOT;
    else if (c.pi[PI_VOTE] > 1) r.status = BAD_VOTE;
    if (r.status == COUNTED) {
      for (size_t j = 0; j < admitted.size() && r.status == COUNTED; j++)
        if (std::equal(&c.pi[PI_NULLIFIER], &c.pi[PI_NULLIFIER] + 4, &admitted[j][PI_NULLIFIER])) {
          r.status = DOUBLE_VOTE;
          r.first = number[j];  // the earliest admitted one: it is the counted one
        }
      admitted.push_back(c.pi);
      number.push_back(num);
      counted.push_back(r.status == COUNTED);
      if (r.status == COUNTED) (c.pi[PI_VOTE] ? yes : no)++;
    }
    results.push_back(r);
  }
};

// casts the stream in batches of `batch` (0: whole) into a HostBox of `capacity`, growing it to
// reserve_to[i] once reserve_at[i] ballots were cast, and holds everything to the brute force
static void run(const std::vector<Cast> &stream, uint64_t capacity, size_t batch,
                const std::vector<std::pair<size_t, uint64_t>> &reserves = {}) {
  Screen sc;
  memcpy(sc.proposal, PROPOSAL, 32);
  sc.roots.assign(ROOT_A, ROOT_A + 4);
  sc.roots.insert(sc.roots.end(), ROOT_B, ROOT_B + 4);
  Brute br;
  br.sc = sc;
  HostBox box;
  box.open(capacity);
  CHECK(box.slot.size() >= 2 * capacity && (box.slot.size() & box.mask) == 0);
  Packed pk;
  std::vector<Result> out;
  std::vector<uint64_t> pis;
  std::vector<uint32_t> verdicts;
  size_t at = 0, next_reserve = 0;
  uint64_t cast = 0;
  while (at < stream.size()) {
    size_t end = std::min(stream.size(), batch ? at + batch : stream.size());
    if (next_reserve < reserves.size()) {
      if (reserves[next_reserve].first == at) {
        box.reserve(reserves[next_reserve].second);
        CHECK(box.capacity == reserves[next_reserve].second && box.slot.size() >= 2 * box.capacity);
        next_reserve++;
        continue;
      }
      end = std::min(end, reserves[next_reserve].first);
    }
    const uint32_t n = (uint32_t)(end - at);
    pis.clear();
    verdicts.clear();
    bool any = false;
    for (size_t i = at; i < end; i++) {
      pis.insert(pis.end(), stream[i].pi.begin(), stream[i].pi.end());
      verdicts.push_back(stream[i].verdict);
      any = any || stream[i].verdict;
      br.cast(stream[i]);
    }
    out.assign(n, Result{99, 99, 99, 99});
    screen_and_pack(sc, pis.data(), any ? verdicts.data() : nullptr, n, cast, out.data(), pk);
    CHECK(pk.size() == pk.pos.size() && pk.nullifier.size() == 4 * pk.size() && pk.flags.size() == pk.size());
    CHECK(box.count() + pk.size() <= box.capacity);  // the streams fit: the ABI refuses the others
    box.admit_packed(pk, out.data());
    cast += n;
    for (uint32_t i = 0; i < n; i++) {
      const Result &w = br.results[at + i], &g = out[i];
      CHECK(g.status == w.status && g.verify_status == w.verify_status && g.number == w.number && g.first == w.first);
    }
    at = end;
  }
  CHECK(box.yes == br.yes && box.no == br.no && box.count() == br.admitted.size());
  uint64_t rc[4];
  box.recount(rc);
  CHECK(rc[0] == br.yes && rc[1] == br.no && rc[2] == br.yes + br.no && rc[3] == box.count());
  for (size_t j = 0; j < br.admitted.size(); j++) {
    CHECK(!memcmp(&box.nullifier[4 * j], &br.admitted[j][PI_NULLIFIER], 32) && box.number[j] == br.number[j]);
    CHECK(((box.flags[j] & FLAG_COUNTED) != 0) == br.counted[j]);
    CHECK((box.flags[j] & FLAG_VOTE) == br.admitted[j][PI_VOTE]);
  }
  // every occupied slot holds a counted entry reachable from its home slot
  uint64_t occupied = 0;
  for (uint64_t s = 0; s < box.slot.size(); s++)
    if (box.slot[s] != EMPTY) {
      occupied++;
      CHECK(box.slot[s] < box.count() && (box.flags[box.slot[s]] & FLAG_COUNTED));
    }
  CHECK(occupied == br.yes + br.no);
}

static void run_all(const std::vector<Cast> &stream, uint64_t capacity,
                    const std::vector<std::pair<size_t, uint64_t>> &reserves = {}) {
  for (size_t batch : {(size_t)1, (size_t)7, (size_t)64, (size_t)0}) run(stream, capacity, batch, reserves);
}

int main() {
  std::mt19937_64 rng(7);
  auto felt = [&]() { return rng() % P; };
  auto fresh = [&](uint64_t *n) {
    for (int i = 0; i < 4; i++) n[i] = felt();
  };
  // the slot count: the power of two >= 2 C, from 1 to 2^31
  CHECK(table_slots(1) == 2 && table_slots(2) == 4 && table_slots(3) == 8 && table_slots(32) == 64);
  CHECK(table_slots(33) == 128 && table_slots(MAX_CAPACITY) == 1ull << 32 && table_slots(MAX_CAPACITY - 1) == 1ull << 32);
  CHECK(table_slots((1ull << 30) + 1) == 1ull << 32 && table_slots(1ull << 30) == 1ull << 31);
  uint64_t n[4], m[4];
  {  // capacity 1: one entry, two slots; the double needs a second entry
    fresh(n);
    run_all({ballot(n, 1)}, 1);
    run_all({ballot(n, 1), ballot(n, 0)}, 2);
  }
  {  // distinct, exactly full; then the same stream again: all doubles
    std::vector<Cast> s;
    for (int i = 0; i < 32; i++) {
      fresh(n);
      s.push_back(ballot(n, i & 1));
    }
    run_all(s, 32);
    std::vector<Cast> twice = s;
    twice.insert(twice.end(), s.begin(), s.end());
    run_all(twice, 64);
  }
  {  // one nullifier 64 times
    fresh(n);
    std::vector<Cast> s(64, ballot(n, 1));
    run_all(s, 64);
  }
  {  // 20 nullifiers with home slot S - 2 that differ in felt 1: the chain wraps; then each again
    std::vector<Cast> s;
    const uint64_t f0 = (felt() >> 24 << 7) | 126;
    for (int rep = 0; rep < 2; rep++)
      for (uint64_t i = 0; i < 20; i++) {
        const uint64_t k[4] = {f0, 1000 + i, 7, 7};
        s.push_back(ballot(k, i & 1));
      }
    run_all(s, 64);
  }
  {  // equal in felts 0..2, different in felt 3
    std::vector<Cast> s;
    fresh(n);
    for (uint64_t i = 0; i < 16; i++) {
      n[3] = i;
      s.push_back(ballot(n, 1));
    }
    run_all(s, 16);
  }
  {  // two nullifiers with one home slot, 30 copies each, shuffled; many nullifiers, four copies each
    std::vector<Cast> s;
    fresh(n);
    fresh(m);
    m[0] = (m[0] >> 24 << 7) | 5;
    n[0] = (n[0] >> 24 << 7) | 5;
    for (int i = 0; i < 30; i++) {
      s.push_back(ballot(n, i & 1));
      s.push_back(ballot(m, 1));
    }
    std::shuffle(s.begin(), s.end(), rng);
    run_all(s, 64);
    s.clear();
    for (int i = 0; i < 512; i++) {
      fresh(n);
      for (int c = 0; c < 4; c++) s.push_back(ballot(n, (i + c) & 1));
    }
    std::shuffle(s.begin(), s.end(), rng);
    run_all(s, 2048);
  }
  {  // screened ballots among good ones: every status, and the order of the checks
    const uint64_t other[4] = {42, 1, 2, 4}, unknown[4] = {11, 12, 13, P - 2};
    uint64_t g[4][4];
    for (auto &x : g) fresh(x);
    uint64_t badfelt[4] = {g[2][0], g[2][1], g[2][2], P};
    std::vector<Cast> s = {
        ballot(g[0], 1), ballot(g[1], 1, other), ballot(g[1], 0, PROPOSAL, ROOT_B), ballot(g[2], 1, PROPOSAL, unknown),
        ballot(g[2], 2), ballot(badfelt, 1), ballot(g[2], 1, PROPOSAL, ROOT_A, 9), ballot(g[2], 1),
        ballot(g[3], 2, other, unknown), ballot(g[3], 2, PROPOSAL, unknown), ballot(g[3], P, other, ROOT_A, 3),
        ballot(g[3], P, other), ballot(g[0], 0), ballot(g[3], ~0ull), ballot(g[3], 0), ballot(g[1], 1)};
    run_all(s, 16);
    run_all(s, 6);  // the admitted ones fill it exactly
  }
  {  // growth in mid-stream, doubles of pre-reserve ballots after each reserve, down to a table that is half full
    std::vector<std::array<uint64_t, 4>> g(100);
    for (auto &x : g) fresh(x.data());
    std::vector<Cast> s;
    auto b = [&](int i) { s.push_back(ballot(g[i].data(), i & 1)); };
    for (int i = 0; i < 24; i++) b(i);
    b(3), b(3);
    const size_t r1 = s.size();
    for (int i : {0, 23, 24, 25, 5}) b(i);
    for (int i = 26; i < 50; i++) b(i);
    const size_t r2 = s.size();
    for (int i : {1, 24, 49, 50}) b(i);
    for (int i = 51; i < 100; i++) b(i);
    b(99), b(0);
    run_all(s, 32, {{r1, 64}, {r2, 128}});
    run_all(s, 26, {{r1, 55}, {r2, s.size()}});  // reserves to exactly what is needed
  }
  printf("ballot_host_check: ok\n");
  return 0;
}
