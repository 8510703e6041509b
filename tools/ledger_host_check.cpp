// ledger_host_check.cpp — the transfer ledger's host-only code (csrc/ledger_table.h:
// the screen with its sorted roots, the pack step, the two host tables, the
// limb sums, reserve, the lookups) under the sanitizers, against a brute-force
// scan of the list of admitted transfers: the test streams' shapes (one
// nullifier, colliding home slots in either table, a chain that wraps,
// felt-3-only differences, shuffled copies, screened transfers, padding, the
// largest amounts, growth at exactly-full capacity) under several batchings.
// A stand-alone CPU program; device code runs under no sanitizer.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/ledger_host_check.cpp -o ledger_host_check && ./ledger_host_check
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <array>
#include <random>
#include "../qp-zk-circuits-rm_amd/csrc/ledger_table.h"

using namespace ql;

#define CHECK(x)                                                     \
  do {                                                               \
    if (!(x)) {                                                      \
      fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #x); \
      exit(1);                                                       \
    }                                                                \
  } while (0)

typedef std::array<uint64_t, NPI> Pi;
typedef std::array<uint64_t, 4> Key;
struct Cast {
  Pi pi;
  uint32_t verdict;
};

static const Key ROOT_A = {11, 12, 13, P - 1}, ROOT_B = {21, 22, 23, 24}, ROOT_UNKNOWN = {11, 12, 13, P - 2};
static const Key ACC = {5, 6, 7, 8};
static const Key FULL = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};

static Cast transfer(const Key &nul, const Key &limbs, const Key &account = ACC, const Key &root = ROOT_A,
                     uint32_t verdict = 0) {
  Cast c;
  for (int i = 0; i < 4; i++) {
    c.pi[PI_NULLIFIER + i] = nul[i];
    c.pi[PI_ROOT + i] = root[i];
    c.pi[PI_AMOUNT + i] = limbs[i];
    c.pi[PI_ACCOUNT + i] = account[i];
  }
  c.verdict = verdict;
  return c;
}

// the semantics by brute force: linear scans of the roots, of every earlier admitted transfer, of the accounts
struct Brute {
  std::vector<Key> roots;
  bool has_padding = false;
  Pi padding;
  std::vector<Result> results;
  std::vector<Pi> admitted;
  std::vector<uint64_t> number;
  std::vector<bool> credited;
  std::vector<Key> accounts;  // in the order of their first credit
  std::vector<std::array<uint64_t, 4>> sums;
  std::vector<uint64_t> first_seq;
  void cast(const Cast &c) {
    const uint64_t num = results.size();
    Result r{CREDITED, c.verdict, num, num};
    const Key root = {c.pi[4], c.pi[5], c.pi[6], c.pi[7]};
    if (c.verdict) r.status = PROOF_REJECTED;
    else if (std::any_of(c.pi.begin(), c.pi.end(), [](uint64_t x) { return x >= P; })) r.status = MALFORMED;
    else if (has_padding && c.pi == padding) r.status = PADDING;
    else if (std::any_of(c.pi.begin() + 8, c.pi.begin() + 12, [](uint64_t x) { return x > 0xFFFFFFFFull; })) r.status = BAD_AMOUNT;
    else if (std::find(roots.begin(), roots.end(), root) == roots.end()) r.status = UNKNOWN_ROOT;
    if (r.status == CREDITED) {
      for (size_t j = 0; j < admitted.size() && r.status == CREDITED; j++)
        if (std::equal(c.pi.begin(), c.pi.begin() + 4, admitted[j].begin())) {
          r.status = DOUBLE_SPEND;
          r.first = number[j];  // the earliest admitted one: it is the credited one
        }
      if (r.status == CREDITED) {
        const Key acc = {c.pi[12], c.pi[13], c.pi[14], c.pi[15]};
        size_t a = std::find(accounts.begin(), accounts.end(), acc) - accounts.begin();
        if (a == accounts.size()) {
          accounts.push_back(acc);
          sums.push_back({0, 0, 0, 0});
          first_seq.push_back(admitted.size());
        }
        for (int j = 0; j < 4; j++) sums[a][j] += c.pi[PI_AMOUNT + j];
      }
      admitted.push_back(c.pi);
      number.push_back(num);
      credited.push_back(r.status == CREDITED);
    }
    results.push_back(r);
  }
};

// everything the ledger answers, against the brute force
static void compare(const HostLedger &led, const Brute &br) {
  CHECK(led.count() == br.admitted.size() && led.accounts() == br.accounts.size());
  CHECK(led.credited == (uint64_t)std::count(br.credited.begin(), br.credited.end(), true));
  CHECK(led.nslot.size() >= 2 * led.capacity && (led.nslot.size() & led.mask) == 0 && led.count() <= led.capacity);
  uint64_t grand[4] = {0, 0, 0, 0};
  for (size_t j = 0; j < br.admitted.size(); j++) {
    const Pi &pi = br.admitted[j];
    CHECK(!memcmp(&led.nullifier[4 * j], &pi[PI_NULLIFIER], 32) && !memcmp(&led.account[4 * j], &pi[PI_ACCOUNT], 32));
    CHECK(led.number[j] == br.number[j] && ((led.flags[j] & FLAG_CREDITED) != 0) == br.credited[j]);
    for (int i = 0; i < 4; i++) CHECK(led.amount[4 * j + i] == pi[PI_AMOUNT + i]);
    // find: the first admitted entry with this nullifier
    size_t first = 0;
    while (!std::equal(pi.begin(), pi.begin() + 4, br.admitted[first].begin())) first++;
    CHECK(led.find(&pi[PI_NULLIFIER]) == first);
  }
  for (size_t a = 0; a < br.accounts.size(); a++) {
    const uint32_t seq = led.payee[a];
    CHECK(seq == br.first_seq[a] && !memcmp(&led.account[4 * (size_t)seq], br.accounts[a].data(), 32));
    uint64_t s[4];
    CHECK(led.total_for(br.accounts[a].data(), s));
    for (int j = 0; j < 4; j++) {
      CHECK(s[j] == br.sums[a][j] && led.sum[4 * (size_t)led.astay[seq] + j] == s[j]);
      grand[j] += s[j];
    }
  }
  const uint64_t absent[4] = {3, 1, 4, 1};
  uint64_t s[4] = {9, 9, 9, 9}, rc[6];
  CHECK(!led.total_for(absent, s) && !s[0] && !s[1] && !s[2] && !s[3] && led.find(absent) == NOT_FOUND);
  led.recount(rc);
  CHECK(rc[0] == led.credited && rc[1] == led.count());
  for (int j = 0; j < 4; j++) CHECK(rc[2 + j] == grand[j]);
  // every occupied slot holds a credited entry; the occupied account slots are the accounts; other sums are zero
  uint64_t n_occ = 0, a_occ = 0;
  for (uint64_t at = 0; at < led.nslot.size(); at++) {
    if (led.nslot[at] != EMPTY) {
      n_occ++;
      CHECK(led.nslot[at] < led.count() && (led.flags[led.nslot[at]] & FLAG_CREDITED));
    }
    if (led.aslot[at] != EMPTY) {
      a_occ++;
      CHECK(led.aslot[at] < led.count() && led.astay[led.aslot[at]] == at);
    } else {
      for (int j = 0; j < 4; j++) CHECK(led.sum[4 * at + j] == 0);
    }
  }
  CHECK(n_occ == led.credited && a_occ == led.accounts());
}

// casts the stream in batches of `batch` (0: whole) into a HostLedger of `capacity`, moving it to
// reserves[i].second once reserves[i].first transfers were cast, and holds everything to the brute force
static void run(const std::vector<Cast> &stream, uint64_t capacity, size_t batch, const Pi *padding,
                const std::vector<std::pair<size_t, uint64_t>> &reserves = {}) {
  Screen sc;
  Brute br;
  for (const Key &r : {ROOT_B, ROOT_A, ROOT_B}) {  // out of order and one twice: held sorted, once
    if (!sc.accepts(r.data())) sc.add_root(r.data());
    br.roots.push_back(r);
  }
  CHECK(sc.nroots() == 2 && key_compare(&sc.roots[0], &sc.roots[4]) < 0 && !sc.accepts(ROOT_UNKNOWN.data()));
  if (padding) {
    sc.has_padding = br.has_padding = true;
    memcpy(sc.padding, padding->data(), sizeof sc.padding);
    br.padding = *padding;
  }
  HostLedger led;
  led.open(capacity);
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
        led.reserve(reserves[next_reserve].second);
        CHECK(led.capacity == reserves[next_reserve].second);
        compare(led, br);
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
    CHECK(pk.pos.size() == pk.size() && pk.nullifier.size() == 4 * pk.size() && pk.amount.size() == 4 * pk.size() &&
          pk.account.size() == 4 * pk.size());
    CHECK(led.count() + pk.size() <= led.capacity);  // the streams fit: the ABI refuses the others
    led.admit_packed(pk, out.data());
    cast += n;
    for (uint32_t i = 0; i < n; i++) {
      const Result &w = br.results[at + i], &g = out[i];
      CHECK(g.status == w.status && g.verify_status == w.verify_status && g.number == w.number && g.first == w.first);
    }
    at = end;
  }
  compare(led, br);
}

static void run_all(const std::vector<Cast> &stream, uint64_t capacity, const Pi *padding = nullptr,
                    const std::vector<std::pair<size_t, uint64_t>> &reserves = {}) {
  for (size_t batch : {(size_t)1, (size_t)7, (size_t)64, (size_t)0}) run(stream, capacity, batch, padding, reserves);
}

int main() {
  std::mt19937_64 rng(11);
  auto felt = [&]() { return rng() % P; };
  auto fresh = [&]() { return Key{felt(), felt(), felt(), felt()}; };
  auto limbs = [&]() { return Key{rng() >> 32, rng() >> 32, rng() >> 32, rng() >> 32}; };
  CHECK(table_slots(1) == 2 && table_slots(4) == 8 && table_slots(5) == 16 && table_slots(MAX_CAPACITY) == 1ull << 32);
  {  // the sorted roots: 4096 in a scrambled order, each found, a neighbour of each not
    Screen sc;
    std::vector<Key> rs;
    for (uint64_t i = 0; i < MAX_ROOTS; i++) rs.push_back(Key{(i * 7919) % 4099, i % 3, felt(), 1});
    for (const Key &r : rs)
      if (!sc.accepts(r.data())) sc.add_root(r.data());
    CHECK(sc.nroots() == MAX_ROOTS);
    for (uint32_t i = 0; i + 1 < sc.nroots(); i++) CHECK(key_compare(&sc.roots[4 * i], &sc.roots[4 * i + 4]) < 0);
    for (Key r : rs) {
      CHECK(sc.accepts(r.data()));
      r[3] = 2;
      CHECK(!sc.accepts(r.data()));
    }
  }
  {  // capacity 1: one entry, two slots per table; the double needs a second entry
    const Key n = fresh();
    run_all({transfer(n, limbs())}, 1);
    run_all({transfer(n, limbs()), transfer(n, limbs())}, 2);
  }
  {  // distinct over five accounts, exactly full; then the same nullifiers again: all doubles
    std::vector<Cast> s;
    std::vector<Key> acc = {fresh(), fresh(), fresh(), fresh(), fresh()};
    for (int i = 0; i < 32; i++) s.push_back(transfer(fresh(), limbs(), acc[i % 5]));
    run_all(s, 32);
    std::vector<Cast> twice = s;
    for (const Cast &c : s) twice.push_back(transfer(Key{c.pi[0], c.pi[1], c.pi[2], c.pi[3]}, limbs(), acc[0]));
    run_all(twice, 64);
  }
  {  // one nullifier 64 times; 513 transfers of 2^128 - 1 to one account, and amounts of 0
    const Key n = fresh();
    run_all(std::vector<Cast>(64, transfer(n, limbs())), 64);
    std::vector<Cast> s;
    for (int i = 0; i < 513; i++) s.push_back(transfer(fresh(), FULL));
    for (int i = 0; i < 3; i++) s.push_back(transfer(fresh(), Key{0, 0, 0, 0}, ROOT_B));
    run_all(s, 516);
  }
  for (int table = 0; table < 2; table++) {
    // capacity 4, 8 slots, in the nullifier table and then in the account table: a and b share home slot 7 (b
    // wraps to slot 0), c has a's felt 0 and another felt 3, b again; exactly full, then a table of 16 slots
    const Key a = {(felt() >> 24 << 4) | 7, 1, 2, 3}, b = {(felt() >> 24 << 4) | 7, 1, 2, 3}, c = {a[0], 1, 2, 4};
    const Key d = {(felt() >> 24 << 4) | 15, 6, 6, 6};
    std::vector<Cast> s;
    for (const Key &k : {a, b, c, b, c, d, a, d})
      s.push_back(table == 0 ? transfer(k, limbs(), s.size() & 1 ? ACC : ROOT_B) : transfer(fresh(), limbs(), k));
    run_all(s, 4, nullptr, {{4, 8}});
    run_all(s, 8);
    // 20 keys with home slot S - 2 that differ in felt 1: the chain wraps; then each again
    std::vector<Cast> w;
    const uint64_t f0 = (felt() >> 24 << 7) | 126;
    for (int rep = 0; rep < 2; rep++)
      for (uint64_t i = 0; i < 20; i++) {
        const Key k = {f0, 1000 + i, 7, 7};
        w.push_back(table == 0 ? transfer(k, limbs()) : transfer(fresh(), limbs(), k));
      }
    run_all(w, 64);
  }
  {  // two nullifiers with one home slot, 30 copies each, shuffled; many nullifiers, three copies each, 64 accounts
    std::vector<Cast> s;
    Key n = fresh(), m = fresh();
    m[0] = (m[0] >> 24 << 7) | 5;
    n[0] = (n[0] >> 24 << 7) | 5;
    for (int i = 0; i < 30; i++) {
      s.push_back(transfer(n, limbs()));
      s.push_back(transfer(m, limbs(), ROOT_B));
    }
    std::shuffle(s.begin(), s.end(), rng);
    run_all(s, 64);
    s.clear();
    std::vector<Key> acc(64);
    for (Key &k : acc) k = fresh();
    for (int i = 0; i < 512; i++) {
      const Key k = fresh();
      for (int c = 0; c < 3; c++) s.push_back(transfer(k, limbs(), acc[rng() % 64]));
    }
    std::shuffle(s.begin(), s.end(), rng);
    run_all(s, 1536);
  }
  {  // screened transfers among good ones: every status, the order of the checks, the padding inputs
    Key g[5];
    for (Key &x : g) x = fresh();
    const Key one = {0, 0, 0, 1}, wide = {0, 0, 1ull << 32, 5}, badnul = {g[1][0], g[1][1], g[1][2], P};
    const Cast pad = transfer(g[4], Key{0, 0, 0, 1000}, Key{9, 9, 9, 9});
    Cast near = pad;
    near.pi[15] = 8;
    std::vector<Cast> s = {transfer(g[0], one),
                           transfer(g[1], one, ACC, ROOT_A, 4),
                           transfer(badnul, one),
                           pad,
                           transfer(g[1], wide),
                           transfer(g[1], one, ACC, ROOT_UNKNOWN),
                           transfer(g[1], one, ACC, ROOT_B),
                           transfer(g[1], one),
                           transfer(g[2], wide, ACC, ROOT_UNKNOWN),
                           transfer(badnul, wide, ACC, ROOT_UNKNOWN, 9),
                           transfer(g[2], Key{P, 0, 0, 0}),
                           near,
                           transfer(g[0], FULL, ROOT_B),
                           transfer(g[3], Key{0, 0, 0, 0}),
                           pad,
                           transfer(g[2], FULL)};
    run_all(s, 16, &pad.pi);
    run_all(s, 7, &pad.pi);   // the admitted ones fill it exactly
    run_all(s, 16, nullptr);  // no padding inputs: the pad is a transfer, its copy a double spend
    std::vector<Cast> pads(8, pad);
    run_all(pads, 1, &pad.pi);  // all padding: nothing admitted
    run_all(pads, 8, nullptr);
  }
  {  // growth in mid-stream at exactly-full capacity, doubles of earlier transfers after each reserve
    std::vector<Key> g(100), acc(7);
    for (Key &x : g) x = fresh();
    for (Key &x : acc) x = fresh();
    std::vector<Cast> s;
    auto b = [&](int i) { s.push_back(transfer(g[i], limbs(), acc[i % 7])); };
    for (int i = 0; i < 24; i++) b(i);
    b(3), b(3);
    const size_t r1 = s.size();
    for (int i : {0, 23, 24, 25, 5}) b(i);
    for (int i = 26; i < 50; i++) b(i);
    const size_t r2 = s.size();
    for (int i : {1, 24, 49, 50}) b(i);
    for (int i = 51; i < 100; i++) b(i);
    b(99), b(0);
    run_all(s, 32, nullptr, {{r1, 64}, {r2, 128}});
    run_all(s, 26, nullptr, {{r1, 55}, {r2, s.size()}});  // reserves to exactly what is needed
  }
  printf("ledger_host_check: ok\n");
  return 0;
}
