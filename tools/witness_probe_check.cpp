// witness_probe_check.cpp — the witness probe's program validator
// (csrc/witness_program.h) under the sanitizers: one good program, then one
// malformed program per rule, each of which must be refused with the rule's
// text.  Every table is a heap vector of exactly its stated size, so a check
// that read past a table (a level table one entry short, a wire table of a
// narrower W) would be an AddressSanitizer report, not a wrong answer.  A
// stand-alone CPU program; device code runs under no sanitizer.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/witness_probe_check.cpp -o witness_probe_check && ./witness_probe_check
#include <stdio.h>
#include <stdlib.h>
#include <functional>
#include <string>
#include <vector>
#include "../qp-zk-circuits-rm_amd/csrc/witness_program.h"

using namespace qwp;

#define CHECK(x)                                                     \
  do {                                                               \
    if (!(x)) {                                                      \
      fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #x); \
      exit(1);                                                       \
    }                                                                \
  } while (0)

// a program that owns its tables
struct Prog {
  std::vector<uint64_t> gens, in_vals;
  std::vector<uint32_t> level_off, level_pos, wslot, in_slots, wslot_cm, pi_slots;
  uint32_t nrows = 0, W = 135, nslots = 0, limbs = 63, zero_slot = 0, num_consts = 2, B = 1, form = 0;
  bool expand = false;
  void rec(uint32_t kind, uint32_t row, uint32_t s0 = 0, uint32_t s1 = 0, uint32_t s2 = 0, uint32_t s3 = 0,
           uint64_t k0 = 0, uint64_t k1 = 0) {
    gens.insert(gens.end(), {kind | (uint64_t)row << 32, s0 | (uint64_t)s1 << 32, s2 | (uint64_t)s3 << 32, k0, k1});
  }
  uint64_t &word(uint32_t i, uint32_t w) { return gens[5 * (size_t)i + w]; }
  qp_witness_program view() const {
    qp_witness_program p{};
    p.gens = gens.data();
    p.ngens = (uint32_t)(gens.size() / 5);
    p.level_off = level_off.data();
    p.level_pos = level_pos.data();
    p.nlevels = (uint32_t)(level_pos.size() / 2);
    p.wslot = wslot.data();
    p.nrows = nrows;
    p.W = W;
    p.nslots = nslots;
    p.limbs = limbs;
    p.zero_slot = zero_slot;
    p.num_consts = num_consts;
    p.in_slots = in_slots.data();
    p.in_vals = in_vals.empty() ? nullptr : in_vals.data();
    p.nin = (uint32_t)in_slots.size();
    p.B = B;
    p.form = form;
    if (expand) {
      p.wslot_cm = wslot_cm.data();
      p.pi_slots = pi_slots.data();
      p.npis = (uint32_t)pi_slots.size();
    }
    return p;
  }
};

// seven records of seven kinds in one level, the Poseidon last; six rows; every wire its own slot
static Prog good() {
  Prog g;
  g.nrows = 6;
  g.nslots = 1 + g.nrows * g.W + 16;
  g.wslot.resize((size_t)g.nrows * g.W);
  for (size_t i = 0; i < g.wslot.size(); i++) g.wslot[i] = 1 + (uint32_t)i;
  g.wslot[7] |= MULTI;
  const uint32_t f = 1 + g.nrows * g.W;  // free slots
  g.rec(K_ARITH, 0, f, f + 1, f + 2, (f + 3) | MULTI, 1, 1);                     // 0
  g.rec(K_EXT_DIV, 0, f + 4, f + 5, f + 6, f + 7, (f + 8) | (uint64_t)(f + 9) << 32);  // 1
  g.rec(K_WIRE_SPLIT, 0, f, 2);                                                // 2: rows 0, 1
  g.rec(K_RANDOM_ACCESS, 2, 3);                                                // 3
  g.rec(K_ARITH_EXT, 3, 9, 0, 0, 0, 1, 1);                                     // 4
  g.rec(K_MUL_EXT, 4, 12, 0, 0, 0, 1);                                         // 5
  g.rec(K_POSEIDON, 5);                                                        // 6
  g.level_off = {0, 7};
  g.level_pos = {6, 1};
  for (uint32_t i = 0; i < 10; i++) g.in_slots.push_back(f + i);
  g.B = 2;
  g.in_vals.assign((size_t)g.B * g.in_slots.size(), 5);
  return g;
}

static int ncases = 0;
static void refused(const char *text, const std::function<void(Prog &)> &mutate) {
  Prog g = good();
  mutate(g);
  const std::string got = validate(g.view());
  if (got.find(text) == std::string::npos) {
    fprintf(stderr, "expected \"%s\", got \"%s\"\n", text, got.c_str());
    exit(1);
  }
  ncases++;
}

int main() {
  {
    Prog g = good();
    CHECK(validate(g.view()).empty());
    // every form; the expansion maps; no records at all; a WIRE_SPLIT over no gate touches no row
    for (uint32_t f = 0; f < QP_WFORM_COUNT; f++) {
      g.form = f;
      CHECK(validate(g.view()).empty());
    }
    g.expand = true;
    g.wslot_cm.assign(g.wslot.size(), g.nslots - 1);
    g.pi_slots = {0, g.nslots - 1};
    CHECK(validate(g.view()).empty());
    Prog e;
    e.nslots = 1;
    e.W = 64;
    e.level_off = {0};
    CHECK(validate(e.view()).empty());
    e.rec(K_WIRE_SPLIT, 1000, 0, 0);
    e.level_off = {0, 1};
    e.level_pos = {1, 0};
    CHECK(validate(e.view()).empty());
    // an empty level between two others; its run is the empty run at its end
    Prog l = good();
    l.level_off = {0, 7, 7, 7};
    l.level_pos = {6, 1, 7, 0, 7, 0};
    CHECK(validate(l.view()).empty());
  }
  refused("unknown form", [](Prog &g) { g.form = QP_WFORM_COUNT; });
  refused("B outside 1..64", [](Prog &g) { g.B = 65; g.in_vals.assign(65 * g.in_slots.size(), 1); });
  refused("B outside 1..64", [](Prog &g) { g.B = 0; });
  refused("nslots outside 1..2^20", [](Prog &g) { g.nslots = (1u << 20) + 1; });
  refused("more than 2^16 records", [](Prog &g) {
    g.gens.assign(5 * ((size_t)MAX_GENS + 1), 0);
    g.level_off = {0, MAX_GENS + 1};
    g.level_pos = {MAX_GENS + 1, 0};
  });
  refused("limbs above 63", [](Prog &g) { g.limbs = 64; });
  refused("1 + limbs above W", [](Prog &g) { g.W = 63; g.wslot.resize((size_t)g.nrows * 63); });
  refused("zero_slot outside the slots", [](Prog &g) { g.zero_slot = g.nslots; });
  refused("null table", [](Prog &g) { g.in_vals.clear(); g.in_vals.shrink_to_fit(); });
  refused("level_off decreases at level 1", [](Prog &g) { g.level_off = {0, 7, 6}; g.level_pos = {6, 1, 7, 0}; });
  refused("level_off does not end at the record count", [](Prog &g) { g.level_off = {0, 6}; });
  refused("unknown kind in record 0", [](Prog &g) { g.word(0, 0) = NKINDS; });
  refused("W is not 135 for the row-layout record 3", [](Prog &g) { g.W = 134; g.wslot.resize((size_t)g.nrows * 134); });
  refused("row outside the wire table in record 6", [](Prog &g) { g.word(6, 0) = K_POSEIDON | (uint64_t)g.nrows << 32; });
  refused("row outside the wire table in record 2", [](Prog &g) { g.word(2, 1) = (g.word(2, 1) & 0xFFFFFFFFu) | (uint64_t)7 << 32; });
  refused("row outside the wire table in record 2", [](Prog &g) {  // row + count wraps 32 bits
    g.word(2, 0) = K_WIRE_SPLIT | (uint64_t)0xFFFFFFFFu << 32;
    g.word(2, 1) = (g.word(2, 1) & 0xFFFFFFFFu) | (uint64_t)2 << 32;
  });
  refused("slot outside the slots in record 0", [](Prog &g) { g.word(0, 2) = (g.word(0, 2) & 0xFFFFFFFFu) | (uint64_t)g.nslots << 32; });
  refused("slot outside the slots in record 0", [](Prog &g) { g.word(0, 1) = (uint64_t)(g.nslots | MULTI); });
  refused("quotient slot outside the slots in record 1", [](Prog &g) { g.word(1, 3) = g.nslots | (uint64_t)1 << 32; });
  refused("quotient slot outside the slots in record 1", [](Prog &g) { g.word(1, 3) = 1 | (uint64_t)g.nslots << 32; });
  refused("random-access copy above 3 in record 3", [](Prog &g) { g.word(3, 1) = 4; });
  refused("arithmetic-extension op above 9 in record 4", [](Prog &g) { g.word(4, 1) = 10; });
  refused("mul-extension op above 12 in record 5", [](Prog &g) { g.word(5, 1) = 13; });
  refused("Poseidon run outside level 0", [](Prog &g) { g.level_pos = {6, 2}; });
  refused("Poseidon run outside level 1", [](Prog &g) { g.level_off = {0, 7, 7}; g.level_pos = {6, 1, 6, 0}; });
  refused("record that is no Poseidon in the Poseidon run of level 0", [](Prog &g) { g.level_pos = {5, 2}; });
  refused("Poseidon record outside the Poseidon run of level 0", [](Prog &g) { g.level_pos = {7, 0}; });
  refused("slot outside the slots at wslot entry 410", [](Prog &g) { g.wslot[410] = g.nslots | MULTI; });
  refused("slot outside the slots at in_slots entry 0", [](Prog &g) { g.in_slots[0] = g.nslots; });
  refused("slot outside the slots at in_slots entry 9", [](Prog &g) { g.in_slots[9] = 1 | MULTI; });
  refused("slot outside the slots at wslot_cm entry 3", [](Prog &g) {
    g.expand = true;
    g.wslot_cm.assign(g.wslot.size(), 0);
    g.wslot_cm[3] = 1 | MULTI;
  });
  refused("slot outside the slots at pi_slots entry 1", [](Prog &g) {
    g.expand = true;
    g.wslot_cm.assign(g.wslot.size(), 0);
    g.pi_slots = {0, g.nslots};
  });
  printf("witness_probe_check: ok (%d refusals)\n", ncases);
  return 0;
}
