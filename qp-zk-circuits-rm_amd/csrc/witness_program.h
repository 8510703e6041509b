// witness_program.h — validation of a caller's generator program before the
// TEST-ONLY probe (witness_probe.cpp) hands it to the witness kernels.  Host
// C++ only, no HIP: tools/witness_probe_check.cpp runs it under the sanitizers.
//
// The kernels trust their tables (the builder made them); a program from a
// test did not come from the builder, so every index a kernel would follow is
// bounded here: the rows a record touches, every slot id (records, the wire
// table, the inputs, the expansion maps), the wire offsets a row-layout kind
// reads (W = 135), the per-kind operation indices, and the level tables the
// schedulers walk.  Empty string: well-formed.
#pragma once
#include <stdint.h>
#include <string>
#include "../../include/qpgpu.h"

namespace qwp {

constexpr uint32_t MULTI = 0x80000000u;  // == qc::DEV_MULTI
constexpr uint32_t NKINDS = 14, ROW_W = 135;
constexpr uint32_t MAX_B = 64, MAX_SLOTS = 1u << 20, MAX_GENS = 1u << 16, MAX_NIN = 1u << 20, MAX_NPIS = 1u << 16;
// qc::GenKind order (witness.hip WG_*)
enum : uint32_t { K_CONSTANT = 0, K_ARITH, K_POSEIDON, K_BASE_SPLIT, K_EQUALITY, K_WIRE_SPLIT, K_EXT_DIV,
                  K_RANDOM_ACCESS, K_ARITH_EXT, K_MUL_EXT, K_REDUCING, K_REDUCING_EXT, K_POSEIDON_MDS, K_COSET_INTERP };

struct Rec {  // one DevGen record out of its five words
  uint32_t kind, row, s[4];
  uint64_t k0, k1;
};
inline Rec rec(const uint64_t *g) {
  return Rec{(uint32_t)g[0], (uint32_t)(g[0] >> 32),
             {(uint32_t)g[1], (uint32_t)(g[1] >> 32), (uint32_t)g[2], (uint32_t)(g[2] >> 32)}, g[3], g[4]};
}
// the kinds that read a gate row's wires at the standard config's offsets
inline bool row_layout(uint32_t k) {
  return k == K_POSEIDON || k == K_RANDOM_ACCESS || k == K_ARITH_EXT || k == K_MUL_EXT || k == K_REDUCING ||
         k == K_REDUCING_EXT || k == K_POSEIDON_MDS || k == K_COSET_INTERP;
}

inline std::string validate(const qp_witness_program &p) {
  auto at = [](const char *what, uint64_t i) { return std::string(what) + " " + std::to_string(i); };
  if (p.form >= QP_WFORM_COUNT) return "unknown form";
  if (p.B < 1 || p.B > MAX_B) return "B outside 1..64";
  if (p.nslots < 1 || p.nslots > MAX_SLOTS) return "nslots outside 1..2^20";
  if (p.ngens > MAX_GENS) return "more than 2^16 records";
  if (p.nlevels > MAX_GENS) return "more than 2^16 levels";
  if (p.nin > MAX_NIN) return "more than 2^20 inputs";
  if (p.limbs > 63) return "limbs above 63";
  if ((uint64_t)1 + p.limbs > p.W) return "1 + limbs above W";
  if ((uint64_t)p.nrows * p.W > ((uint64_t)1 << 28)) return "wire table above 2^28 entries";
  if (p.zero_slot >= p.nslots) return "zero_slot outside the slots";
  if (!p.level_off || (p.nlevels && !p.level_pos) || (p.ngens && !p.gens) || (p.nrows && !p.wslot) ||
      (p.nin && (!p.in_slots || !p.in_vals)))
    return "null table";
  // levels
  for (uint32_t l = 0; l < p.nlevels; l++)
    if (p.level_off[l] > p.level_off[l + 1]) return at("level_off decreases at level", l);
  if (p.level_off[p.nlevels] != p.ngens) return "level_off does not end at the record count";
  // records
  auto slot_ok = [&](uint32_t s) { return (s & ~MULTI) < p.nslots; };
  for (uint32_t i = 0; i < p.ngens; i++) {
    const Rec g = rec(p.gens + 5 * (size_t)i);
    if (g.kind >= NKINDS) return at("unknown kind in record", i);
    if (row_layout(g.kind) && p.W != ROW_W) return at("W is not 135 for the row-layout record", i);
    uint64_t last_row = 0;
    bool has_row = row_layout(g.kind) || g.kind == K_BASE_SPLIT;
    if (has_row) last_row = g.row;
    if (g.kind == K_WIRE_SPLIT && g.s[1]) {
      has_row = true;
      last_row = (uint64_t)g.row + g.s[1] - 1;
    }
    if (has_row && last_row >= p.nrows) return at("row outside the wire table in record", i);
    uint32_t nsl = 0;
    switch (g.kind) {
      case K_CONSTANT: nsl = p.num_consts < 2 ? 1 : 2; break;
      case K_ARITH:
      case K_EQUALITY:
      case K_EXT_DIV: nsl = 4; break;
      case K_BASE_SPLIT:
      case K_WIRE_SPLIT: nsl = 1; break;
      default: break;
    }
    for (uint32_t k = 0; k < nsl; k++)
      if (!slot_ok(g.s[k])) return at("slot outside the slots in record", i);
    if (g.kind == K_EXT_DIV && (!slot_ok((uint32_t)g.k0) || !slot_ok((uint32_t)(g.k0 >> 32))))
      return at("quotient slot outside the slots in record", i);
    if (g.kind == K_RANDOM_ACCESS && g.s[0] >= 4) return at("random-access copy above 3 in record", i);
    if (g.kind == K_ARITH_EXT && g.s[0] >= 10) return at("arithmetic-extension op above 9 in record", i);
    if (g.kind == K_MUL_EXT && g.s[0] >= 13) return at("mul-extension op above 12 in record", i);
  }
  // the Poseidon run of each level: inside the level, Poseidon records only, and all of them
  for (uint32_t l = 0; l < p.nlevels; l++) {
    const uint64_t lo = p.level_off[l], hi = p.level_off[l + 1];
    const uint64_t plo = p.level_pos[2 * l], pcnt = p.level_pos[2 * l + 1];
    if (plo < lo || plo + pcnt > hi) return at("Poseidon run outside level", l);
    for (uint64_t i = lo; i < hi; i++) {
      const bool in_run = i >= plo && i < plo + pcnt;
      const bool pos = rec(p.gens + 5 * (size_t)i).kind == K_POSEIDON;
      if (in_run && !pos) return at("record that is no Poseidon in the Poseidon run of level", l);
      if (!in_run && pos) return at("Poseidon record outside the Poseidon run of level", l);
    }
  }
  // tables
  for (uint64_t i = 0, n = (uint64_t)p.nrows * p.W; i < n; i++)
    if (!slot_ok(p.wslot[i])) return at("slot outside the slots at wslot entry", i);
  // the input store and the expansion index with the id as it stands: no flag bit
  for (uint32_t i = 0; i < p.nin; i++)
    if (p.in_slots[i] >= p.nslots) return at("slot outside the slots at in_slots entry", i);
  if (p.wslot_cm) {
    if (!p.nrows) return "expansion of an empty wire table";
    if (p.npis > MAX_NPIS) return "more than 2^16 public inputs";
    if (p.npis && !p.pi_slots) return "null table";
    for (uint64_t i = 0, n = (uint64_t)p.nrows * p.W; i < n; i++)
      if (p.wslot_cm[i] >= p.nslots) return at("slot outside the slots at wslot_cm entry", i);
    for (uint32_t i = 0; i < p.npis; i++)
      if (p.pi_slots[i] >= p.nslots) return at("slot outside the slots at pi_slots entry", i);
  }
  return "";
}

}  // namespace qwp
