// witness_launch.h — the launch shapes of device witness generation, in one
// place for its two callers: the prover (prover.cpp gen_witness_batch) and the
// TEST-ONLY probe (witness_probe.cpp qp_debug_witness_program).  Grid sizes,
// coop_max and the per-level block split live here and nowhere else, so a
// program run through the probe takes the launches a proof takes.
#pragma once
#include <algorithm>
#include "witness_kernels.h"

namespace qpk {

// which scheduler runs the generators, and how the cooperative Poseidons sit
struct WitnessForm {
  unsigned threads;  // workgroup size of k_witness_gen (256 leaf circuits, 512 aggregation); sets coop_max
  bool by_level;     // a k_witness_level launch per dependency level, else one k_witness_gen workgroup per proof
  bool row;          // cooperative Poseidons one per 16-lane row, else one per wave
};

inline unsigned witness_cdiv(uint64_t a, unsigned b) { return (unsigned)((a + b - 1) / b); }

// every slot UNSET (slot 0: zero), then the input values into their slots
inline void witness_launch_init(uint64_t *vals, uint32_t nslots, const uint32_t *in_slots, const uint64_t *in_vals,
                                uint32_t nin, uint32_t nb, hipStream_t s) {
  k_witness_init<<<dim3(std::min<unsigned>(witness_cdiv(nslots, 256), 256), nb), 256, 0, s>>>(vals, nslots, nslots,
                                                                                               nullptr, nullptr, 0);
  if (nin) k_witness_inputs<<<dim3(witness_cdiv(nin, 256), nb), 256, 0, s>>>(vals, nslots, in_slots, in_vals, nin);
}

// the generators of nb proofs: `a` with every field set but coop_max and row;
// level_off / level_pos here are the HOST copies of a.level_off / a.level_pos
inline void witness_launch_gens(WitnessGenArgs a, const WitnessForm &f, const uint32_t *level_off,
                                const uint32_t *level_pos, uint32_t nb, hipStream_t s) {
  // up to 4 Poseidon generators per wave per level run cooperatively (12 lanes
  // on one permutation) instead of one per lane
  a.coop_max = 4 * (f.threads / 64);
  a.row = f.row;
  if (f.by_level) {
    for (uint32_t l = 0; l < a.nlevels; l++) {
      const uint32_t pcnt = level_pos[2 * l + 1], nother = level_off[l + 1] - level_off[l] - pcnt;
      const uint32_t na = witness_cdiv(nother, 256), npb = witness_cdiv(pcnt, a.row ? 16 : 4);
      if (na + npb) k_witness_level<<<dim3(na + npb, nb), 256, 0, s>>>(a, l, na);
    }
  } else {
    k_witness_gen<<<nb, f.threads, 0, s>>>(a);
  }
}

}  // namespace qpk
