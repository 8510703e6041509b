// prover_dev.h — the few helpers that more than one prover stage file
// (pp_z.hip, quotient.hip, openings.hip, fri.hip) uses; nothing else includes it.
#pragma once
#include "field.h"
#include "kernels.h"

namespace qpk {

using gl::ext;

static inline unsigned cdiv(uint64_t a, unsigned b) { return (unsigned)((a + b - 1) / b); }

__device__ __forceinline__ uint64_t wpow_N(const uint64_t *__restrict__ tw, uint32_t j, uint32_t logN) {
  // w_N^j from the half table of w_{2^TW_LOG}: w_N^j = w_T^{j << (TW_LOG-logN)}
  return tw_get(tw, j << (TW_LOG - logN));
}

}  // namespace qpk
