// verifier.h — the native batch verifier (plonky2 VerifierCircuitData::verify,
// the reference's qp-wormhole-verifier): host part in verifier.cpp, the query
// rounds' kernels in verifier.hip, the per-lane checks both share in
// verifier_rounds.h.
#pragma once
#include <hip/hip_runtime.h>
#include "verifier_rounds.h"

namespace qv {

// one lane per (proof, query, tree): leaf digest, climb, cap comparison.
// The job's pointers are device pointers.
void launch_paths(const PathJob &job, hipStream_t s);
// one lane per (proof, query): the query round's arithmetic
void launch_fri(const FriJob &job, hipStream_t s);

// the same checks on the host (ctx == NULL), lanes [lo, hi)
void host_paths(const PathJob &job, uint32_t cls, uint32_t lo, uint32_t hi, uint32_t ok_base);
void host_fri(const FriJob &job, uint32_t lo, uint32_t hi);

}  // namespace qv
