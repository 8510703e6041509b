// verifier.h — the native batch verifier (plonky2 VerifierCircuitData::verify,
// the reference's qp-wormhole-verifier): host part in verifier.cpp, the query
// rounds' kernels in verifier.hip, the per-lane checks both share in
// verifier_rounds.h.
#pragma once
#include <hip/hip_runtime.h>
#include "verifier_rounds.h"

struct qp_verifier;

namespace qv {

// what the ballot box (ballot.cpp) reads of a verifier: the circuit's public-input
// count (0: the handle is not usable) and its last error
uint32_t public_input_count(const qp_verifier *v);
// the public inputs [public_input_count] inside a proof's bytes: valid for a
// proof on which this verifier's verdict was QP_VERIFY_OK (its length and
// every felt were checked then); 8-byte little-endian words, not aligned
const uint8_t *public_inputs(const qp_verifier *v, const uint8_t *proof);

// one lane per (proof, query, tree): leaf digest, climb, cap comparison.
// The job's pointers are device pointers.
void launch_paths(const PathJob &job, hipStream_t s);
// one lane per (proof, query): the query round's arithmetic
void launch_fri(const FriJob &job, hipStream_t s);

// the same checks on the host (ctx == NULL), lanes [lo, hi)
void host_paths(const PathJob &job, uint32_t cls, uint32_t lo, uint32_t hi, uint32_t ok_base);
void host_fri(const FriJob &job, uint32_t lo, uint32_t hi);

}  // namespace qv
