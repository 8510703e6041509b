// poseidon_dev.h — the kernels' entry points to the Poseidon permutation (leaf
// hashing, Merkle levels, PoW, the verifier): poseidon_fast.h's form, same
// function as ps::permute (poseidon.h).  State is NON-canonical in [0, 2^64)
// going in and coming out; call canon on the lanes read out.
#pragma once
#include "field.h"
#include "poseidon.h"
#include "field_nc.h"
#include "poseidon_fast.h"

namespace psd {

using gfn::canon;
using pf::permute_nc;
using pf::permute;  // permute_nc, then canon on all 12 lanes

// two_to_one form: s[8..11] == 0 on entry, only lanes 0..3 read
__device__ __forceinline__ void permute_nc_node(uint64_t s[12]) { pf::permute_nc_capz<0xFu>(s); }

}  // namespace psd
