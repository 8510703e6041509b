// input_screen.hip — the screen of Wormhole circuit inputs on the device
// (gfx950).  The rules are input_screen.h's, the ones the host path runs; here
// they run over poseidon_fast.h's permutation: the state stays non-canonical
// between permutations (permute_nc takes any 64-bit lanes), canon on the four
// lanes kept, as k_ledger_leaves runs it.  VALU-bound and latency-bound: a lane
// of k_screen_nodes runs 24 dependent permutations over 768 bytes it alone
// reads; registers only, no LDS.  Each sponge loop is rolled (one inlined
// permutation per loop body), so the kernels stay a few permutations long.
// Nothing is read in the launch that writes it, nothing spins, and the only
// atomic is the error word's atomicOr.
#include "input_screen.h"
#include "input_screen_kernels.h"
#include "poseidon_dev.h"

namespace qpk {

namespace {
struct DevHash {
  static __device__ __forceinline__ void permute(uint64_t s[12]) { pf::permute_nc(s); }
  static __device__ __forceinline__ uint64_t canon(uint64_t x) { return psd::canon(x); }
};

__device__ __forceinline__ void store_digest(uint64_t *p, const uint64_t d[4]) {
  ulonglong2 *o = reinterpret_cast<ulonglong2 *>(p);
  o[0] = make_ulonglong2(d[0], d[1]);
  o[1] = make_ulonglong2(d[2], d[3]);
}
}  // namespace

__global__ void __launch_bounds__(256) k_screen_nodes(ScreenDev d) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= d.nwork) return;
  const uint32_t w = d.work[k];
  if (w >= d.m * qis::MAX_NODES) {  // cannot be reached: the host packs the list
    atomicOr(d.err, SCREEN_ERR_WORK);
    return;
  }
  const uint32_t input = w / qis::MAX_NODES, node = w % qis::MAX_NODES;
  const uint8_t *rec = d.rec + (uint64_t)input * qis::REC_BYTES;
  const uint32_t *limbs = qis::rec_nodes(rec) + node * qis::NODE_STRIDE;
  uint64_t dig[4], child[4];
  qis::child_digest(limbs, qis::rec_start(rec)[node], child);
  qis::node_digest<DevHash>(limbs, dig);
  store_digest(d.dig + (uint64_t)w * 4, dig);
  store_digest(d.child + (uint64_t)w * 4, child);
}

__global__ void __launch_bounds__(256) k_screen_resolve(ScreenDev d) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= d.m) return;
  const uint64_t *hdr = qis::rec_hdr(d.rec + (uint64_t)j * qis::REC_BYTES);
  uint32_t status = SCREEN_NO_STATUS, witness = 0;
  if (hdr[qis::H_PROOF_LEN] > qis::MAX_NODES)  // cannot be reached: pack_input refuses such an input
    atomicOr(d.err, SCREEN_ERR_PROOF_LEN);
  else
    status = qis::resolve<DevHash>(hdr, d.dig + (uint64_t)j * qis::MAX_NODES * 4,
                                   d.child + (uint64_t)j * qis::MAX_NODES * 4, &witness);
  reinterpret_cast<uint2 *>(d.res)[j] = make_uint2(status, witness);
}

void screen_nodes(const ScreenDev &d, hipStream_t s) {
  if (!d.nwork) return;
  k_screen_nodes<<<screen_blocks(d.nwork), SCREEN_BLOCK, 0, s>>>(d);
}

void screen_resolve(const ScreenDev &d, hipStream_t s) {
  if (!d.m) return;
  k_screen_resolve<<<screen_blocks(d.m), SCREEN_BLOCK, 0, s>>>(d);
}

}  // namespace qpk
