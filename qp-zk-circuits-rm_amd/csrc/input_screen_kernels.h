// input_screen_kernels.h — argument layout and launchers of input_screen.hip:
// the screen of Wormhole circuit inputs on the device.  The rules and the
// record layout: input_screen.h.  One launcher per step; the launcher owns the
// grid and block sizes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace qpk {

// one uploaded batch of m packed inputs (all pointers device):
//   work[nwork]   the nodes to hash, dense: input * 20 + node, node < the input's proof_len
//   rec[m]        the records (qis::REC_BYTES each)
//   dig, child    [m][20][4]: a node's digest and the child digest found in it, written for the work items
//   res[m][2]     status, witness
//   err           the defensive error word
struct ScreenDev {
  const uint32_t *work;
  const uint8_t *rec;
  uint64_t *dig, *child;
  uint32_t *res;
  uint32_t *err;
  uint32_t nwork, m;
};

// bits of the error word: a work item beyond m * 20, a header whose proof_len is above 20 (neither
// can be reached: the host packs both)
constexpr uint32_t SCREEN_ERR_WORK = 1, SCREEN_ERR_PROOF_LEN = 2;
constexpr uint32_t SCREEN_NO_STATUS = 0xFFFFFFFFu;  // res of an input whose header was refused

constexpr uint32_t SCREEN_BLOCK = 256;
inline uint32_t screen_blocks(uint64_t n) { return (uint32_t)((n + SCREEN_BLOCK - 1) / SCREEN_BLOCK); }

// one lane per work item: the node's 24-permutation sponge and the child digest found in it
void screen_nodes(const ScreenDev &d, hipStream_t s);
// after screen_nodes, a launch of its own: one lane per input; the nullifier, unspendable-account and
// leaf hashes, the chain compare, status and witness
void screen_resolve(const ScreenDev &d, hipStream_t s);

}  // namespace qpk
