// input_screen.h — the screen of Wormhole circuit inputs: per input, exactly
// what the circuit (wormhole.cpp build_wormhole + commit) decides, as the first
// check that fails.  One statement of the rules, compiled for the host and,
// under hipcc, for the device: input_screen.cpp runs them with the host Poseidon
// (ctx == NULL), input_screen.hip with poseidon_fast.h's, and the stand-alone
// check tools/input_screen_check.cpp holds them to a brute-force restatement.
//
//   # status          fires when                                          witness
//   0 OK              the circuit is satisfiable by this input            0
//   1 FIELD_RANGE     a 32-byte digest has an 8-byte chunk >= p           0 nullifier, 1 unspendable account, 2 root
//                     (commit refuses these)                              hash, 3 funding account, 4 exit account (lowest)
//   2 PROOF_TOO_LONG  num_nodes > 20                                      num_nodes
//   3 NODE_TOO_LARGE  a node longer than 752 bytes (188 felts of 4)       the lowest such node
//   4 NULLIFIER       nullifier != H(H("~nullif~" | secret | count))      0
//   5 UNSPENDABLE     unspendable account != H(H("wormhole" | secret))    0
//   6 STORAGE_NODE    some i < proof_len: H(node i) != the digest due     the lowest such i
//   7 STORAGE_LEAF    proof_len < 20 and felts 1..3 of the leaf hash !=   proof_len
//                     felts 1..3 of the digest due at position proof_len
//
// H is hash_n_to_hash_no_pad: rate 8, overwrite mode.  Felts of a byte string
// are its 4-byte little-endian limbs, a short last limb zero-extended.  A node
// is hashed as its 188 felts zero-padded whatever its length: 23 chunks of 8
// and one of 4, 24 permutations.  Node 0 must hash to the root, node i to the
// digest found in node i - 1: the four (lo, hi) limb pairs from felt index / 8
// (the hex index's floor) on, reduced mod p as the circuit's lo + 2^32 hi is,
// and ZERO when that start is >= 180 (the circuit scans starts 0..179 only).
// The leaf is the 14 felts count(2) | funding account(4) | unspendable
// account(4) | amount(4); the digest due at position proof_len is the root when
// proof_len is 0.  The circuit's quirks are part of the definition: felt 0 of
// the leaf hash is not compared, at proof_len 20 no leaf check exists, the exit
// account is unconstrained (its range is still checked by commit).
//
// Statuses 1..3 are decided by pack_input on the host; what passes them is
// packed into a record (below) that the rules read, on either path.
#pragma once
#include <stdint.h>
#include <string.h>
#include "../../include/qpgpu.h"

#if defined(__HIPCC__)
#define QIS_HD __host__ __device__
#else
#define QIS_HD
#endif

namespace qis {

constexpr uint64_t P = 0xFFFFFFFF00000001ull;
constexpr uint32_t MAX_NODES = 20;     // storage_proof/mod.rs:21
constexpr uint32_t NODE_FELTS = 188;   // storage_proof/mod.rs:22
constexpr uint32_t NODE_BYTES = 4 * NODE_FELTS;
constexpr uint32_t SCAN_STARTS = 180;  // the circuit looks for the child digest at felts 0..179
constexpr uint32_t NODE_CHUNKS = 24;   // permutations per node: ceil(188 / 8)

// qp_input_status (qpgpu.h), in the order of the checks
enum : uint32_t { OK = 0, FIELD_RANGE = 1, PROOF_TOO_LONG = 2, NODE_TOO_LARGE = 3, NULLIFIER = 4, UNSPENDABLE = 5,
                  STORAGE_NODE = 6, STORAGE_LEAF = 7, STATUS_COUNT = 8 };

// The record of one packed input, REC_BYTES long, 16-byte aligned:
//   nodes [20][192] u32   the limbs of node i, zero-padded; a node's stride is 192 limbs so that the
//                         24th chunk's eight loads stay inside the node (limbs 188..191 are zero and unread)
//   start [20] u32        min(index / 8, 180): the felt the child digest starts at, 180 = none
//   pad   [4] u32
//   hdr   [64] u64        three preimages of 16 felts each, the digests they must give, the root, proof_len
// Nodes at and above proof_len are not written and not read.
constexpr uint32_t NODE_STRIDE = 192;
constexpr uint32_t REC_NODES = 0, REC_START = MAX_NODES * NODE_STRIDE * 4, REC_HDR = REC_START + (MAX_NODES + 4) * 4;
constexpr uint32_t HDR_WORDS = 64;
constexpr uint32_t REC_BYTES = REC_HDR + HDR_WORDS * 8;
static_assert(REC_HDR % 16 == 0 && REC_BYTES % 16 == 0, "records and their headers stay 16-byte aligned");
// header words
constexpr uint32_t H_PRE = 0;          // [3][16]: the nullifier, unspendable-account and leaf preimages
constexpr uint32_t H_EXPECT = 48;      // [2][4]: the nullifier and the unspendable account of the input
constexpr uint32_t H_ROOT = 56;        // [4]
constexpr uint32_t H_PROOF_LEN = 60;
// felts of the three preimages beyond the first chunk of 8 (12, 10 and 14 felts in all)
QIS_HD inline uint32_t pre_tail(uint32_t h) { return h == 0 ? 4 : h == 1 ? 2 : 6; }

QIS_HD inline const uint32_t *rec_nodes(const uint8_t *rec) { return reinterpret_cast<const uint32_t *>(rec + REC_NODES); }
QIS_HD inline const uint32_t *rec_start(const uint8_t *rec) { return reinterpret_cast<const uint32_t *>(rec + REC_START); }
QIS_HD inline const uint64_t *rec_hdr(const uint8_t *rec) { return reinterpret_cast<const uint64_t *>(rec + REC_HDR); }

// ---- the rules over a record.  HASH gives the permutation and the canonical form of a lane:
// HASH::permute(s) over any 64-bit lanes, HASH::canon(x) < p.

// H(node): limbs[192], the node's 188 felts zero-padded
template <class HASH>
QIS_HD inline void node_digest(const uint32_t *limbs, uint64_t out[4]) {
  uint64_t s[12];
  for (int j = 0; j < 12; j++) s[j] = 0;
#pragma unroll 1
  for (uint32_t c = 0; c < NODE_CHUNKS; c++) {
    const uint32_t *src = limbs + 8 * c;
    const bool whole = c + 1 < NODE_CHUNKS;  // the last chunk overwrites lanes 0..3 only
#pragma unroll
    for (int j = 0; j < 8; j++) s[j] = j < 4 || whole ? (uint64_t)src[j] : s[j];
    HASH::permute(s);
  }
  for (int j = 0; j < 4; j++) out[j] = HASH::canon(s[j]);
}

// the digest found in a node at felt `start`
QIS_HD inline void child_digest(const uint32_t *limbs, uint32_t start, uint64_t out[4]) {
  for (int y = 0; y < 4; y++) {
    uint64_t v = 0;
    if (start < SCAN_STARTS) v = (uint64_t)limbs[start + 2 * y] | (uint64_t)limbs[start + 2 * y + 1] << 32;
    out[y] = v >= P ? v - P : v;
  }
}

// statuses 4..7 of a record whose nodes' digests dig[i][4] and child digests child[i][4], i < proof_len,
// were computed by node_digest and child_digest.  proof_len <= 20 (the caller checks).
template <class HASH>
QIS_HD inline uint32_t resolve(const uint64_t *hdr, const uint64_t *dig, const uint64_t *child, uint32_t *witness) {
  uint64_t s[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, d[4] = {0, 0, 0, 0};
  uint32_t differs = 0;
  // H(H(nullifier preimage)), H(H(unspendable preimage)), H(leaf) as one rolled loop of eight permutations:
  // hash h takes steps 3 h .. 3 h + 2: the preimage's first eight felts over a zero state, its tail over
  // lanes 0.., and (the first two hashes) the digest alone over a zero state again
#pragma unroll 1
  for (uint32_t step = 0; step < 8; step++) {
    const uint32_t h = step / 3, phase = step % 3;
    const uint64_t *pre = hdr + H_PRE + 16 * h;
    if (phase == 0) {
#pragma unroll
      for (int j = 0; j < 12; j++) s[j] = j < 8 ? pre[j] : 0;
    } else if (phase == 1) {
      const uint32_t tail = pre_tail(h);
#pragma unroll
      for (int j = 0; j < 6; j++) s[j] = (uint32_t)j < tail ? pre[8 + j] : s[j];
    } else {
#pragma unroll
      for (int j = 4; j < 12; j++) s[j] = 0;
    }
    HASH::permute(s);
    if (phase == 2 || step == 7) {  // a digest is complete; the last one, the leaf hash, stays in d
#pragma unroll
      for (int j = 0; j < 4; j++) d[j] = HASH::canon(s[j]);
      if (h < 2) {
#pragma unroll
        for (int j = 0; j < 4; j++)
          if (d[j] != hdr[H_EXPECT + 4 * h + j]) differs |= 1u << h;
      }
    }
  }
  *witness = 0;
  if (differs & 1) return NULLIFIER;
  if (differs & 2) return UNSPENDABLE;
  const uint32_t proof_len = (uint32_t)hdr[H_PROOF_LEN];
  uint64_t due[4];
  for (int j = 0; j < 4; j++) due[j] = hdr[H_ROOT + j];
  for (uint32_t i = 0; i < proof_len; i++) {
    bool same = true;
    for (int j = 0; j < 4; j++) same = same && dig[4 * i + j] == due[j];
    if (!same) {
      *witness = i;
      return STORAGE_NODE;
    }
    for (int j = 0; j < 4; j++) due[j] = child[4 * i + j];
  }
  if (proof_len < MAX_NODES && (d[1] != due[1] || d[2] != due[2] || d[3] != due[3])) {  // d = the leaf hash
    *witness = proof_len;
    return STORAGE_LEAF;
  }
  return OK;
}

// ---- the host's part: statuses 1..3 and the packing

inline uint32_t load_le32(const uint8_t *b, size_t n) {  // n <= 4 bytes, zero-extended
  uint32_t v = 0;
  for (size_t k = 0; k < n; k++) v |= (uint32_t)b[k] << (8 * k);
  return v;
}
// a 32-byte digest as four 8-byte little-endian felts; false if one is >= p
inline bool digest_felts(const uint8_t b[32], uint64_t out[4]) {
  bool ok = true;
  for (int i = 0; i < 4; i++) {
    uint64_t v = 0;
    for (int k = 0; k < 8; k++) v |= (uint64_t)b[8 * i + k] << (8 * k);
    ok = ok && v < P;
    out[i] = v;
  }
  return ok;
}

// what the whole call refuses (a programming error, not a bad input): a null array where num_nodes
// announces entries, a null node with a length
inline bool pointers_ok(const qp_wormhole_inputs &in) {
  if (!in.num_nodes) return true;
  if (!in.nodes || !in.node_lens || !in.indices) return false;
  for (uint32_t i = 0; i < in.num_nodes; i++)
    if (!in.nodes[i] && in.node_lens[i]) return false;
  return true;
}

// statuses 1..3 of an input, in order; OK: the input is packed into rec[REC_BYTES] (16-byte aligned).
// A refused input may leave a partly written record behind: the caller reuses it.
inline uint32_t pack_input(const qp_wormhole_inputs &in, uint8_t *rec, uint32_t *witness) {
  uint64_t dg[5][4];
  const uint8_t *const digests[5] = {in.nullifier, in.unspendable_account, in.root_hash, in.funding_account,
                                     in.exit_account};
  *witness = 0;
  for (uint32_t k = 0; k < 5; k++)
    if (!digest_felts(digests[k], dg[k])) {
      *witness = k;
      return FIELD_RANGE;
    }
  if (in.num_nodes > MAX_NODES) {
    *witness = in.num_nodes;
    return PROOF_TOO_LONG;
  }
  for (uint32_t i = 0; i < in.num_nodes; i++)
    if (in.node_lens[i] > NODE_BYTES) {
      *witness = i;
      return NODE_TOO_LARGE;
    }
  uint32_t *nodes = reinterpret_cast<uint32_t *>(rec + REC_NODES);
  uint32_t *start = reinterpret_cast<uint32_t *>(rec + REC_START);
  uint64_t *hdr = reinterpret_cast<uint64_t *>(rec + REC_HDR);
  for (uint32_t i = 0; i < in.num_nodes; i++) {
    uint32_t *limbs = nodes + (size_t)i * NODE_STRIDE;
    const uint32_t len = in.node_lens[i], full = len / 4;
    for (uint32_t k = 0; k < full; k++) limbs[k] = load_le32(in.nodes[i] + 4 * (size_t)k, 4);
    uint32_t k = full;
    if (len % 4) limbs[k++] = load_le32(in.nodes[i] + 4 * (size_t)full, len % 4);
    for (; k < NODE_STRIDE; k++) limbs[k] = 0;
    const uint64_t felt = in.indices[i] / 8;
    start[i] = felt < SCAN_STARTS ? (uint32_t)felt : SCAN_STARTS;
  }
  for (uint32_t i = in.num_nodes; i < MAX_NODES + 4; i++) start[i] = SCAN_STARTS;
  memset(hdr, 0, HDR_WORDS * 8);
  uint64_t *nul = hdr + H_PRE, *uns = hdr + H_PRE + 16, *leaf = hdr + H_PRE + 32;
  nul[0] = load_le32((const uint8_t *)"~nullif~", 4), nul[1] = load_le32((const uint8_t *)"~nullif~" + 4, 4);
  uns[0] = load_le32((const uint8_t *)"wormhole", 4), uns[1] = load_le32((const uint8_t *)"wormhole" + 4, 4);
  for (uint32_t k = 0; k < 8; k++) nul[2 + k] = uns[2 + k] = load_le32(in.secret + 4 * k, 4);
  const uint64_t count_hi = in.transfer_count >> 32, count_lo = in.transfer_count & 0xFFFFFFFFull;
  nul[10] = leaf[0] = count_hi;
  nul[11] = leaf[1] = count_lo;
  for (uint32_t k = 0; k < 4; k++) {
    leaf[2 + k] = dg[3][k];
    leaf[6 + k] = dg[1][k];
    // the u128 amount's 32-bit limbs, most significant first (u128_to_felts)
    leaf[10 + k] = load_le32(in.funding_amount + 4 * (3 - k), 4);
    hdr[H_EXPECT + k] = dg[0][k];
    hdr[H_EXPECT + 4 + k] = dg[1][k];
    hdr[H_ROOT + k] = dg[2][k];
  }
  hdr[H_PROOF_LEN] = in.num_nodes;
  return OK;
}

inline const char *status_text(uint32_t status) {
  static const char *const text[STATUS_COUNT] = {
      "ok",
      "a digest chunk is out of field range",
      "the storage proof is longer than 20 nodes",
      "a storage-proof node is longer than 752 bytes",
      "the nullifier is not the hash of the secret and the transfer count",
      "the unspendable account is not the hash of the secret",
      "a storage-proof node does not hash to the digest expected at its position",
      "the leaf hash is not the digest expected below the last storage-proof node"};
  return status < STATUS_COUNT ? text[status] : "unknown input status";
}

}  // namespace qis
