// input_screen_check.cpp — the input screen's host-only code (csrc/input_screen.h:
// statuses 1..3 and the packing of an input into a record, the rolled sponges,
// the child digest, the chain compare) under the sanitizers, against a
// brute-force restatement of the rules over vectors and a plain sponge: the
// packing of nodes of 0, 1, 751, 752 and 753 bytes and of 20 and 21 nodes into
// a record of exactly REC_BYTES on the heap, the child digest at starts 0, 179,
// 180 and beyond and with limb pairs >= p, and seeded tries of depth 0..20 with
// one or two faults each.  A stand-alone CPU program; device code runs under no
// sanitizer.
//
//   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//       tools/input_screen_check.cpp -o input_screen_check && ./input_screen_check
#include <stdio.h>
#include <stdlib.h>
#include <memory>
#include <random>
#include <utility>
#include <vector>
#include "../qp-zk-circuits-rm_amd/csrc/field.h"
#include "../qp-zk-circuits-rm_amd/csrc/poseidon.h"
#include "../qp-zk-circuits-rm_amd/csrc/input_screen.h"

using namespace qis;

#define CHECK(x)                                                     \
  do {                                                               \
    if (!(x)) {                                                      \
      fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #x); \
      exit(1);                                                       \
    }                                                                \
  } while (0)

struct HostHash {
  static void permute(uint64_t s[12]) {
    for (int j = 0; j < 12; j++) s[j] = gl::canon(s[j]);
    ps::permute(s);
  }
  static uint64_t canon(uint64_t x) { return gl::canon(x); }
};

typedef std::vector<uint64_t> Felts;
typedef std::pair<uint32_t, uint32_t> Verdict;

// ---- the restatement: hash_n_to_hash_no_pad as plonky2 writes it, the rules over vectors

static Felts hash_no_pad(const Felts &in) {
  uint64_t s[12] = {0};
  for (size_t off = 0; off < in.size(); off += 8) {
    for (size_t j = 0; j < 8 && off + j < in.size(); j++) s[j] = in[off + j] % P;
    ps::permute(s);
  }
  return Felts(s, s + 4);
}
static Felts bytes_felts(const uint8_t *b, size_t n) {
  Felts f;
  for (size_t i = 0; i < n; i += 4) {
    uint64_t v = 0;
    for (size_t k = 0; k < 4 && i + k < n; k++) v |= (uint64_t)b[i + k] << (8 * k);
    f.push_back(v);
  }
  return f;
}
static Felts digest_of(const uint8_t b[32]) {
  Felts f(4, 0);
  for (int i = 0; i < 32; i++) f[i / 8] |= (uint64_t)b[i] << (8 * (i % 8));
  return f;
}
static void append(Felts &a, const Felts &b) { a.insert(a.end(), b.begin(), b.end()); }

static Felts brute_leaf(const qp_wormhole_inputs &in) {
  Felts leaf = {in.transfer_count >> 32, in.transfer_count & 0xFFFFFFFFull};
  append(leaf, digest_of(in.funding_account));
  append(leaf, digest_of(in.unspendable_account));
  for (int k = 3; k >= 0; k--) leaf.push_back(bytes_felts(in.funding_amount + 4 * k, 4)[0]);
  return hash_no_pad(leaf);
}

static Verdict brute(const qp_wormhole_inputs &in) {
  const uint8_t *const digests[5] = {in.nullifier, in.unspendable_account, in.root_hash, in.funding_account,
                                     in.exit_account};
  for (uint32_t k = 0; k < 5; k++)
    for (uint64_t v : digest_of(digests[k]))
      if (v >= P) return {FIELD_RANGE, k};
  if (in.num_nodes > 20) return {PROOF_TOO_LONG, in.num_nodes};
  for (uint32_t i = 0; i < in.num_nodes; i++)
    if (in.node_lens[i] > 752) return {NODE_TOO_LARGE, i};
  const Felts count = {in.transfer_count >> 32, in.transfer_count & 0xFFFFFFFFull};
  Felts pre = bytes_felts((const uint8_t *)"~nullif~", 8);
  append(pre, bytes_felts(in.secret, 32));
  append(pre, count);
  if (hash_no_pad(hash_no_pad(pre)) != digest_of(in.nullifier)) return {NULLIFIER, 0};
  pre = bytes_felts((const uint8_t *)"wormhole", 8);
  append(pre, bytes_felts(in.secret, 32));
  if (hash_no_pad(hash_no_pad(pre)) != digest_of(in.unspendable_account)) return {UNSPENDABLE, 0};
  Felts due = digest_of(in.root_hash);
  for (uint32_t i = 0; i < in.num_nodes; i++) {
    Felts f = bytes_felts(in.nodes[i], in.node_lens[i]);
    f.resize(188, 0);
    if (hash_no_pad(f) != due) return {STORAGE_NODE, i};
    const uint64_t s = in.indices[i] / 8;
    for (int y = 0; y < 4; y++)
      due[y] = s < 180 ? (uint64_t)(((unsigned __int128)f[s + 2 * y] + ((unsigned __int128)f[s + 2 * y + 1] << 32)) % P) : 0;
  }
  if (in.num_nodes < 20) {
    const Felts leaf = brute_leaf(in);
    for (int y = 1; y < 4; y++)
      if (leaf[y] != due[y]) return {STORAGE_LEAF, in.num_nodes};
  }
  return {OK, 0};
}

// ---- the code under test: pack_input into a heap record of exactly REC_BYTES, then the rules

struct Record {
  std::unique_ptr<uint64_t[]> words{new uint64_t[REC_BYTES / 8]};
  uint8_t *bytes() { return reinterpret_cast<uint8_t *>(words.get()); }
};

static Verdict screened(const qp_wormhole_inputs &in) {
  Record rec;
  CHECK(pointers_ok(in));
  uint32_t witness = 77;
  uint32_t status = pack_input(in, rec.bytes(), &witness);
  if (status != OK) return {status, witness};
  const uint64_t *hdr = rec_hdr(rec.bytes());
  const uint32_t proof_len = (uint32_t)hdr[H_PROOF_LEN];
  CHECK(proof_len == in.num_nodes && proof_len <= MAX_NODES);
  std::vector<uint64_t> dig(4 * (size_t)proof_len), child(4 * (size_t)proof_len);  // exact: an overrun is seen
  for (uint32_t i = 0; i < proof_len; i++) {
    const uint32_t *limbs = rec_nodes(rec.bytes()) + (size_t)i * NODE_STRIDE;
    node_digest<HostHash>(limbs, dig.data() + 4 * i);
    child_digest(limbs, rec_start(rec.bytes())[i], child.data() + 4 * i);
  }
  status = resolve<HostHash>(hdr, dig.data(), child.data(), &witness);
  return {status, witness};
}

// ---- inputs that own their storage

struct Input {
  qp_wormhole_inputs in{};
  std::vector<std::vector<uint8_t>> nodes;
  std::vector<const uint8_t *> ptrs;
  std::vector<uint32_t> lens;
  std::vector<uint64_t> indices;
  const qp_wormhole_inputs &view() {
    ptrs.clear(), lens.clear();
    for (auto &nd : nodes) {
      ptrs.push_back(nd.empty() ? nullptr : nd.data());
      lens.push_back((uint32_t)nd.size());
    }
    in.num_nodes = (uint32_t)nodes.size();
    in.nodes = ptrs.data(), in.node_lens = lens.data(), in.indices = indices.data();
    return in;
  }
};

static void put_digest(uint8_t out[32], const Felts &d) {
  for (int i = 0; i < 32; i++) out[i] = (uint8_t)(d[i / 8] >> (8 * (i % 8)));
}

static std::mt19937_64 rng(20251021);
static uint64_t below(uint64_t n) { return rng() % n; }

// a consistent input: a trie of `depth` nodes of random lengths, each holding the next digest somewhere
static void build(Input &x, uint32_t depth) {
  for (uint8_t &b : x.in.secret) b = (uint8_t)rng();
  for (uint8_t &b : x.in.funding_amount) b = (uint8_t)rng();
  x.in.transfer_count = rng();
  put_digest(x.in.funding_account, {below(P), below(P), below(P), P - 1});
  put_digest(x.in.exit_account, {below(P), 0, below(P), below(P)});
  Felts pre = bytes_felts((const uint8_t *)"wormhole", 8);
  append(pre, bytes_felts(x.in.secret, 32));
  put_digest(x.in.unspendable_account, hash_no_pad(hash_no_pad(pre)));
  pre = bytes_felts((const uint8_t *)"~nullif~", 8);
  append(pre, bytes_felts(x.in.secret, 32));
  pre.push_back(x.in.transfer_count >> 32), pre.push_back(x.in.transfer_count & 0xFFFFFFFFull);
  put_digest(x.in.nullifier, hash_no_pad(hash_no_pad(pre)));
  Felts child = brute_leaf(x.in);
  x.nodes.assign(depth, {});
  x.indices.assign(depth, 0);
  for (uint32_t i = depth; i-- > 0;) {
    const uint32_t len = 32 + (uint32_t)below(752 - 32 + 1), start = (uint32_t)below((len - 32) / 4 + 1);
    std::vector<uint8_t> &nd = x.nodes[i];
    nd.resize(len);
    for (uint8_t &b : nd) b = (uint8_t)rng();
    for (int k = 0; k < 32; k++) nd[4 * start + k] = (uint8_t)(child[k / 8] >> (8 * (k % 8)));
    x.indices[i] = 8 * (uint64_t)start + below(8);
    Felts f = bytes_felts(nd.data(), nd.size());
    f.resize(188, 0);
    child = hash_no_pad(f);
  }
  put_digest(x.in.root_hash, child);
}

static uint32_t seen[STATUS_COUNT];

static void agree(Input &x) {
  const Verdict want = brute(x.view()), got = screened(x.view());
  if (want != got) {
    fprintf(stderr, "screen (%u, %u) != restatement (%u, %u) at %u nodes\n", got.first, got.second, want.first,
            want.second, x.in.num_nodes);
    exit(1);
  }
  seen[got.first]++;
}

static void check_packing() {
  // node lengths around the limb and node edges: the limbs, the zero padding up to the stride, the verdict
  for (uint32_t len : {0u, 1u, 751u, 752u, 753u}) {
    Input x;
    build(x, 3);
    x.nodes[1].assign(len, 0);
    for (uint32_t k = 0; k < len; k++) x.nodes[1][k] = (uint8_t)(0xA1 + k);
    Record rec;
    uint32_t witness = 77;
    const uint32_t status = pack_input(x.view(), rec.bytes(), &witness);
    if (len > 752) {
      CHECK(status == NODE_TOO_LARGE && witness == 1);
      continue;
    }
    CHECK(status == OK && witness == 0);
    const Felts f = bytes_felts(x.nodes[1].data(), len);
    CHECK(f.size() == (len + 3) / 4);
    const uint32_t *limbs = rec_nodes(rec.bytes()) + NODE_STRIDE;
    for (uint32_t k = 0; k < NODE_STRIDE; k++) CHECK(limbs[k] == (k < f.size() ? f[k] : 0));
    CHECK(rec_start(rec.bytes())[1] == x.indices[1] / 8 && rec_hdr(rec.bytes())[H_PROOF_LEN] == 3);
    agree(x);
  }
  for (uint32_t count : {20u, 21u}) {
    Input x;
    build(x, 20);
    if (count == 21) x.nodes.push_back(std::vector<uint8_t>(40, 7)), x.indices.push_back(0);
    Record rec;
    uint32_t witness = 77;
    const uint32_t status = pack_input(x.view(), rec.bytes(), &witness);
    CHECK(count == 20 ? status == OK && witness == 0 : status == PROOF_TOO_LONG && witness == 21);
    agree(x);
  }
  // the whole call's refusals
  Input x;
  build(x, 2);
  x.view();
  qp_wormhole_inputs broken = x.in;
  broken.nodes = nullptr;
  CHECK(!pointers_ok(broken));
  broken = x.in, broken.node_lens = nullptr;
  CHECK(!pointers_ok(broken));
  broken = x.in, broken.indices = nullptr;
  CHECK(!pointers_ok(broken));
  x.ptrs[1] = nullptr;
  CHECK(!pointers_ok(x.in));
  broken = x.in, broken.num_nodes = 0, broken.nodes = nullptr, broken.node_lens = nullptr, broken.indices = nullptr;
  CHECK(pointers_ok(broken));
}

static void check_child_digest() {
  std::vector<uint32_t> limbs(NODE_STRIDE, 0);
  for (uint32_t k = 0; k < NODE_FELTS; k++) limbs[k] = 0xFFFFFFFFu;  // every pair is 2^64 - 1 >= p
  for (uint32_t start : {0u, 1u, 100u, 179u}) {
    uint64_t got[4];
    child_digest(limbs.data(), start, got);
    for (int y = 0; y < 4; y++) CHECK(got[y] == ~0ull - P);
  }
  for (uint32_t k = 0; k < NODE_FELTS; k++) limbs[k] = k % 2 ? 0xFFFFFFFFu : k / 2;  // pairs around p: p - 1, p, p + 1, ..
  for (uint32_t start : {0u, 2u, 178u}) {
    uint64_t got[4];
    child_digest(limbs.data(), start, got);
    for (int y = 0; y < 4; y++) {
      const uint64_t v = 0xFFFFFFFF00000000ull | (start / 2 + y);
      CHECK(got[y] == (v >= P ? v - P : v) && got[y] < P);
    }
  }
  for (uint32_t start : {180u, 181u, 187u, 188u, 0xFFFFFFFFu}) {
    uint64_t got[4] = {1, 1, 1, 1};
    child_digest(limbs.data(), start, got);  // reads nothing
    CHECK(!got[0] && !got[1] && !got[2] && !got[3]);
  }
}

static void check_tries() {
  for (uint32_t depth : {0u, 1u, 2u, 5u, 19u, 20u})
    for (uint32_t fault = 0; fault < 14; fault++) {
      Input x;
      build(x, depth);
      const uint32_t at = depth ? (uint32_t)below(depth) : 0;
      switch (fault) {
        case 0: break;
        case 1: x.in.nullifier[below(32)] ^= 1; break;
        case 2: x.in.unspendable_account[below(32)] ^= 1; break;
        case 3: x.in.transfer_count ^= 1ull << below(64); break;
        case 4: x.in.funding_amount[below(16)] ^= 0x10; break;
        case 5: x.in.exit_account[1] ^= 1; break;
        case 6: x.in.root_hash[below(32)] ^= 2; break;
        case 7: if (depth) x.nodes[at][below(x.nodes[at].size())] ^= 0x80; break;
        case 8: if (depth) x.indices[at] += 8; break;
        case 9: if (depth) x.indices[at] = 8 * (180 + below(1000)); break;
        case 10: if (depth) x.nodes[at].resize(753 + below(100), 0); break;
        case 11: put_digest(x.in.root_hash, {1, 2, P + below(1000), 4}), x.in.secret[0] ^= 1; break;
        case 12: if (depth) x.nodes[at].push_back(0); break;  // a zero byte more, up to 753 bytes
        case 13: if (depth > 1) x.nodes[0][3] ^= 4, x.nodes[depth - 1][0] ^= 4; x.in.funding_account[0] ^= 1; break;
      }
      agree(x);
    }
  for (uint32_t round = 0; round < 40; round++) {  // more depths, two faults at random
    Input x;
    build(x, (uint32_t)below(21));
    const uint32_t depth = (uint32_t)x.nodes.size();
    for (int k = 0; k < 2; k++)
      switch (below(5)) {
        case 0: x.in.secret[below(32)] ^= 1; break;
        case 1: if (depth) x.nodes[below(depth)][below(32)] ^= 1; break;
        case 2: x.in.funding_account[below(24)] ^= 1; break;
        case 3: if (depth) x.indices[below(depth)] ^= 8; break;
        default: break;
      }
    agree(x);
  }
}

int main() {
  check_packing();
  check_child_digest();
  check_tries();
  for (uint32_t s = 0; s < STATUS_COUNT; s++) CHECK(seen[s] > 0);
  printf("input_screen_check ok: statuses seen");
  for (uint32_t s = 0; s < STATUS_COUNT; s++) printf(" %u:%u", s, seen[s]);
  printf("\n");
  return 0;
}
