// circuit.cpp — see circuit.h.  Follows upstream plonky2 (qp-plonky2 1.1.1):
//   gadgets/arithmetic.rs   arithmetic + special cases + operation dedup
//   gadgets/split_base.rs   split_le via BaseSumGate<2> (63 limbs)
//   gadgets/select.rs, gadgets/equality (is_equal + EqualityGenerator)
//   hash/hashing.rs         hash_n_to_m_no_pad (overwrite mode, PoseidonGate)
//   plonk/circuit_builder.rs build(): PI hash -> PublicInputGate, constant
//                           gates, padding to 2^k, selector_polynomials
//                           (greedy groups, max degree = qdf + 1), wire
//                           partition -> sigma polys (k_i * w^row)
//   gates/poseidon.rs       PoseidonGenerator wire layout
#include "paths.h"
#include "circuit.h"
#include <algorithm>
#include <numeric>
#include <stdexcept>
#include <unordered_map>
#include <stdlib.h>
#include <string.h>
#include "field.h"
#include "poseidon.h"

namespace qc {

static const F NEG_ONE = gl::P - 1;
static const uint64_t UNUSED_SELECTOR = 0xFFFFFFFFull;

CircuitBuilder::CircuitBuilder(const CircuitConfig &cfg) : cfg_(cfg) {
  arith_ops_ = builder_params(G_ARITHMETIC, cfg).p0;
  base_sum_limbs_ = builder_params(G_BASE_SUM, cfg).p0;
}

Target CircuitBuilder::add_virtual_target() { return Target::virt(nvirt_++); }

std::vector<Target> CircuitBuilder::add_virtual_targets(size_t n) {
  std::vector<Target> v(n);
  for (auto &t : v) t = add_virtual_target();
  return v;
}

Target CircuitBuilder::add_virtual_public_input() {
  Target t = add_virtual_target();
  register_public_input(t);
  return t;
}

std::vector<Target> CircuitBuilder::add_virtual_hash_public_input() {
  auto v = add_virtual_hash();
  for (auto t : v) register_public_input(t);
  return v;
}

uint32_t CircuitBuilder::add_gate(GateKind k, F c0, F c1) {
  uint32_t row = (uint32_t)rows_.size();
  rows_.push_back(GateInst{k, c0, c1});
  Gen g{};
  g.row = row;
  if (k == G_CONSTANT) { g.kind = GEN_CONSTANT; gens_.push_back(g); }
  if (k == G_POSEIDON) { g.kind = GEN_POSEIDON; gens_.push_back(g); }
  if (k == G_BASE_SUM) { g.kind = GEN_BASE_SPLIT; gens_.push_back(g); }
  return row;
}

Target CircuitBuilder::constant(F c) {
  c = gl::canon(c);
  auto it = const_to_target_.find(c);
  if (it != const_to_target_.end()) return it->second;
  Target t = add_virtual_target();
  const_to_target_[c] = t;
  target_to_const_[t.v] = c;
  return t;
}

bool CircuitBuilder::as_const(Target t, F &v) const {
  auto it = target_to_const_.find(t.v);
  if (it == target_to_const_.end()) return false;
  v = it->second;
  return true;
}

void CircuitBuilder::connect(Target a, Target b) {
  if (!a.is_virtual() && a.col() >= cfg_.num_routed_wires) throw std::runtime_error("connect: unrouted wire");
  if (!b.is_virtual() && b.col() >= cfg_.num_routed_wires) throw std::runtime_error("connect: unrouted wire");
  copies_.push_back({a, b});
}

void CircuitBuilder::connect_hashes(const std::vector<Target> &a, const std::vector<Target> &b) {
  for (size_t i = 0; i < 4; i++) connect(a[i], b[i]);
}

Target CircuitBuilder::arithmetic(F c0, F c1, Target m0, Target m1, Target addend) {
  // arithmetic_special_cases
  Target z = zero();
  F m0c, m1c, ac;
  bool hm0 = as_const(m0, m0c), hm1 = as_const(m1, m1c), ha = as_const(addend, ac);
  bool first_zero = c0 == 0 || m0 == z || m1 == z;
  bool second_zero = c1 == 0 || addend == z;
  bool first_const = first_zero || (hm0 && hm1);
  F first_val = first_zero ? 0 : (first_const ? gl::mul(gl::mul(m0c, m1c), c0) : 0);
  bool second_const = second_zero || ha;
  F second_val = second_zero ? 0 : (ha ? gl::mul(ac, c1) : 0);
  if (first_const && second_const) return constant(gl::add(first_val, second_val));
  if (first_zero && c1 == 1) return addend;
  if (second_zero) {
    if (hm0 && gl::mul(m0c, c0) == 1) return m1;
    if (hm1 && gl::mul(m1c, c0) == 1) return m0;
  }
  auto key = std::make_tuple(c0, c1, m0.v, m1.v, addend.v);
  if (arith_cache_.empty()) arith_cache_.reserve(1u << 16);
  auto it = arith_cache_.find(key);
  if (it != arith_cache_.end()) return it->second;
  // find_slot for ArithmeticGate with constants (c0, c1)
  auto sk = std::make_pair(c0, c1);
  auto os = arith_open_.find(sk);
  uint32_t row, op;
  if (os == arith_open_.end() || os->second.second >= arith_ops_) {
    row = add_gate(G_ARITHMETIC, c0, c1);
    op = 0;
  } else {
    row = os->second.first;
    op = os->second.second;
  }
  arith_open_[sk] = {row, op + 1};
  connect(m0, Target::wire(row, 4 * op));
  connect(m1, Target::wire(row, 4 * op + 1));
  connect(addend, Target::wire(row, 4 * op + 2));
  Gen g{};
  g.kind = GEN_ARITH;
  g.row = row;
  g.op = op;
  gens_.push_back(g);
  Target out = Target::wire(row, 4 * op + 3);
  arith_cache_[key] = out;
  return out;
}

Target CircuitBuilder::add(Target x, Target y) { return arithmetic(1, 1, x, one(), y); }
Target CircuitBuilder::sub(Target x, Target y) { return arithmetic(1, NEG_ONE, x, one(), y); }
Target CircuitBuilder::mul(Target x, Target y) { return arithmetic(1, 0, x, y, x); }
Target CircuitBuilder::mul_add(Target x, Target y, Target z) { return arithmetic(1, 1, x, y, z); }
Target CircuitBuilder::mul_sub(Target x, Target y, Target z) { return arithmetic(1, NEG_ONE, x, y, z); }
Target CircuitBuilder::mul_const(F c, Target x) {
  Target ct = constant(c);
  return mul(ct, x);
}
Target CircuitBuilder::mul_const_add(F c, Target x, Target y) {
  Target ct = constant(c);
  return mul_add(ct, x, y);
}
Target CircuitBuilder::add_virtual_bool_target_safe() {
  Target t = add_virtual_target();
  connect(mul_sub(t, t, t), zero());
  return t;
}

// common/src/gadgets.rs:53-65: a + b - 2ab
Target xor_gadget(CircuitBuilder &b, Target a, Target c) {
  Target ab = b.mul(a, c);
  Target two_ab = b.mul_const(2, ab);
  Target a_plus_b = b.add(a, c);
  return b.sub(a_plus_b, two_ab);
}

// common/src/gadgets.rs:14-41: left < right for a constant left
Target is_const_less_than(CircuitBuilder &b, uint32_t left, Target right, uint32_t n_log) {
  auto right_bits = b.split_le(right, n_log);
  Target lt = b._false();
  Target eq = b._true();
  for (uint32_t i = n_log; i-- > 0;) {
    Target a = b.constant_bool((left >> i) & 1);
    Target bb = right_bits[i];
    Target not_a = b._not(a);
    Target not_a_and_b = b._and(not_a, bb);
    Target this_lt = b._and(not_a_and_b, eq);
    lt = b._or(lt, this_lt);
    Target a_xor_b = xor_gadget(b, a, bb);
    Target not_xor = b._not(a_xor_b);
    eq = b._and(eq, not_xor);
  }
  return lt;
}

Target CircuitBuilder::_not(Target b) {
  Target o = one();
  return sub(o, b);
}
Target CircuitBuilder::_or(Target a, Target b) {
  Target t = arithmetic(NEG_ONE, 1, a, b, a);
  return add(t, b);
}
Target CircuitBuilder::select(Target b, Target x, Target y) {
  Target tmp = mul_sub(b, y, y);
  return mul_sub(b, x, tmp);
}

Target CircuitBuilder::is_equal(Target x, Target y) {
  Target z = zero();
  Target equal = add_virtual_target();
  Target not_equal = _not(equal);
  Target inv = add_virtual_target();
  Gen g{};
  g.kind = GEN_EQUALITY;
  g.a = x; g.b = y; g.c = equal; g.d = inv;
  gens_.push_back(g);
  simple_gens_.push_back(g);
  Target diff = sub(x, y);
  Target not_equal_check = mul(equal, diff);
  Target diff_normalized = mul(diff, inv);
  connect(not_equal_check, z);
  // qp-plonky2 checks diff * inv == not_equal with an arithmetic op
  // (diff_normalized - not_equal == 0) instead of upstream's copy constraint.
  // Pinned by the reference's current-circuit proofs (tests/test_reference_layout.py):
  // the extra (1,-1) op puts the fixture's PublicInputGate at row 7039 (181 ops
  // per storage node later than without it), its cells hold
  // (diff_normalized, 1, not_equal) -- (1-eq, 1, 1-eq) in the fixture's wire
  // openings -- and only this routing gives the fixture's 80 sigma columns.
  connect(sub(diff_normalized, not_equal), z);
  return equal;
}

std::vector<Target> CircuitBuilder::split_le(Target x, uint32_t num_bits) {
  std::vector<Target> bits;
  if (num_bits == 0) {
    assert_zero(x);
    return bits;
  }
  uint32_t L = base_sum_limbs_;
  uint32_t k = (num_bits + L - 1) / L;
  std::vector<uint32_t> gates;
  for (uint32_t i = 0; i < k; i++) gates.push_back(add_gate(G_BASE_SUM));
  for (uint32_t g : gates)
    for (uint32_t l = 0; l < L; l++) bits.push_back(Target::wire(g, 1 + l));
  for (size_t i = num_bits; i < bits.size(); i++) assert_zero(bits[i]);
  bits.resize(num_bits);
  Target acc = zero();
  F base = gl::pow(2, L);
  for (size_t i = gates.size(); i-- > 0;) acc = mul_const_add(base, acc, Target::wire(gates[i], 0));
  connect(acc, x);
  // WireSplitGenerator: the integer's L-bit chunks into the gates' sum wires
  // (with one gate the sum wire is the integer itself, so the schedule skips
  // it; upstream's generator list has it either way)
  Gen g{};
  g.kind = GEN_WIRE_SPLIT;
  g.a = x;
  g.row = gates[0];
  g.op = k;
  if (k > 1) gens_.push_back(g);
  simple_gens_.push_back(g);
  return bits;
}

std::vector<Target> CircuitBuilder::permute_swapped(const std::vector<Target> &state, Target swap) {
  uint32_t row = add_gate(G_POSEIDON);
  connect(swap, Target::wire(row, 24));
  for (uint32_t i = 0; i < 12; i++) connect(state[i], Target::wire(row, i));
  std::vector<Target> out(12);
  for (uint32_t i = 0; i < 12; i++) out[i] = Target::wire(row, 12 + i);
  return out;
}

std::vector<Target> CircuitBuilder::hash_n_to_hash_no_pad(const std::vector<Target> &inputs) {
  Target z = zero();
  std::vector<Target> state(12, z);
  for (size_t off = 0; off < inputs.size(); off += 8) {
    for (size_t i = 0; i < 8 && off + i < inputs.size(); i++) state[i] = inputs[off + i];
    state = permute(state);
  }
  return std::vector<Target>(state.begin(), state.begin() + 4);
}

std::vector<Target> CircuitBuilder::hash_or_noop(const std::vector<Target> &inputs) {
  if (inputs.size() > 4) return hash_n_to_hash_no_pad(inputs);
  std::vector<Target> out(inputs);
  while (out.size() < 4) out.push_back(zero());
  return out;
}

// gadgets/random_access.rs random_access: find_slot over RandomAccessGate copies
Target CircuitBuilder::random_access(Target index, const std::vector<Target> &v) {
  if (v.size() != RA_VEC) throw std::runtime_error("random_access: only 16-element vectors are supported");
  if (ra_open_.second >= RA_COPIES) ra_open_ = {add_gate(G_RANDOM_ACCESS), 0};
  const uint32_t row = ra_open_.first, copy = ra_open_.second++;
  Target claimed = add_virtual_target();
  for (uint32_t i = 0; i < RA_VEC; i++) connect(v[i], Target::wire(row, ra_wire_item(i, copy)));
  connect(index, Target::wire(row, ra_wire_index(copy)));
  connect(claimed, Target::wire(row, ra_wire_claimed(copy)));
  Gen g{};
  g.kind = GEN_RANDOM_ACCESS;
  g.row = row;
  g.op = copy;
  gens_.push_back(g);
  return claimed;
}

// ---------------------------------------------------------------- build

namespace {
struct UF {
  std::vector<uint32_t> p;
  explicit UF(size_t n) : p(n) { std::iota(p.begin(), p.end(), 0); }
  uint32_t find(uint32_t x) {
    while (p[x] != x) {
      p[x] = p[p[x]];
      x = p[x];
    }
    return x;
  }
  void unite(uint32_t a, uint32_t b) {
    a = find(a);
    b = find(b);
    if (a != b) p[std::max(a, b)] = std::min(a, b);
  }
};

// lists of uint32 appended row by row into one offsets and one values array
// (the build's per-generator lists without an allocation per list)
struct Rows {
  std::vector<uint32_t> off{0}, val;
  struct Span {
    uint32_t *b, *e;
    uint32_t *begin() const { return b; }
    uint32_t *end() const { return e; }
    size_t size() const { return (size_t)(e - b); }
  };
  void push(uint32_t v) { val.push_back(v); }
  void close() { off.push_back((uint32_t)val.size()); }
  void close_unique() {  // the open row sorted, duplicates dropped
    const auto b = val.begin() + off.back();
    std::sort(b, val.end());
    val.erase(std::unique(b, val.end()), val.end());
    close();
  }
  Span operator[](size_t r) { return {val.data() + off[r], val.data() + off[r + 1]}; }
};

// counting sort: for keys k[i] < nkeys (i in order), off[k] .. off[k + 1] of
// the returned index list holds the i with key k, ascending
void group_by_key(const std::vector<uint32_t> &keys, size_t nkeys, std::vector<uint32_t> &off,
                  std::vector<uint32_t> &idx) {
  off.assign(nkeys + 1, 0);
  for (uint32_t k : keys) off[k + 1]++;
  for (size_t k = 0; k < nkeys; k++) off[k + 1] += off[k];
  idx.resize(keys.size());
  std::vector<uint32_t> cur(off.begin(), off.end() - 1);
  for (size_t i = 0; i < keys.size(); i++) idx[cur[keys[i]]++] = (uint32_t)i;
}
}  // namespace

CircuitData CircuitBuilder::build() {
  // public-input hash routed to a PublicInputGate
  auto pih = hash_n_to_hash_no_pad(public_inputs_);
  uint32_t pi_row = add_gate(G_PUBLIC_INPUT);
  for (uint32_t i = 0; i < 4; i++) connect(pih[i], Target::wire(pi_row, i));
  // randomize_unused_pi_wires: the remaining wires of the PublicInputGate row
  // carry random values -- in qp-plonky2 under both configs (the reference's
  // non-zk dummy_proof.bin has them too: tests/test_reference_layout.py); they
  // are inputs of commit() here
  std::vector<Target> zk_cells;
  for (uint32_t j = 4; j < cfg_.num_wires; j++) zk_cells.push_back(Target::wire(pi_row, j));
  mark_inputs(zk_cells);
  // constant gates: cfg.num_constants constants per ConstantGate row, in
  // ascending canonical value (plonky2 build(): constants_to_targets
  // .sorted_by_key(|(c, _)| c.to_canonical_u64()) zipped with the generators)
  std::vector<std::pair<F, Target>> consts;
  for (auto &kv : const_to_target_) consts.push_back({kv.first, kv.second});
  std::sort(consts.begin(), consts.end(), [](const std::pair<F, Target> &a, const std::pair<F, Target> &b) {
    return a.first < b.first;
  });
  const uint32_t ncg = cfg_.num_constants;
  for (size_t i = 0; i < consts.size(); i += ncg) {
    F c0 = consts[i].first, c1 = i + 1 < consts.size() ? consts[i + 1].first : 0;
    uint32_t row = add_gate(G_CONSTANT, c0, c1);
    // connect(wire, t) as upstream: the fresh gate wire's set absorbs t's, so the
    // wire becomes the set's root (representative_map, prover.bin's watch keys)
    for (uint32_t j = 0; j < ncg && i + j < consts.size(); j++) connect(Target::wire(row, j), consts[i + j].second);
  }
  // pad to a power of two with NoopGate
  size_t nrows = rows_.size();
  size_t n = 1;
  while (n < nrows) n <<= 1;
  if (n < 8) n = 8;
  while (rows_.size() < n) add_gate(G_NOOP);

  CircuitData cd;
  cd.config = cfg_;
  cd.n = (uint32_t)n;
  cd.simple_gens = simple_gens_;
  cd.copies = copies_;
  cd.num_virtual_targets = nvirt_;
  cd.public_input_targets = public_inputs_;
  cd.degree_bits = 0;
  while ((1u << cd.degree_bits) < n) cd.degree_bits++;
  cd.rows = rows_;
  cd.pi_row = pi_row;
  cd.quotient_degree_factor = cfg_.max_quotient_degree_factor;
  cd.num_public_inputs = (uint32_t)public_inputs_.size();
  // gate set in common-data order (degree, id string)
  bool present[G_NKINDS] = {false};
  for (auto &r : rows_) present[r.kind] = true;
  // CommonCircuitData.gates: sorted by (degree, id string) -- e.g. degree 1:
  // "ConstantGate.." < "PoseidonMdsGate.." < "PublicInputGate"; degree 2:
  // "BaseSumGate.." < "ReducingExtensionGate.." < "ReducingGate.."; degree 3:
  // "ArithmeticExtensionGate.." < "ArithmeticGate.." < "MulExtensionGate.."
  const GateKind order[] = {G_NOOP, G_CONSTANT, G_POSEIDON_MDS, G_PUBLIC_INPUT, G_BASE_SUM, G_REDUCING_EXT,
                            G_REDUCING, G_ARITH_EXT, G_ARITHMETIC, G_MUL_EXT, G_RANDOM_ACCESS, G_COSET_INTERP,
                            G_POSEIDON};
  for (GateKind k : order)
    if (present[k]) {
      cd.gate_kinds.push_back(k);
      const GateParams p = builder_params(k, cfg_);
      cd.gate_params.push_back(p.p0);
      cd.gate_params2.push_back(p.p1);
      cd.gate_params3.push_back(p.p2);
    }
  const uint32_t num_gates = (uint32_t)cd.gate_kinds.size();
  std::vector<GateShape> shapes;
  for (uint32_t i = 0; i < num_gates; i++)
    shapes.push_back(gate_shape(cd.gate_kinds[i], cd.gate_params[i], cd.gate_params2[i], cd.gate_params3[i]));
  uint32_t gate_index[G_NKINDS];
  for (uint32_t i = 0; i < num_gates; i++) gate_index[cd.gate_kinds[i]] = i;
  // selector_polynomials
  const uint32_t max_degree = cd.quotient_degree_factor + 1;
  const uint32_t max_gate_degree = shapes.back().degree;
  if (max_gate_degree + num_gates - 1 <= max_degree) {
    cd.groups.push_back({0, num_gates});
    cd.selector_indices.assign(num_gates, 0);
  } else {
    uint32_t start = 0;
    while (start < num_gates) {
      uint32_t size = 0;
      while (start + size < num_gates && size + shapes[start + size].degree < max_degree) size++;
      if (!size) throw std::runtime_error("gate degree too high for the quotient degree factor");
      cd.groups.push_back({start, start + size});
      start += size;
    }
    for (uint32_t i = 0; i < num_gates; i++)
      for (uint32_t g = 0; g < cd.groups.size(); g++)
        if (i >= cd.groups[g].first && i < cd.groups[g].second) cd.selector_indices.push_back(g);
  }
  const uint32_t nsel = (uint32_t)cd.groups.size();
  // gate constants and constraint count: the maximum over the gates
  uint32_t max_gate_consts = 0;
  cd.num_gate_constraints = 0;
  for (const GateShape &sh : shapes) {
    max_gate_consts = std::max(max_gate_consts, (uint32_t)sh.consts);
    cd.num_gate_constraints = std::max(cd.num_gate_constraints, (uint32_t)sh.constraints);
  }
  cd.num_constants = nsel + max_gate_consts;
  // num_partial_products: routed wires in chunks of qdf, minus one
  cd.num_partial_products = (cfg_.num_routed_wires + cd.quotient_degree_factor - 1) / cd.quotient_degree_factor - 1;
  cd.k_is.resize(cfg_.num_routed_wires);
  for (uint32_t i = 0; i < cfg_.num_routed_wires; i++) cd.k_is[i] = gl::pow(gl::GEN, i);
  {
    uint32_t db = cd.degree_bits;
    while (db > cfg_.final_poly_bits && db + cfg_.rate_bits - cfg_.arity_bits >= cfg_.cap_height) {
      cd.fri_arity_bits.push_back(cfg_.arity_bits);
      db -= cfg_.arity_bits;
    }
  }
  // ---- partition of targets
  const uint32_t W = cfg_.num_wires, R = cfg_.num_routed_wires;
  const size_t nwires = n * (size_t)W;
  auto tindex = [&](Target t) -> uint32_t { return t.is_virtual() ? (uint32_t)(nwires + (t.v & ~Target::VIRT)) : t.row() * W + t.col(); };
  UF uf(nwires + nvirt_);
  for (auto &cp : copies_) uf.unite(tindex(cp.first), tindex(cp.second));
  // partition id per target (dense, in target-index order of first member).
  // Every parent index is below its child's (unite hangs the larger root
  // under the smaller, find halves paths), so a set's root is its first
  // member and one ascending pass labels every target from its parent's label
  uint32_t nparts = 0;
  std::vector<uint32_t> part(nwires + nvirt_);
  for (size_t i = 0; i < nwires + nvirt_; i++) part[i] = uf.p[i] == i ? nparts++ : part[uf.p[i]];
  // ---- sigma polynomials: each partition's routed wires form a cycle
  {
    // each partition's routed wires, in (row, col) order, form a cycle: the
    // successor of routed wire k = row * R + col is the partition's next
    // member, the last member's its first (one backward pass)
    const size_t nk = (size_t)n * R;
    std::vector<uint32_t> succ(nk), first(nparts, UINT32_MAX);
    for (size_t k = nk; k-- > 0;) {
      const uint32_t p = part[(k / R) * W + k % R];
      succ[k] = first[p];
      first[p] = (uint32_t)k;
    }
    for (size_t k = 0; k < nk; k++)
      if (succ[k] == UINT32_MAX) succ[k] = first[part[(k / R) * W + k % R]];
    const uint64_t w = gl::root_of_unity(cd.degree_bits);
    std::vector<F> wpow(n);
    wpow[0] = 1;
    for (uint32_t i = 1; i < n; i++) wpow[i] = gl::mul(wpow[i - 1], w);
    cd.constants_sigmas.assign((size_t)(cd.num_constants + R) * n, 0);
    F *sig = cd.constants_sigmas.data() + (size_t)cd.num_constants * n;
    // sigma_col[row] = k_dcol * w^drow of the successor, column by column
    // (sequential stores instead of one scattered store per wire)
    for (uint32_t col = 0; col < R; col++)
      for (uint32_t row = 0; row < n; row++) {
        const uint32_t d = succ[(size_t)row * R + col];
        sig[(size_t)col * n + row] = gl::mul(cd.k_is[d % R], wpow[d / R]);
      }
    // selectors + gate constants
    for (uint32_t row = 0; row < n; row++) {
      const GateInst &gi = rows_[row];
      uint32_t gidx = gate_index[gi.kind];
      uint32_t grp = cd.selector_indices[gidx];
      for (uint32_t s = 0; s < nsel; s++)
        cd.constants_sigmas[(size_t)s * n + row] = s == grp ? (F)gidx : (nsel > 1 ? UNUSED_SELECTOR : (F)gidx);
      if (max_gate_consts >= 1) cd.constants_sigmas[(size_t)nsel * n + row] = gi.c0;
      if (max_gate_consts >= 2) cd.constants_sigmas[(size_t)(nsel + 1) * n + row] = gi.c1;
    }
  }
  // ---- generator schedule (worklist over partitions) + compact value slots
  {
    auto pt = [&](Target t) { return part[tindex(t)]; };
    auto wpt = [&](uint32_t row, uint32_t col) { return part[row * W + col]; };
    Rows gin, gout;  // per generator: the partitions it reads (sorted, unique) / writes
    for (size_t gi = 0; gi < gens_.size(); gi++) {
      const Gen &g = gens_[gi];
      switch (g.kind) {
        case GEN_CONSTANT:
          for (uint32_t j = 0; j < ncg; j++) gout.push(wpt(g.row, j));
          break;
        case GEN_ARITH:
          for (uint32_t j = 0; j < 3; j++) gin.push(wpt(g.row, 4 * g.op + j));
          gout.push(wpt(g.row, 4 * g.op + 3));
          break;
        case GEN_POSEIDON:
          for (uint32_t j = 0; j < 12; j++) gin.push(wpt(g.row, j));
          gin.push(wpt(g.row, 24));
          for (uint32_t j = 12; j < W; j++)
            if (j != 24) gout.push(wpt(g.row, j));
          break;
        case GEN_BASE_SPLIT:
          gin.push(wpt(g.row, 0));
          for (uint32_t j = 1; j <= base_sum_limbs_; j++) gout.push(wpt(g.row, j));
          break;
        case GEN_EQUALITY:
          gin.push(pt(g.a));
          gin.push(pt(g.b));
          gout.push(pt(g.c));
          gout.push(pt(g.d));
          break;
        case GEN_WIRE_SPLIT:
          gin.push(pt(g.a));
          for (uint32_t j = 0; j < g.op; j++) gout.push(wpt(g.row + j, 0));
          break;
        case GEN_EXT_DIV:
          for (Target t : {g.a, g.b, g.c, g.d}) gin.push(pt(t));
          gout.push(pt(g.e));
          gout.push(pt(g.f));
          break;
        case GEN_RANDOM_ACCESS:
          gin.push(wpt(g.row, ra_wire_index(g.op)));
          for (uint32_t i = 0; i < RA_VEC; i++) gin.push(wpt(g.row, ra_wire_item(i, g.op)));
          gout.push(wpt(g.row, ra_wire_claimed(g.op)));
          for (uint32_t i = 0; i < RA_BITS; i++) gout.push(wpt(g.row, ra_wire_bit(i, g.op)));
          break;
        default: {
          std::vector<std::pair<uint32_t, uint32_t>> rd, wr;
          gen_row_wires(g.kind, g.row, g.op, rd, wr);
          for (auto &rc : rd) gin.push(wpt(rc.first, rc.second));
          for (auto &rc : wr) gout.push(wpt(rc.first, rc.second));
          break;
        }
      }
      gin.close_unique();
      gout.close();
    }
    // value slots: only partitions some generator or input sets; slot 0 is the
    // never-set zero slot shared by everything else
    std::vector<uint32_t> sid(nparts, 0);
    uint32_t nslots = 1;
    auto take = [&](uint32_t p) {
      if (!sid[p]) sid[p] = nslots++;
    };
    for (Target t : inputs_) take(pt(t));
    for (uint32_t p : gout.val) take(p);
    cd.num_slots = nslots;
    for (auto &p : gin.val) p = sid[p];
    for (auto &p : gout.val) p = sid[p];
    // watchers of slot s: woff[s] .. woff[s + 1] of wgen, generators in order
    std::vector<uint32_t> remaining(gens_.size()), woff, wgen;
    {
      std::vector<uint32_t> wpos;
      group_by_key(gin.val, nslots, woff, wpos);
      std::vector<uint32_t> gen_of(gin.val.size());
      for (size_t gi = 0; gi < gens_.size(); gi++) {
        remaining[gi] = gin.off[gi + 1] - gin.off[gi];
        for (uint32_t k = gin.off[gi]; k < gin.off[gi + 1]; k++) gen_of[k] = (uint32_t)gi;
      }
      wgen.resize(wpos.size());
      for (size_t k = 0; k < wpos.size(); k++) wgen[k] = gen_of[wpos[k]];
    }
    std::vector<uint8_t> known(nslots, 0);
    std::vector<uint32_t> queue;
    auto mark = [&](uint32_t s) {
      if (s && !known[s]) {
        known[s] = 1;
        queue.push_back(s);
      }
    };
    for (Target t : inputs_) mark(sid[pt(t)]);
    std::vector<uint32_t> ready;
    for (size_t gi = 0; gi < gens_.size(); gi++)
      if (!remaining[gi]) ready.push_back((uint32_t)gi);
    size_t qh = 0;
    while (true) {
      while (!ready.empty()) {
        uint32_t gi = ready.back();
        ready.pop_back();
        cd.schedule.push_back(gens_[gi]);
        for (uint32_t s : gout[gi]) mark(s);
      }
      if (qh == queue.size()) break;
      uint32_t s = queue[qh++];
      for (uint32_t k = woff[s]; k < woff[s + 1]; k++)
        if (--remaining[wgen[k]] == 0) ready.push_back(wgen[k]);
    }
    if (cd.schedule.size() != gens_.size())
      throw std::runtime_error("witness generation cannot be scheduled: " +
                               std::to_string(gens_.size() - cd.schedule.size()) + " generators never become ready");
    cd.wire_slot.resize(nwires);
    cd.wire_slot_cm.resize(nwires);
    for (size_t i = 0; i < nwires; i++) cd.wire_slot[i] = sid[part[i]];
    // the column-major copy by 64-row tiles (each column's 64 stores contiguous)
    for (uint32_t r0 = 0; r0 < n; r0 += 64) {
      const uint32_t r1 = std::min<uint32_t>(n, r0 + 64);
      for (uint32_t col = 0; col < W; col++)
        for (uint32_t row = r0; row < r1; row++) cd.wire_slot_cm[(size_t)col * n + row] = cd.wire_slot[(size_t)row * W + col];
    }
    cd.virt_slot.resize(nvirt_);
    for (uint32_t v = 0; v < nvirt_; v++) cd.virt_slot[v] = sid[part[nwires + v]];
    {
      auto z = const_to_target_.find(0);
      cd.zero_const_slot = z == const_to_target_.end() ? 0 : sid[pt(z->second)];
    }
    for (Gen &g : cd.schedule) {
      auto ws = [&](uint32_t row, uint32_t col) { return sid[wpt(row, col)]; };
      switch (g.kind) {
        case GEN_ARITH:
          for (uint32_t j = 0; j < 4; j++) g.s[j] = ws(g.row, 4 * g.op + j);
          g.k0 = rows_[g.row].c0;
          g.k1 = rows_[g.row].c1;
          break;
        case GEN_EQUALITY:
          g.s[0] = sid[pt(g.a)];
          g.s[1] = sid[pt(g.b)];
          g.s[2] = sid[pt(g.c)];
          g.s[3] = sid[pt(g.d)];
          break;
        case GEN_CONSTANT:
          g.s[0] = ws(g.row, 0);
          g.s[1] = ncg > 1 ? ws(g.row, 1) : 0;
          g.k0 = rows_[g.row].c0;
          g.k1 = rows_[g.row].c1;
          break;
        case GEN_BASE_SPLIT:
          g.s[0] = ws(g.row, 0);
          break;
        case GEN_WIRE_SPLIT:
          g.s[0] = sid[pt(g.a)];
          break;
        case GEN_EXT_DIV:
          g.s[0] = sid[pt(g.a)];
          g.s[1] = sid[pt(g.b)];
          g.s[2] = sid[pt(g.c)];
          g.s[3] = sid[pt(g.d)];
          g.s[4] = sid[pt(g.e)];
          g.s[5] = sid[pt(g.f)];
          break;
        case GEN_ARITH_EXT:
        case GEN_MUL_EXT:
          g.k0 = rows_[g.row].c0;
          g.k1 = rows_[g.row].c1;
          break;
        default:
          break;
      }
    }
    for (Target t : public_inputs_) cd.pi_slots.push_back(sid[pt(t)]);
    for (Target t : zk_cells) cd.zk_slots.push_back(sid[pt(t)]);
    // device schedule: a generator runs at the first level where all its
    // inputs exist; its outputs exist from the next level on.  Every generator
    // kind has a device form (witness.hip), the recursive verifier's included.
    if (cd.device_witness) {
      std::vector<uint8_t> is_in(nslots, 0);
      for (Target t : inputs_) {
        const uint32_t s = sid[pt(t)];
        if (s && !is_in[s]) {
          is_in[s] = 1;
          cd.input_slots.push_back(s);
        }
      }
      const size_t ng = cd.schedule.size();
      Rows rds, wrs;  // per generator: the slots it reads / writes
      std::vector<uint32_t> rd, wr;
      for (size_t i = 0; i < ng; i++) {
        const Gen &g = cd.schedule[i];
        rd.clear();
        wr.clear();
        switch (g.kind) {
          case GEN_CONSTANT: wr = {g.s[0], g.s[1]}; break;
          case GEN_ARITH: rd = {g.s[0], g.s[1], g.s[2]}; wr = {g.s[3]}; break;
          case GEN_EQUALITY: rd = {g.s[0], g.s[1]}; wr = {g.s[2], g.s[3]}; break;
          case GEN_BASE_SPLIT:
            rd = {g.s[0]};
            for (uint32_t j = 1; j <= base_sum_limbs_; j++) wr.push_back(cd.wire_slot[(size_t)g.row * W + j]);
            break;
          case GEN_POSEIDON:
            for (uint32_t j = 0; j < 12; j++) rd.push_back(cd.wire_slot[(size_t)g.row * W + j]);
            rd.push_back(cd.wire_slot[(size_t)g.row * W + 24]);
            for (uint32_t j = 12; j < W; j++)
              if (j != 24) wr.push_back(cd.wire_slot[(size_t)g.row * W + j]);
            break;
          case GEN_WIRE_SPLIT:
            rd = {g.s[0]};
            for (uint32_t j = 0; j < g.op; j++) wr.push_back(cd.wire_slot[(size_t)(g.row + j) * W]);
            break;
          case GEN_EXT_DIV:
            rd = {g.s[0], g.s[1], g.s[2], g.s[3]};
            wr = {g.s[4], g.s[5]};
            break;
          case GEN_RANDOM_ACCESS:
            rd.push_back(cd.wire_slot[(size_t)g.row * W + ra_wire_index(g.op)]);
            for (uint32_t i = 0; i < RA_VEC; i++) rd.push_back(cd.wire_slot[(size_t)g.row * W + ra_wire_item(i, g.op)]);
            wr.push_back(cd.wire_slot[(size_t)g.row * W + ra_wire_claimed(g.op)]);
            for (uint32_t i = 0; i < RA_BITS; i++) wr.push_back(cd.wire_slot[(size_t)g.row * W + ra_wire_bit(i, g.op)]);
            break;
          default: {
            std::vector<std::pair<uint32_t, uint32_t>> rw, ww;
            gen_row_wires(g.kind, g.row, g.op, rw, ww);
            for (auto &rc : rw) rd.push_back(cd.wire_slot[(size_t)rc.first * W + rc.second]);
            for (auto &rc : ww) wr.push_back(cd.wire_slot[(size_t)rc.first * W + rc.second]);
            break;
          }
        }
        for (uint32_t v : rd) rds.push(v);
        rds.close();
        for (uint32_t v : wr) wrs.push(v);
        wrs.close();
      }
      // host chains (CircuitData::host_gens): forward, the Poseidon (and
      // constant) generators computable from inputs alone with their chain
      // depth in permutations; backward, those at least tmin deep and every
      // such generator feeding one
      const uint32_t tmin = (uint32_t)qpk::path_opt("host_chain", HOST_CHAIN_MIN);  // path hook host_chain
      std::vector<uint8_t> on_host(ng, 0);
      if (tmin) {
        std::vector<uint8_t> hostable(ng, 0), hw(nslots, 0), need(nslots, 0);
        std::vector<uint32_t> depth(ng, 0), sdepth(nslots, 0);
        for (size_t i = 0; i < ng; i++) {
          const uint32_t k = cd.schedule[i].kind;
          if (k != GEN_POSEIDON && k != GEN_CONSTANT) continue;
          bool ok = true;
          uint32_t d = 0;
          for (uint32_t s : rds[i]) {
            if (s && !is_in[s] && !hw[s]) {
              ok = false;
              break;
            }
            d = std::max(d, sdepth[s]);
          }
          if (!ok) continue;
          hostable[i] = 1;
          depth[i] = d + (k == GEN_POSEIDON ? 1 : 0);
          for (uint32_t s : wrs[i])
            if (s) {
              hw[s] = 1;
              sdepth[s] = std::max(sdepth[s], depth[i]);
            }
        }
        for (size_t i = ng; i-- > 0;) {
          if (!hostable[i]) continue;
          bool take = depth[i] >= tmin;
          for (uint32_t s : wrs[i]) take = take || (s && need[s]);
          if (!take) continue;
          on_host[i] = 1;
          for (uint32_t s : rds[i]) need[s] = 1;
        }
        // segments: the constants first (every chain reads them), then the
        // independent chains -- union-find over slots one host generator
        // writes and another reads or writes -- each in schedule order
        std::vector<uint32_t> uf(ng), writer(nslots, UINT32_MAX);
        std::iota(uf.begin(), uf.end(), 0u);
        auto find = [&](uint32_t x) {
          while (uf[x] != x) x = uf[x] = uf[uf[x]];
          return x;
        };
        std::vector<uint32_t> cons;
        for (size_t i = 0; i < ng; i++) {
          if (!on_host[i]) continue;
          for (uint32_t s : wrs[i])
            if (s && !is_in[s]) {
              is_in[s] = 1;
              cd.input_slots.push_back(s);
            }
          if (cd.schedule[i].kind == GEN_CONSTANT) {
            cons.push_back((uint32_t)i);
            continue;
          }
          for (uint32_t s : rds[i])
            if (s && writer[s] != UINT32_MAX) uf[find((uint32_t)i)] = find(writer[s]);
          for (uint32_t s : wrs[i])
            if (s) {
              if (writer[s] != UINT32_MAX) uf[find((uint32_t)i)] = find(writer[s]);
              writer[s] = (uint32_t)i;
            }
        }
        cd.host_gens = cons;
        cd.host_seg_off = {0, (uint32_t)cons.size()};
        std::vector<uint32_t> roots;
        std::vector<std::vector<uint32_t>> segs;
        std::unordered_map<uint32_t, uint32_t> seg_of;
        for (size_t i = 0; i < ng; i++) {
          if (!on_host[i] || cd.schedule[i].kind == GEN_CONSTANT) continue;
          const uint32_t r = find((uint32_t)i);
          auto it = seg_of.find(r);
          if (it == seg_of.end()) {
            it = seg_of.emplace(r, (uint32_t)segs.size()).first;
            segs.emplace_back();
          }
          segs[it->second].push_back((uint32_t)i);
        }
        for (auto &sg : segs) {
          cd.host_gens.insert(cd.host_gens.end(), sg.begin(), sg.end());
          cd.host_seg_off.push_back((uint32_t)cd.host_gens.size());
        }
        if (cd.host_gens.empty()) cd.host_seg_off.clear();
      }
      std::sort(cd.input_slots.begin(), cd.input_slots.end());
      const uint32_t INF = 0xFFFFFFFFu;
      std::vector<uint32_t> avail(nslots, INF);
      avail[0] = 0;
      for (uint32_t s : cd.input_slots) avail[s] = 0;
      std::vector<uint32_t> lvl(ng, INF);
      uint32_t nlev = 0;
      // writers per slot (saturating at 2): host-set slots count as one
      std::vector<uint8_t> nwr(nslots, 0);
      for (uint32_t s : cd.input_slots) nwr[s] = 1;
      for (uint32_t s : cd.zk_slots) nwr[s] = 1;
      for (size_t i = 0; i < ng; i++) {
        if (on_host[i]) continue;
        uint32_t l = 0;
        for (uint32_t s : rds[i]) {
          if (avail[s] == INF) throw std::runtime_error("device witness schedule: input not available");
          l = std::max(l, avail[s]);
        }
        lvl[i] = l;
        nlev = std::max(nlev, l + 1);
        for (uint32_t s : wrs[i]) {
          if (s) avail[s] = std::min(avail[s], l + 1);
          if (nwr[s] < 2) nwr[s]++;
        }
      }
      // slots with one writer take a plain store on the device; the shared
      // zero slot and slots written twice keep the compare-and-swap that
      // detects "set twice with different values" (DEV_MULTI, witness.hip)
      nwr[0] = 2;
      if (nslots >= DEV_MULTI) throw std::runtime_error("device witness schedule: too many value slots");
      auto flag = [&](uint32_t s) { return s < nslots && nwr[s] >= 2 ? s | DEV_MULTI : s; };
      cd.dev_wslot.resize(cd.wire_slot.size());
      for (size_t i = 0; i < cd.wire_slot.size(); i++) cd.dev_wslot[i] = flag(cd.wire_slot[i]);
      cd.level_off.assign(nlev + 1, 0);
      for (uint32_t l : lvl)
        if (l != INF) cd.level_off[l + 1]++;
      for (uint32_t l = 0; l < nlev; l++) cd.level_off[l + 1] += cd.level_off[l];
      std::vector<uint32_t> fill(cd.level_off.begin(), cd.level_off.end() - 1);
      cd.dev_gens.resize(ng - cd.host_gens.size());
      // within a level, generators of one kind are contiguous (a wave then runs
      // one switch arm instead of serialising several)
      std::vector<uint32_t> order;
      for (size_t i = 0; i < ng; i++)
        if (!on_host[i]) order.push_back((uint32_t)i);
      std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
        return lvl[x] != lvl[y] ? lvl[x] < lvl[y] : cd.schedule[x].kind < cd.schedule[y].kind;
      });
      for (size_t k = 0; k < order.size(); k++) {
        const size_t i = order[k];
        const Gen &g = cd.schedule[i];
        DevGen &d = cd.dev_gens[fill[lvl[i]]++];
        d.kind = g.kind;
        d.row = g.row;
        for (int j = 0; j < 4; j++) d.s[j] = flag(g.s[j]);
        d.k0 = g.k0;
        d.k1 = g.k1;
        if (g.kind == GEN_WIRE_SPLIT) {
          d.s[1] = g.op;  // number of BaseSum gates from `row`
        } else if (g.kind == GEN_EXT_DIV) {
          d.k0 = flag(g.s[4]) | (uint64_t)flag(g.s[5]) << 32;  // quotient slots
        } else if (g.kind == GEN_RANDOM_ACCESS || g.kind == GEN_ARITH_EXT || g.kind == GEN_MUL_EXT) {
          d.s[0] = g.op;  // copy / op
        }
      }
      // each level's Poseidon generators are contiguous (kind order): their
      // range lets the device pick the cooperative form for narrow levels
      cd.level_pos.assign(2 * (size_t)nlev, 0);
      for (uint32_t l = 0; l < nlev; l++) {
        uint32_t first = cd.level_off[l + 1], cnt = 0;
        for (uint32_t i = cd.level_off[l]; i < cd.level_off[l + 1]; i++)
          if (cd.dev_gens[i].kind == GEN_POSEIDON) {
            first = std::min(first, i);
            cnt++;
          }
        cd.level_pos[2 * l] = first;
        cd.level_pos[2 * l + 1] = cnt;
      }
    }
  }
  return cd;
}

uint32_t CircuitData::slot_of(Target t) const {
  if (t.is_virtual()) {
    const uint32_t v = t.v & ~Target::VIRT;
    return v < virt_slot.size() ? virt_slot[v] : 0xFFFFFFFFu;
  }
  return wire_slot[(size_t)t.row() * config.num_wires + t.col()];
}

// ---------------------------------------------------------------- serialization

namespace {
struct ByteWriter {
  std::vector<uint8_t> b;
  void u64(uint64_t v) {
    for (int i = 0; i < 8; i++) b.push_back((uint8_t)(v >> (8 * i)));
  }
  void u32(uint32_t v) {
    for (int i = 0; i < 4; i++) b.push_back((uint8_t)(v >> (8 * i)));
  }
  void u8(uint8_t v) { b.push_back(v); }
};
void write_fri_config(ByteWriter &w, const CircuitConfig &c) {
  w.u64(c.rate_bits);
  w.u64(c.cap_height);
  w.u64(c.num_query_rounds);
  w.u32(c.pow_bits);
  w.u8(1);  // FriReductionStrategy::ConstantArityBits
  w.u64(c.arity_bits);
  w.u64(c.final_poly_bits);
}
}  // namespace

std::vector<uint8_t> CircuitData::common_bytes() const {
  ByteWriter w;
  const CircuitConfig &c = config;
  w.u64(c.num_wires);
  w.u64(c.num_routed_wires);
  w.u64(c.num_constants);
  w.u64(c.security_bits);
  w.u64(c.num_challenges);
  w.u64(c.max_quotient_degree_factor);
  w.u8(c.use_base_arithmetic_gate);
  w.u8(c.zero_knowledge);
  write_fri_config(w, c);
  write_fri_config(w, c);
  w.u64(fri_arity_bits.size());
  for (auto a : fri_arity_bits) w.u64(a);
  w.u64(degree_bits);
  // FriParams.hiding: the reference's zk config under the workspace's
  // `no_random` feature commits without salt columns (dummy_proof_zk.bin,
  // verified in tests/test_current_circuit_fixture.py), i.e. no hiding
  w.u8(0);
  w.u64(selector_indices.size());
  for (auto s : selector_indices) w.u64(s);
  w.u64(groups.size());
  for (auto &g : groups) {
    w.u64(g.first);
    w.u64(g.second);
  }
  w.u64(quotient_degree_factor);
  w.u64(num_gate_constraints);
  w.u64(num_constants);
  w.u64(num_public_inputs);
  w.u64(k_is.size());
  for (auto k : k_is) w.u64(k);
  w.u64(num_partial_products);
  w.u64(0);  // num_lookup_polys
  w.u64(0);  // num_lookup_selectors
  w.u64(0);  // luts
  w.u64(gate_kinds.size());
  for (size_t i = 0; i < gate_kinds.size(); i++) {
    const GateKind k = gate_kinds[i];
    const uint32_t prm[3] = {gate_params[i], gate_params2[i], gate_params3[i]};
    w.u32(serial_id(k));
    for (uint32_t j = 0; j < serial_params(k); j++) w.u64(prm[j]);
    if (k == G_COSET_INTERP) {  // CosetInterpolationGate { subgroup_bits, degree, barycentric_weights }
      const uint32_t np = 1u << gate_params[i];
      const F om = gl::root_of_unity(gate_params[i]), ninv = gl::inv(np);
      w.u64(np);
      for (uint32_t j = 0; j < np; j++) w.u64(gl::mul(gl::pow(om, j), ninv));  // 1 / prod_{l != j}(w^j - w^l) = w^j / n
    }
  }
  return w.b;
}

// ---------------------------------------------------------------- witness

Witness::Witness(const CircuitData &cd, F *vals) : cd_(cd), known_(cd.num_slots, 0) {
  if (vals) {
    vals_ = vals;
    memset(vals_, 0, (size_t)cd.num_slots * 8);
  } else {
    own_.assign(cd.num_slots, 0);
    vals_ = own_.data();
  }
}

bool Witness::set_slot(uint32_t s, F v) {
  v = gl::canon(v);
  if (!s) return false;  // the shared zero slot is never settable
  if (known_[s]) return vals_[s] == v;
  known_[s] = 1;
  vals_[s] = v;
  return true;
}

bool Witness::set(Target t, F v) {
  uint32_t s = cd_.slot_of(t);
  if (s == 0xFFFFFFFFu) return false;
  return set_slot(s, v);
}

bool Witness::set_wire(uint32_t row, uint32_t col, F v) {
  return set_slot(cd_.wire_slot[(size_t)row * cd_.config.num_wires + col], v);
}

F Witness::wire(uint32_t row, uint32_t col) const {
  return vals_[cd_.wire_slot[(size_t)row * cd_.config.num_wires + col]];
}

namespace {

inline F red128(unsigned __int128 x) { return gl::reduce128((uint64_t)x, (uint64_t)(x >> 64)); }

// x^7 on the host (64x64->128 products)
inline F sbox_h(F x) {
  const F x2 = red128((unsigned __int128)x * x);
  const F x3 = red128((unsigned __int128)x2 * x);
  const F x4 = red128((unsigned __int128)x2 * x2);
  return red128((unsigned __int128)x3 * x4);
}

constexpr uint64_t MDS_C[12] = {17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20};

// MDS layer with the small circulant constants, one 128-bit accumulation and
// one reduction per lane (each term < 2^70, 13 terms < 2^74)
inline void mds_h(F s[12]) {
  F o[12];
#pragma unroll
  for (int r = 0; r < 12; r++) {
    unsigned __int128 acc = 0;
#pragma unroll
    for (int i = 0; i < 12; i++) acc += (unsigned __int128)s[(i + r) % 12] * MDS_C[i];
    if (r == 0) acc += (unsigned __int128)s[0] * 8;
    o[r] = red128(acc);
  }
#pragma unroll
  for (int r = 0; r < 12; r++) s[r] = o[r];
}

// inverses of the small integers 1..SMALL_INV: EqualityGenerator inverts
// x - y, which in the reference circuits is mostly a short index distance
constexpr uint32_t SMALL_INV = 4096;
const F *small_inverses() {
  static const std::vector<F> t = [] {
    std::vector<F> v(SMALL_INV + 1, 0);
    v[1] = 1;
    for (uint32_t k = 2; k <= SMALL_INV; k++)  // inv(k) = -(p / k) * inv(p mod k)
      v[k] = gl::neg(gl::mul(gl::P / k, v[gl::P % k]));
    return v;
  }();
  return t.data();
}

inline F inv_diff(F x, F y) {
  if (x >= y) {
    const F d = x - y;
    return d <= SMALL_INV ? small_inverses()[d] : gl::inv(d);
  }
  const F d = y - x;
  return d <= SMALL_INV ? gl::neg(small_inverses()[d]) : gl::inv(gl::sub(x, y));
}

}  // namespace

bool Witness::generate(std::string &err) {
  for (const Gen &g : cd_.schedule)
    if (!run(g, err)) return false;
  return true;
}

bool Witness::generate_host_chains(std::string &err, int seg) {
  const auto &off = cd_.host_seg_off;
  if (off.empty()) return true;
  const uint32_t lo = seg < 0 ? 0 : off[seg], hi = seg < 0 ? off.back() : off[seg + 1];
  for (uint32_t k = lo; k < hi; k++)
    if (!run(cd_.schedule[cd_.host_gens[k]], err)) return false;
  return true;
}

bool Witness::run(const Gen &g, std::string &err) {
  const uint32_t W = cd_.config.num_wires;
  const uint32_t L = cd_.config.num_routed_wires - 1 < 63 ? cd_.config.num_routed_wires - 1 : 63;
  const uint32_t zslot = cd_.zero_const_slot;
  F *v = vals_;
  {
    bool ok = true;
    switch (g.kind) {
      case GEN_CONSTANT:
        ok = set_slot(g.s[0], g.k0) && (cd_.config.num_constants < 2 || set_slot(g.s[1], g.k1));
        break;
      case GEN_ARITH: {
        // output = c0 * m0 * m1 + c1 * addend
        const F m = gl::mul(gl::mul(v[g.s[0]], v[g.s[1]]), g.k0);
        ok = set_slot(g.s[3], gl::add(m, gl::mul(v[g.s[2]], g.k1)));
        break;
      }
      case GEN_BASE_SPLIT: {
        const F sum = v[g.s[0]];
        const uint32_t *ws = cd_.wire_slot.data() + (size_t)g.row * W + 1;
        for (uint32_t l = 0; l < L && ok; l++) {
          const F bit = (sum >> l) & 1;
          // limbs past a range check's width are connected to zero(): they
          // only need checking (a set bit there is the reference's conflict)
          if (ws[l] == zslot && zslot) ok = bit == 0;
          else ok = set_slot(ws[l], bit);
        }
        break;
      }
      case GEN_EQUALITY: {
        const F x = v[g.s[0]], y = v[g.s[1]];
        ok = set_slot(g.s[2], x == y ? 1 : 0) && set_slot(g.s[3], x == y ? 0 : inv_diff(x, y));
        break;
      }
      case GEN_WIRE_SPLIT: {
        F x = v[g.s[0]];
        for (uint32_t j = 0; j < g.op && ok; j++) {
          const F sum = L < 64 ? (x & ((1ull << L) - 1)) : x;
          x = L < 64 ? x >> L : 0;
          ok = set_wire(g.row + j, 0, sum);
        }
        break;
      }
      case GEN_EXT_DIV: {
        const gl::ext den{v[g.s[2]], v[g.s[3]]};
        if (!den.c0 && !den.c1) {
          err = "division by zero in an extension-field quotient";
          return false;
        }
        const gl::ext q = gl::ext_mul(gl::ext{v[g.s[0]], v[g.s[1]]}, gl::ext_inv(den));
        ok = set_slot(g.s[4], q.c0) && set_slot(g.s[5], q.c1);
        break;
      }
      case GEN_RANDOM_ACCESS: {
        const F idx = wire(g.row, ra_wire_index(g.op));
        if (idx >= RA_VEC) {
          err = "random access index " + std::to_string(idx) + " out of range";
          return false;
        }
        ok = set_wire(g.row, ra_wire_claimed(g.op), wire(g.row, ra_wire_item((uint32_t)idx, g.op)));
        for (uint32_t i = 0; i < RA_BITS && ok; i++) ok = set_wire(g.row, ra_wire_bit(i, g.op), (idx >> i) & 1);
        break;
      }
      case GEN_ARITH_EXT:
      case GEN_MUL_EXT: {
        // ArithmeticExtensionGenerator / MulExtensionGenerator: c0 m0 m1 (+ c1 addend)
        const bool ae = g.kind == GEN_ARITH_EXT;
        const uint32_t o = ae ? 8 * g.op : 6 * g.op;
        gl::ext r = gl::ext_scale(gl::ext_mul(gl::ext{wire(g.row, o), wire(g.row, o + 1)},
                                              gl::ext{wire(g.row, o + 2), wire(g.row, o + 3)}), g.k0);
        if (ae) r = gl::ext_add(r, gl::ext_scale(gl::ext{wire(g.row, o + 4), wire(g.row, o + 5)}, g.k1));
        const uint32_t oo = ae ? o + 6 : o + 4;
        ok = set_wire(g.row, oo, r.c0) && set_wire(g.row, oo + 1, r.c1);
        break;
      }
      case GEN_REDUCING:
      case GEN_REDUCING_EXT: {
        // ReducingGenerator: acc <- acc * alpha + coeff_i, every accumulator written
        const bool base = g.kind == GEN_REDUCING;
        const uint32_t nc = base ? RED_COEFFS : REDE_COEFFS, cw = base ? 1 : 2;
        const gl::ext alpha{wire(g.row, 2), wire(g.row, 3)};
        gl::ext acc{wire(g.row, 4), wire(g.row, 5)};
        for (uint32_t i = 0; i < nc && ok; i++) {
          const gl::ext c{wire(g.row, 6 + cw * i), base ? 0 : wire(g.row, 7 + 2 * i)};
          acc = gl::ext_add(gl::ext_mul(acc, alpha), c);
          const uint32_t aw = i + 1 == nc ? 0 : 6 + cw * nc + 2 * i;
          ok = set_wire(g.row, aw, acc.c0) && set_wire(g.row, aw + 1, acc.c1);
        }
        break;
      }
      case GEN_POSEIDON_MDS: {
        // PoseidonMdsGenerator: the MDS layer of each component
        F a[12], b[12];
        for (int i = 0; i < 12; i++) {
          a[i] = wire(g.row, 2 * i);
          b[i] = wire(g.row, 2 * i + 1);
        }
        mds_h(a);
        mds_h(b);
        for (int i = 0; i < 12 && ok; i++) ok = set_wire(g.row, 24 + 2 * i, a[i]) && set_wire(g.row, 25 + 2 * i, b[i]);
        break;
      }
      case GEN_COSET_INTERP: {
        // InterpolationGenerator (gates/coset_interpolation.rs): shifted point,
        // partial barycentric sums over chunks of the subgroup, the value
        const F shift = wire(g.row, 0);
        if (!shift) {
          err = "coset interpolation with a zero shift";
          return false;
        }
        const gl::ext pt = gl::ext_scale(gl::ext{wire(g.row, CI_EVAL_POINT), wire(g.row, CI_EVAL_POINT + 1)},
                                         gl::inv(shift));
        ok = set_wire(g.row, CI_SHIFTED, pt.c0) && set_wire(g.row, CI_SHIFTED + 1, pt.c1);
        const F om = gl::root_of_unity(CI_BITS), ninv = gl::inv(CI_POINTS);
        gl::ext ev{0, 0}, pr{1, 0};
        uint32_t lo = 0, hi = CI_DEGREE;
        for (uint32_t it = 0; ok; it++) {
          for (uint32_t i = lo; i < hi; i++) {
            const F x = gl::pow(om, i);
            const gl::ext term = gl::ext_sub(pt, gl::ext{x, 0});
            const gl::ext v = gl::ext_scale(gl::ext{wire(g.row, CI_VALUES + 2 * i), wire(g.row, CI_VALUES + 2 * i + 1)},
                                            gl::mul(x, ninv));
            ev = gl::ext_add(gl::ext_mul(ev, term), gl::ext_mul(v, pr));
            pr = gl::ext_mul(pr, term);
          }
          if (it == CI_NINT) break;
          ok = set_wire(g.row, CI_INTER + 2 * it, ev.c0) && set_wire(g.row, CI_INTER + 2 * it + 1, ev.c1) &&
               set_wire(g.row, CI_INTER + 2 * (CI_NINT + it), pr.c0) &&
               set_wire(g.row, CI_INTER + 2 * (CI_NINT + it) + 1, pr.c1);
          lo = 1 + (CI_DEGREE - 1) * (it + 1);
          hi = std::min(lo + CI_DEGREE - 1, CI_POINTS);
        }
        if (ok) ok = set_wire(g.row, CI_EVAL_VALUE, ev.c0) && set_wire(g.row, CI_EVAL_VALUE + 1, ev.c1);
        break;
      }
      case GEN_POSEIDON: {
        // PoseidonGenerator (gates/poseidon.rs): swap, deltas, S-box inputs
        // of full rounds 1..3, partial rounds, second-half full rounds, outputs
        const uint32_t *ws = cd_.wire_slot.data() + (size_t)g.row * W;
        F s[12];
        for (int i = 0; i < 12; i++) s[i] = v[ws[i]];
        const F swap = v[ws[24]];
        for (int i = 0; i < 4 && ok; i++) ok = set_slot(ws[25 + i], gl::mul(swap, gl::sub(s[i + 4], s[i])));
        if (swap == 1)
          for (int i = 0; i < 4; i++) std::swap(s[i], s[i + 4]);
        int rc = 0;
        for (int r = 0; r < 4; r++, rc++) {
          for (int i = 0; i < 12; i++) s[i] = gl::add(s[i], ps::rc(rc * 12 + i));
          if (r)
            for (int i = 0; i < 12 && ok; i++) ok = set_slot(ws[29 + (r - 1) * 12 + i], s[i]);
          for (int i = 0; i < 12; i++) s[i] = sbox_h(s[i]);
          mds_h(s);
        }
        for (int r = 0; r < 22; r++, rc++) {
          for (int i = 0; i < 12; i++) s[i] = gl::add(s[i], ps::rc(rc * 12 + i));
          if (ok) ok = set_slot(ws[65 + r], s[0]);
          s[0] = sbox_h(s[0]);
          mds_h(s);
        }
        for (int r = 0; r < 4; r++, rc++) {
          for (int i = 0; i < 12; i++) s[i] = gl::add(s[i], ps::rc(rc * 12 + i));
          for (int i = 0; i < 12 && ok; i++) ok = set_slot(ws[87 + r * 12 + i], s[i]);
          for (int i = 0; i < 12; i++) s[i] = sbox_h(s[i]);
          mds_h(s);
        }
        for (int i = 0; i < 12 && ok; i++) ok = set_slot(ws[12 + i], s[i]);
        break;
      }
    }
    if (!ok) {
      err = "Partition containing a target was set twice with different values (generator kind " +
            std::to_string(g.kind) + " at row " + std::to_string(g.row) + ")";
      return false;
    }
  }
  return true;
}

void Witness::wires_matrix(F *out) const {
  const size_t m = (size_t)cd_.n * cd_.config.num_wires;
  const uint32_t *cm = cd_.wire_slot_cm.data();
  for (size_t i = 0; i < m; i++) out[i] = vals_[cm[i]];
}

std::vector<F> Witness::public_inputs() const {
  std::vector<F> v;
  for (uint32_t s : cd_.pi_slots) v.push_back(vals_[s]);
  return v;
}

}  // namespace qc
