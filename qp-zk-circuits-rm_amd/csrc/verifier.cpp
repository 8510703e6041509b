// verifier.cpp — the native batch verifier's host part and C ABI (qpgpu.h
// "batch proof verifier").  Follows upstream plonky2 (qp-plonky2 1.1.1):
//   plonk/verifier.rs            verify / verify_with_challenges
//   plonk/get_challenges.rs      get_challenges
//   plonk/vanishing_poly.rs      eval_vanishing_poly, check_partial_products
//   gates/*::eval_unfiltered     (gate_constraints.h, shared with the recursive verifier)
//   fri/verifier.rs              verify_fri_proof, PrecomputedReducedOpenings
// Per proof, on a small host pool: parse (every length and every field element
// checked), transcript, zeta^n != 1, the vanishing identity at zeta, PoW, the
// reduced openings; the proof's query data is repacked into aligned u64 arrays.
// The query rounds of the whole chunk then run on the device (verifier.hip) or,
// without a context, through the same per-lane code on the host pool.
#include "../../include/qpgpu.h"
#include <string.h>
#include <memory>
#include <new>
#include <string>
#include <thread>
#include <vector>
#include "ctx.h"
#include "field.h"
#include "gate_constraints.h"
#include "host_util.h"
#include "poseidon.h"
#include "recursion.h"
#include "verifier.h"

namespace {

using gl::ext;
using qr::InnerCommon;
typedef uint64_t F;

const uint64_t UNUSED_SELECTOR = 0xFFFFFFFFull;

// plain extension values as gate_constraints.h's arithmetic
struct VG : qr::AlgOps<VG, gl::ext> {
  using E = gl::ext;
  E ext_zero() { return E{0, 0}; }
  E ext_const(F c0, F c1 = 0) { return E{c0, c1}; }
  E ext(F x) { return E{x, 0}; }
  E add(E a, E c) { return gl::ext_add(a, c); }
  E sub(E a, E c) { return gl::ext_sub(a, c); }
  E mul(E a, E c) { return gl::ext_mul(a, c); }
  E mul_add(E a, E c, E d) { return gl::ext_add(gl::ext_mul(a, c), d); }
  E mul_sub(E a, E c, E d) { return gl::ext_sub(gl::ext_mul(a, c), d); }
  E scale(E a, F c) { return gl::ext_scale(a, c); }
  E add_const(E a, F c) { return E{gl::add(a.c0, c), a.c1}; }
  E mul_many(const std::vector<E> &v) {
    E r{1, 0};
    for (E x : v) r = gl::ext_mul(r, x);
    return r;
  }
  E arithmetic_extension(F c0, F c1, E m0, E m1, E addend) {
    return gl::ext_add(gl::ext_scale(gl::ext_mul(m0, m1), c0), gl::ext_scale(addend, c1));
  }
  E reduce(E base, const std::vector<E> &t) {
    E acc{0, 0};
    for (size_t i = t.size(); i-- > 0;) acc = gl::ext_add(gl::ext_mul(acc, base), t[i]);
    return acc;
  }
  E mul_const_add(F c, E x, E y) { return gl::ext_add(gl::ext_scale(x, c), y); }
  std::vector<E> poseidon_mds(const std::vector<E> &s) {
    std::vector<E> o(12);
    for (int r = 0; r < 12; r++) {
      E acc{0, 0};
      for (int i = 0; i < 12; i++) acc = gl::ext_add(acc, gl::ext_scale(s[(i + r) % 12], ps::mds_circ(i)));
      if (r == 0) acc = gl::ext_add(acc, gl::ext_scale(s[0], 8));
      o[r] = acc;
    }
    return o;
  }
  E exp_u64(E x, uint64_t e) { return gl::ext_pow(x, e); }
};

struct Dims {
  uint32_t log_n, log_N, cap_h, capw, nq, nc, salt, nlayers, final_len, ncls, init_sibs;
  uint32_t width[4], unsalted[4];
  uint32_t cls_width[qv::MAX_CLASSES], cls_sibs[qv::MAX_CLASSES], cls_shift[qv::MAX_CLASSES];
  uint32_t arity_bits[qv::MAX_LAYERS];
  uint32_t nopen;      // extension openings in the proof
  uint32_t pp_stride;  // words of the per-proof block
  size_t fixed_len;    // proof bytes without the public inputs
};

// the chunk's arrays, as word offsets into one buffer (dense for nb proofs)
struct Layout {
  size_t leaves[qv::MAX_CLASSES], sibs[qv::MAX_CLASSES], caps[qv::MAX_CLASSES], idx[qv::MAX_CLASSES], pp, words;
};

Layout make_layout(const Dims &d, uint32_t nb) {
  Layout L{};
  size_t o = 0;
  const size_t lanes = (size_t)nb * d.nq;
  L.caps[0] = o;
  o += d.capw;
  for (uint32_t c = 0; c < d.ncls; c++) {
    L.leaves[c] = o;
    o += lanes * d.cls_width[c];
    L.sibs[c] = o;
    o += lanes * d.cls_sibs[c] * 4;
    if (c) {
      L.caps[c] = o;
      o += (size_t)nb * d.capw;
    }
    L.idx[c] = o;
    o += (lanes + 1) / 2;
  }
  L.pp = o;
  o += (size_t)nb * d.pp_stride;
  L.words = o;
  return L;
}

struct HostHash {
  static void permute(uint64_t s[12]) { ps::permute(s); }
  static void node(uint64_t s[12]) { ps::permute(s); }
};

}  // namespace

namespace qv {
void host_paths(const PathJob &job, uint32_t cls, uint32_t lo, uint32_t hi, uint32_t ok_base) {
  for (uint32_t i = lo; i < hi; i++) job.ok[ok_base + i] = path_ok<HostHash>(job.cls[cls], job.cap_height, i) ? 1 : 0;
}
void host_fri(const FriJob &job, uint32_t lo, uint32_t hi) {
  for (uint32_t i = lo; i < hi; i++) job.code[i] = fri_query(job, i);
}
}  // namespace qv

struct qp_verifier {
  qp_ctx *ctx = nullptr;
  bool usable = false;
  InnerCommon c;
  Dims d{};
  std::vector<uint64_t> cap;  // constants||sigmas cap
  uint64_t digest[4] = {0, 0, 0, 0};
  uint32_t max_batch = 0;
  std::string err;
  std::unique_ptr<qh::ThreadPool> pool;
  // chunk buffers
  uint64_t *h_buf = nullptr, *d_buf = nullptr;  // h_buf pinned with a context
  uint8_t *d_ok = nullptr;
  uint32_t *d_code = nullptr;
  std::vector<uint8_t> h_ok;
  std::vector<uint32_t> h_code;
  std::vector<uint32_t> early;  // per proof of the chunk: status of the host checks
};

namespace qv {
uint32_t public_input_count(const qp_verifier *v) { return v && v->usable ? v->c.num_public_inputs : 0; }
const uint8_t *public_inputs(const qp_verifier *v, const uint8_t *proof) { return proof + v->d.fixed_len; }
}  // namespace qv

namespace {

std::string check_supported(const InnerCommon &c, Dims &d) {
  if (c.num_wires == 0 || c.num_wires > 4096 || c.num_routed_wires == 0 || c.num_routed_wires > c.num_wires)
    return "unsupported wire counts";
  if (c.num_constants > 4096 || c.groups.empty() || c.groups.size() > c.num_constants) return "bad selector groups";
  if (c.quotient_degree_factor == 0 || c.quotient_degree_factor > 64) return "bad quotient degree factor";
  const uint32_t nchunks = (c.num_routed_wires + c.quotient_degree_factor - 1) / c.quotient_degree_factor;
  if (c.num_partial_products != nchunks - 1) return "partial product count differs from the routed wires' chunks";
  if (c.num_query_rounds == 0 || c.num_query_rounds > 64) return "unsupported query round count";
  if (c.rate_bits == 0 || c.rate_bits > 8 || c.degree_bits == 0 || c.degree_bits + c.rate_bits > 30 || c.pow_bits > 64)
    return "unsupported FRI shape";
  if (c.arity_bits.size() > qv::MAX_LAYERS) return "too many FRI layers";
  if (c.num_public_inputs > (1u << 20) || c.num_gate_constraints > (1u << 16)) return "unsupported circuit size";
  d.log_n = c.degree_bits;
  d.log_N = c.degree_bits + c.rate_bits;
  d.cap_h = c.cap_height;
  if (d.cap_h > 16 || d.cap_h > d.log_N) return "cap height exceeds the tree";
  d.capw = 4u << d.cap_h;
  d.nq = c.num_query_rounds;
  d.nc = c.num_challenges;
  d.salt = c.hiding ? 4 : 0;
  d.nlayers = (uint32_t)c.arity_bits.size();
  d.init_sibs = d.log_N - d.cap_h;
  for (int o = 0; o < 4; o++) {
    d.unsalted[o] = c.width(o);
    d.width[o] = d.unsalted[o] + (o ? d.salt : 0);
    d.cls_width[o] = d.width[o];
    d.cls_sibs[o] = d.init_sibs;
    d.cls_shift[o] = 0;
  }
  uint32_t lg = d.log_N, tot = 0;
  for (uint32_t l = 0; l < d.nlayers; l++) {
    const uint32_t ab = c.arity_bits[l];
    if (ab == 0 || ab > 6 || tot + ab > d.log_n || lg - ab < d.cap_h) return "unsupported FRI reduction";
    lg -= ab;
    tot += ab;
    d.arity_bits[l] = ab;
    d.cls_width[4 + l] = 2u << ab;
    d.cls_sibs[4 + l] = lg - d.cap_h;
    d.cls_shift[4 + l] = tot;
  }
  d.ncls = 4 + d.nlayers;
  d.final_len = 1u << (d.log_n - tot);
  d.nopen = d.unsalted[0] + d.unsalted[1] + d.unsalted[2] + d.unsalted[3] + d.nc;
  d.pp_stride = qv::PP_BETAS + 2 * d.nlayers + 2 * d.final_len + d.nq;
  size_t s = (size_t)3 * d.capw * 8 + (size_t)d.nopen * 16 + (size_t)d.nlayers * d.capw * 8;
  size_t q = 0;
  for (uint32_t k = 0; k < d.ncls; k++) q += (size_t)d.cls_width[k] * 8 + 1 + (size_t)d.cls_sibs[k] * 32;
  s += q * d.nq + (size_t)d.final_len * 16 + 8 + 8;
  d.fixed_len = s;
  // the gates' reads stay inside the openings
  const uint32_t nsel = (uint32_t)c.groups.size();
  for (size_t gi = 0; gi < c.gates.size(); gi++) {
    // a parameter is a raw u64 of the common data: bound it before gate_shape multiplies it
    for (uint64_t prm : c.gates[gi].p)
      if (prm > c.num_wires)
        return "gate " + std::to_string(gi) + " (id " + std::to_string(c.gates[gi].id) + "): parameter exceeds the wire count";
    // (zero Reducing coefficients pass here, as upstream's from_bytes takes them)
    const qg::GateShape sh = qg::gate_shape(c.gates[gi].kind, c.gates[gi].p[0], c.gates[gi].p[1], c.gates[gi].p[2]);
    if (!sh.ok || sh.wires > c.num_wires || sh.consts > c.num_constants - nsel ||
        sh.constraints > c.num_gate_constraints)
      return "gate " + std::to_string(gi) + " (id " + std::to_string(c.gates[gi].id) + ") exceeds the circuit's wires, constants or constraints";
    if (c.selector_indices[gi] >= nsel) return "selector index out of range";
  }
  return "";
}

struct Proof {
  std::vector<uint64_t> caps;  // wires, zs, quotient caps, then the layers'
  std::vector<ext> open;       // constants||sigmas, wires, zs, zs_next, pp, quotient
  std::vector<ext> final_poly;
  uint64_t pow_witness = 0;
  std::vector<uint64_t> pis;
};

// canonical-element copy out of the byte stream
bool take(const uint8_t *&p, uint64_t *dst, size_t n) {
  memcpy(dst, p, n * 8);
  p += n * 8;
  bool ok = true;
  for (size_t i = 0; i < n; i++) ok = ok && dst[i] < gl::P;
  return ok;
}

// the per-proof host work; fills slot `s` of the chunk's arrays.  Returns the
// verdict of checks 1-4 / malformed, 0 if the query rounds decide.
uint32_t host_part(const qp_verifier *V, const uint8_t *pb, size_t len, uint64_t *buf, const Layout &L, uint32_t s) {
  const InnerCommon &c = V->c;
  const Dims &d = V->d;
  if (!pb || len < d.fixed_len) return QP_VERIFY_MALFORMED;
  uint64_t npis;
  memcpy(&npis, pb + d.fixed_len - 8, 8);
  if (npis > (1u << 20) || len != d.fixed_len + npis * 8) return QP_VERIFY_MALFORMED;
  Proof P;
  const uint8_t *p = pb;
  bool ok = true;
  P.caps.resize((size_t)(3 + d.nlayers) * d.capw);
  ok = take(p, P.caps.data(), (size_t)3 * d.capw) && ok;
  P.open.resize(d.nopen);
  ok = take(p, (uint64_t *)P.open.data(), (size_t)d.nopen * 2) && ok;
  ok = take(p, P.caps.data() + (size_t)3 * d.capw, (size_t)d.nlayers * d.capw) && ok;
  for (uint32_t q = 0; q < d.nq; q++) {
    const size_t lane = (size_t)s * d.nq + q;
    for (uint32_t k = 0; k < d.ncls; k++) {
      ok = take(p, buf + L.leaves[k] + lane * d.cls_width[k], d.cls_width[k]) && ok;
      ok = (*p++ == d.cls_sibs[k]) && ok;
      ok = take(p, buf + L.sibs[k] + lane * d.cls_sibs[k] * 4, (size_t)d.cls_sibs[k] * 4) && ok;
    }
  }
  P.final_poly.resize(d.final_len);
  ok = take(p, (uint64_t *)P.final_poly.data(), (size_t)d.final_len * 2) && ok;
  ok = take(p, &P.pow_witness, 1) && ok;
  p += 8;
  P.pis.resize(npis);
  ok = take(p, P.pis.data(), npis) && ok;
  if (!ok) return QP_VERIFY_MALFORMED;
  if (npis != c.num_public_inputs) return QP_VERIFY_PUBLIC_INPUT_COUNT;

  const uint32_t nc = d.nc, R = c.num_routed_wires, qdf = c.quotient_degree_factor, npp = c.num_partial_products;
  const ext *cs = P.open.data(), *wires = cs + d.unsalted[0], *zs = wires + d.unsalted[1], *zs_next = zs + nc;
  const ext *pp = zs_next + nc, *quot = pp + (size_t)nc * npp;
  const uint64_t *wires_cap = P.caps.data(), *zs_cap = wires_cap + d.capw, *quot_cap = zs_cap + d.capw;
  const uint64_t *commit_caps = quot_cap + d.capw;

  // ---- get_challenges
  uint64_t pih[4];
  qh::hash_no_pad(P.pis.data(), P.pis.size(), pih);
  qh::Challenger ch;
  ch.observe(V->digest, 4);
  ch.observe(pih, 4);
  ch.observe(wires_cap, d.capw);
  F betas[2], gammas[2], alphas[2];
  for (uint32_t i = 0; i < nc; i++) betas[i] = ch.get();
  for (uint32_t i = 0; i < nc; i++) gammas[i] = ch.get();
  ch.observe(zs_cap, d.capw);
  for (uint32_t i = 0; i < nc; i++) alphas[i] = ch.get();
  ch.observe(quot_cap, d.capw);
  const ext zeta = ch.get_ext();
  // the zeta batch in FriOpenings order (constants, sigmas, wires, zs, pp, quotient), then the g zeta batch
  std::vector<ext> zbatch;
  zbatch.reserve(d.nopen);
  zbatch.insert(zbatch.end(), cs, zs + nc);
  zbatch.insert(zbatch.end(), pp, quot + d.unsalted[3]);
  for (const ext &e : zbatch) ch.observe(&e.c0, 2);
  for (uint32_t i = 0; i < nc; i++) ch.observe(&zs_next[i].c0, 2);
  const ext fri_alpha = ch.get_ext();
  ext fri_betas[qv::MAX_LAYERS];
  for (uint32_t l = 0; l < d.nlayers; l++) {
    ch.observe(commit_caps + (size_t)l * d.capw, d.capw);
    fri_betas[l] = ch.get_ext();
  }
  for (const ext &e : P.final_poly) ch.observe(&e.c0, 2);
  ch.observe(P.pow_witness);
  const uint64_t pow_response = ch.get();
  uint64_t qidx[64];
  for (uint32_t q = 0; q < d.nq; q++) qidx[q] = ch.get() & ((1ull << d.log_N) - 1);

  // ---- zeta^n != 1
  ext zeta_n = zeta;
  for (uint32_t i = 0; i < d.log_n; i++) zeta_n = gl::ext_mul(zeta_n, zeta_n);
  if (gl::ext_eq(zeta_n, ext{1, 0})) return QP_VERIFY_ZETA_IN_SUBGROUP;

  // ---- eval_vanishing_poly at zeta
  VG g;
  std::vector<ext> terms;
  const ext zh = gl::ext_sub(zeta_n, ext{1, 0});
  const ext l0 = gl::ext_mul(zh, gl::ext_inv(gl::ext_scale(gl::ext_sub(zeta, ext{1, 0}), (F)1 << d.log_n)));
  for (uint32_t i = 0; i < nc; i++) terms.push_back(gl::ext_mul(l0, gl::ext_sub(zs[i], ext{1, 0})));
  const ext *sig = cs + c.num_constants;
  for (uint32_t i = 0; i < nc; i++) {
    const ext *partials = pp + (size_t)i * npp;
    const uint32_t nchunks = npp + 1;
    for (uint32_t k = 0; k < nchunks; k++) {
      ext num{1, 0}, den{1, 0};
      for (uint32_t j = k * qdf; j < (k + 1) * qdf && j < R; j++) {
        const ext wg = g.add_const(wires[j], gammas[i]);
        num = gl::ext_mul(num, gl::ext_add(wg, gl::ext_scale(zeta, gl::mul(betas[i], c.k_is[j]))));
        den = gl::ext_mul(den, gl::ext_add(wg, gl::ext_scale(sig[j], betas[i])));
      }
      const ext prev = k == 0 ? zs[i] : partials[k - 1];
      const ext next = k == nchunks - 1 ? zs_next[i] : partials[k];
      terms.push_back(gl::ext_sub(gl::ext_mul(prev, num), gl::ext_mul(next, den)));
    }
  }
  {
    // evaluate_gate_constraints: per gate its selector filter times each constraint
    const uint32_t nsel = (uint32_t)c.groups.size();
    std::vector<ext> gate_terms(c.num_gate_constraints, ext{0, 0});
    const std::vector<ext> wv(wires, wires + d.unsalted[1]);
    const std::vector<F> pi_hash(pih, pih + 4);
    for (size_t gi = 0; gi < c.gates.size(); gi++) {
      const uint32_t si = c.selector_indices[gi];
      const auto grp = c.groups[si];
      const ext sel = cs[si];
      ext filter{1, 0};
      for (uint32_t j = grp.first; j < grp.second; j++)
        if (j != gi) filter = gl::ext_mul(filter, gl::ext_sub(ext{j, 0}, sel));
      if (nsel > 1) filter = gl::ext_mul(filter, gl::ext_sub(ext{UNUSED_SELECTOR, 0}, sel));
      const std::vector<ext> k = qr::gate_constraints(g, c.gates[gi], wv, cs + nsel, pi_hash);
      for (size_t t = 0; t < k.size() && t < gate_terms.size(); t++)
        gate_terms[t] = gl::ext_add(gate_terms[t], gl::ext_mul(filter, k[t]));
    }
    terms.insert(terms.end(), gate_terms.begin(), gate_terms.end());
  }
  for (uint32_t i = 0; i < nc; i++) {
    const ext van = g.reduce(ext{alphas[i], 0}, terms);
    ext t{0, 0};
    for (uint32_t k = qdf; k-- > 0;) t = gl::ext_add(gl::ext_mul(t, zeta_n), quot[(size_t)i * qdf + k]);
    if (!gl::ext_eq(van, gl::ext_mul(zh, t))) return QP_VERIFY_VANISHING_IDENTITY;
  }

  // ---- fri_verify_proof_of_work
  const int lz = pow_response ? __builtin_clzll(pow_response) : 64;
  if (lz < (int)c.pow_bits) return QP_VERIFY_POW;

  // ---- the query rounds' inputs: PrecomputedReducedOpenings, challenges, indices, caps
  uint64_t *blk = buf + L.pp + (size_t)s * d.pp_stride;
  auto put = [&](uint32_t at, ext e) {
    blk[at] = e.c0;
    blk[at + 1] = e.c1;
  };
  put(qv::PP_ZETA, zeta);
  put(qv::PP_ZETA_NEXT, gl::ext_scale(zeta, gl::root_of_unity(d.log_n)));
  put(qv::PP_ALPHA, fri_alpha);
  put(qv::PP_ALPHA_NC, gl::ext_pow(fri_alpha, nc));
  put(qv::PP_RED0, g.reduce(fri_alpha, zbatch));
  put(qv::PP_RED1, g.reduce(fri_alpha, std::vector<ext>(zs_next, zs_next + nc)));
  for (uint32_t l = 0; l < d.nlayers; l++) put(qv::PP_BETAS + 2 * l, fri_betas[l]);
  uint64_t *fp = blk + qv::PP_BETAS + 2 * d.nlayers;
  memcpy(fp, P.final_poly.data(), (size_t)d.final_len * 16);
  for (uint32_t q = 0; q < d.nq; q++) fp[2 * d.final_len + q] = qidx[q];
  for (uint32_t k = 0; k < d.ncls; k++) {
    uint32_t *idx = (uint32_t *)(buf + L.idx[k]) + (size_t)s * d.nq;
    for (uint32_t q = 0; q < d.nq; q++) idx[q] = (uint32_t)(qidx[q] >> d.cls_shift[k]);
    if (k) memcpy(buf + L.caps[k] + (size_t)s * d.capw, P.caps.data() + (size_t)(k - 1) * d.capw, (size_t)d.capw * 8);
  }
  return QP_VERIFY_OK;
}

// a slot whose proof the host checks already decided: well-formed zeros (the
// lanes run, their results are not read)
void clear_slot(const Dims &d, uint64_t *buf, const Layout &L, uint32_t s) {
  for (uint32_t k = 0; k < d.ncls; k++) {
    const size_t lane = (size_t)s * d.nq;
    memset(buf + L.leaves[k] + lane * d.cls_width[k], 0, (size_t)d.nq * d.cls_width[k] * 8);
    memset(buf + L.sibs[k] + lane * d.cls_sibs[k] * 4, 0, (size_t)d.nq * d.cls_sibs[k] * 32);
    memset((uint32_t *)(buf + L.idx[k]) + lane, 0, (size_t)d.nq * 4);
    if (k) memset(buf + L.caps[k] + (size_t)s * d.capw, 0, (size_t)d.capw * 8);
  }
  memset(buf + L.pp + (size_t)s * d.pp_stride, 0, (size_t)d.pp_stride * 8);
}

void make_jobs(const qp_verifier *V, const Layout &L, uint32_t nb, const uint64_t *base, uint8_t *ok, uint32_t *code,
               qv::PathJob &pj, qv::FriJob &fj) {
  const Dims &d = V->d;
  const uint32_t lanes = nb * d.nq;
  pj = qv::PathJob{};
  fj = qv::FriJob{};
  for (uint32_t k = 0; k < d.ncls; k++)
    pj.cls[k] = qv::PathClass{base + L.leaves[k], base + L.sibs[k], (const uint32_t *)(base + L.idx[k]),
                              base + L.caps[k], k ? d.capw : 0, d.cls_width[k], d.cls_sibs[k], d.nq, lanes};
  pj.ncls = d.ncls;
  pj.cap_height = d.cap_h;
  pj.total = lanes * d.ncls;
  pj.ok = ok;
  for (int o = 0; o < 4; o++) {
    fj.leaves[o] = base + L.leaves[o];
    fj.width[o] = d.width[o];
    fj.unsalted[o] = d.unsalted[o];
  }
  for (uint32_t l = 0; l < d.nlayers; l++) {
    fj.evals[l] = base + L.leaves[4 + l];
    fj.arity_bits[l] = d.arity_bits[l];
  }
  fj.nlayers = d.nlayers;
  fj.nq = d.nq;
  fj.log_N = d.log_N;
  fj.nc = d.nc;
  fj.final_len = d.final_len;
  fj.n = lanes;
  fj.pp = base + L.pp;
  fj.pp_stride = d.pp_stride;
  fj.code = code;
}

// plonky2's sequential order over the per-lane results
uint32_t reduce_proof(const Dims &d, uint32_t nb, uint32_t s, const uint8_t *ok, const uint32_t *code) {
  const uint32_t lanes = nb * d.nq;
  for (uint32_t q = 0; q < d.nq; q++) {
    const uint32_t lane = s * d.nq + q;
    for (uint32_t o = 0; o < 4; o++)
      if (!ok[o * lanes + lane]) return QP_VERIFY_INITIAL_MERKLE_PATH;
    const uint32_t cd = code[lane];
    const uint32_t bad_layer = (cd & 0xff) == 6 ? cd >> 8 : d.nlayers;  // first layer whose consistency check fails
    for (uint32_t l = 0; l < d.nlayers; l++) {
      if (l == bad_layer) return QP_VERIFY_FRI_CONSISTENCY;
      if (!ok[(4 + l) * lanes + lane]) return QP_VERIFY_FRI_MERKLE_PATH;
    }
    if (cd) return QP_VERIFY_FINAL_POLY;
  }
  return QP_VERIFY_OK;
}

int verify_chunk(qp_verifier *V, const uint8_t *const *proofs, const size_t *lens, uint32_t nb, uint32_t *status) {
  const Dims &d = V->d;
  const Layout L = make_layout(d, nb);
  uint64_t *buf = V->h_buf;
  memcpy(buf + L.caps[0], V->cap.data(), (size_t)d.capw * 8);
  V->early.assign(nb, 0);
  V->pool->parallel_for(nb, [&](size_t i) {
    uint32_t st = QP_VERIFY_MALFORMED;
    try {
      st = host_part(V, proofs[i], lens[i], buf, L, (uint32_t)i);
    } catch (const std::exception &) {
      st = ~0u;  // allocation failure: reported as the call's error below
    }
    if (st) clear_slot(d, buf, L, (uint32_t)i);
    V->early[i] = st;
  });
  for (uint32_t i = 0; i < nb; i++)
    if (V->early[i] == ~0u) {
      V->err = "out of host memory";
      return QP_ERR_OOM;
    }
  const uint32_t lanes = nb * d.nq;
  qv::PathJob pj;
  qv::FriJob fj;
  if (V->ctx) {
    qp_ctx *c = V->ctx;
    QP_HIP_TRY(V, hipSetDevice(c->device));
    QP_HIP_TRY(V, hipMemcpyAsync(V->d_buf, buf, L.words * 8, hipMemcpyHostToDevice, c->stream));
    make_jobs(V, L, nb, V->d_buf, V->d_ok, V->d_code, pj, fj);
    qv::launch_paths(pj, c->stream);
    QP_HIP_TRY(V, hipGetLastError());
    qv::launch_fri(fj, c->stream);
    QP_HIP_TRY(V, hipGetLastError());
    QP_HIP_TRY(V, hipMemcpyAsync(V->h_ok.data(), V->d_ok, (size_t)lanes * d.ncls, hipMemcpyDeviceToHost, c->stream));
    QP_HIP_TRY(V, hipMemcpyAsync(V->h_code.data(), V->d_code, (size_t)lanes * 4, hipMemcpyDeviceToHost, c->stream));
    QP_HIP_TRY(V, hipStreamSynchronize(c->stream));
  } else {
    make_jobs(V, L, nb, buf, V->h_ok.data(), V->h_code.data(), pj, fj);
    // one task per (proof, tree) and one per proof's arithmetic
    V->pool->parallel_for((size_t)nb * (d.ncls + 1), [&](size_t t) {
      const uint32_t s = (uint32_t)(t / (d.ncls + 1)), k = (uint32_t)(t % (d.ncls + 1));
      if (V->early[s]) return;
      if (k < d.ncls) qv::host_paths(pj, k, s * d.nq, (s + 1) * d.nq, k * lanes);
      else qv::host_fri(fj, s * d.nq, (s + 1) * d.nq);
    });
  }
  for (uint32_t i = 0; i < nb; i++)
    status[i] = V->early[i] ? V->early[i] : reduce_proof(d, nb, i, V->h_ok.data(), V->h_code.data());
  return QP_OK;
}

void release(qp_verifier *V) {
  if (V->ctx) {
    (void)hipSetDevice(V->ctx->device);
    if (V->h_buf) (void)hipHostFree(V->h_buf);
    if (V->d_buf) (void)hipFree(V->d_buf);
    if (V->d_ok) (void)hipFree(V->d_ok);
    if (V->d_code) (void)hipFree(V->d_code);
  } else {
    delete[] V->h_buf;
  }
  V->h_buf = V->d_buf = nullptr;
  V->d_ok = nullptr;
  V->d_code = nullptr;
}

}  // namespace

extern "C" {

int qp_verifier_new(qp_ctx *ctx, const uint8_t *verifier_only, size_t vlen, const uint8_t *common, size_t clen,
                    uint32_t max_batch, qp_verifier **out) {
  if (!out) return QP_ERR_ARG;
  *out = nullptr;
  if (!verifier_only || !common || !max_batch || max_batch > (1u << 16)) return QP_ERR_ARG;
  qp_verifier *V = new (std::nothrow) qp_verifier();
  if (!V) return QP_ERR_OOM;
  *out = V;  // a handle that is not usable still carries the reason
  try {
    V->ctx = ctx;
    V->max_batch = max_batch;
    V->err = qr::parse_common(common, clen, V->c);
    if (V->err.empty()) V->err = check_supported(V->c, V->d);
    if (!V->err.empty()) {
      V->err = "common circuit data: " + V->err;
      return QP_ERR_FORMAT;
    }
    const Dims &d = V->d;
    uint64_t h = 0;
    if (vlen >= 8) memcpy(&h, verifier_only, 8);
    if (vlen < 8 || h != d.cap_h) {
      V->err = "verifier data: cap height differs from the common data's";
      return QP_ERR_FORMAT;
    }
    if (vlen != 8 + (size_t)d.capw * 8 + 32) {
      V->err = "verifier data: " + std::to_string(vlen) + " bytes, expected " + std::to_string(8 + (size_t)d.capw * 8 + 32);
      return QP_ERR_FORMAT;
    }
    V->cap.resize(d.capw);
    const uint8_t *p = verifier_only + 8;
    bool ok = take(p, V->cap.data(), d.capw);
    ok = take(p, V->digest, 4) && ok;
    if (!ok) {
      V->err = "verifier data: non-canonical field element";
      return QP_ERR_FORMAT;
    }
    const Layout L = make_layout(d, max_batch);
    const size_t lanes = (size_t)max_batch * d.nq;
    if (lanes * d.ncls > (1u << 30)) {
      V->err = "max_batch too large for this circuit";
      return QP_ERR_ARG;
    }
    V->h_ok.assign(lanes * d.ncls, 0);
    V->h_code.assign(lanes, 0);
    if (ctx) {
      QP_HIP_TRY(V, hipSetDevice(ctx->device));
      QP_HIP_TRY(V, hipHostMalloc((void **)&V->h_buf, L.words * 8, hipHostMallocDefault));
      QP_HIP_TRY(V, hipMalloc(&V->d_buf, L.words * 8));
      QP_HIP_TRY(V, hipMalloc(&V->d_ok, lanes * d.ncls));
      QP_HIP_TRY(V, hipMalloc(&V->d_code, lanes * 4));
    } else {
      V->h_buf = new uint64_t[L.words];
    }
    const unsigned hw = std::thread::hardware_concurrency();
    const unsigned nthreads = std::min<unsigned>(hw ? hw : 4, 16);
    V->pool.reset(new qh::ThreadPool(nthreads > 1 ? nthreads - 1 : 0));
    V->usable = true;
    return QP_OK;
  } catch (const std::bad_alloc &) {
    V->err = "out of host memory";
    return QP_ERR_OOM;
  } catch (const std::exception &e) {
    V->err = e.what();
    return QP_ERR_STATE;
  }
}

void qp_verifier_free(qp_verifier *V) {
  if (!V) return;
  if (V->ctx && V->usable) (void)hipStreamSynchronize(V->ctx->stream);
  release(V);
  delete V;
}

const char *qp_verifier_last_error(const qp_verifier *V) { return V ? V->err.c_str() : "null verifier"; }

int qp_verifier_verify(qp_verifier *V, const uint8_t *const *proofs, const size_t *lens, uint32_t n,
                       uint32_t *status_out) {
  if (!V) return QP_ERR_ARG;
  if (!V->usable) return QP_ERR_STATE;
  if (!n) return QP_OK;
  if (!proofs || !lens || !status_out) {
    V->err = "null argument";
    return QP_ERR_ARG;
  }
  try {
    for (uint32_t at = 0; at < n; at += V->max_batch) {
      const uint32_t nb = std::min(V->max_batch, n - at);
      const int rc = verify_chunk(V, proofs + at, lens + at, nb, status_out + at);
      if (rc) return rc;
    }
  } catch (const std::bad_alloc &) {
    V->err = "out of host memory";
    return QP_ERR_OOM;
  }
  return QP_OK;
}

int qp_verifier_set_host_threads(qp_verifier *V, uint32_t nthreads) {
  if (!V || !V->usable || nthreads == 0 || nthreads > 256) return QP_ERR_ARG;
  V->pool.reset(new qh::ThreadPool(nthreads - 1));
  return QP_OK;
}

}  // extern "C"
