// seams.cpp — routine-level entry points of the C ABI: the
// pieces of plonky2's prove() a patched qp-plonky2 routes to the GPU for ANY
// circuit over the supported gate set, not only the built-in ones (the
// aggregator's CircuitData::prove, wormhole/aggregator/src/circuits/tree.rs:136):
//   qp_quotient          plonk/prover.rs compute_quotient_polys (leaf gates: the
//                        single-read kernel; any gate list: the generic one)
//   qp_fri_layer_commit  fri/prover.rs fri_committed_trees, one reduction layer
//   qp_fri_fold          the same loop's coefficient fold with beta
//   qp_pow_grind         fri/prover.rs fri_proof_of_work (minimal witness)
//   qp_partial_products_and_zs  plonk/prover.rs wires_permutation_partial_products_and_zs
//   qp_opening_set / qp_batch_eval_ext  plonk/proof.rs OpeningSet::new
//   qp_fri_initial_poly  fri/oracle.rs PolynomialBatch::prove_openings, the polynomial FRI starts from
// The transcript stays with the caller: each seam consumes the challenges the
// caller's Challenger drew and returns what it must observe next.
#include <stdlib.h>
#include <string.h>
#include <string>
#include <algorithm>
#include <new>
#include <vector>
#include "../../include/qpgpu.h"
#include "circuit_obj.h"
#include "ctx.h"
#include "field.h"
#include "kernels.h"
#include "prover_kernels.h"
#include "paths.h"

namespace {

// degrees of the circuit-level seams (qp_quotient's): k_fri_divide runs n / 8
// threads and holds at most 64 values per thread, k_z_scan has its two forms
constexpr uint32_t SEAM_LOG_MIN = 6, SEAM_LOG_MAX = qpk::BIG_LOG_MAX - 1;
constexpr uint32_t PP_MAX_CHUNKS = 16;  // k_pp_rows' per-row chunk arrays

// the shared preconditions of qp_opening_set and qp_fri_initial_poly: four
// batches (constants||sigmas, wires, Zs||partial products, quotient) of ctx,
// of one proof, unsalted, holding coefficients of one degree 2^6..2^15; 1 or 2
// challenges with their Zs present; zeta invertible and outside H.  Fills the
// opening words of the one-proof challenge block ch
int check_circuit_batches(qp_ctx *ctx, const char *fn, const qp_batch *const bt[4], uint32_t nc,
                          const uint64_t *zeta, const void *out, uint64_t *ch) {
  auto fail = [&](const char *why) {
    ctx->err = std::string(fn) + ": " + why;
    return (int)QP_ERR_ARG;
  };
  if (!bt[0] || !bt[1] || !bt[2] || !bt[3] || !zeta || !out) return fail("null argument");
  const uint32_t log_n = bt[0]->log_n;
  for (int i = 0; i < 4; i++) {
    if (bt[i]->ctx != ctx) return fail("a batch belongs to another context");
    if (bt[i]->log_n != log_n) return fail("the batches differ in log_n");
    if (bt[i]->nbat != 1 || bt[i]->nsalt) return fail("needs unsalted batches of one proof");
    if (!bt[i]->d_coeffs || !bt[i]->npolys) return fail("a batch holds no coefficients");
  }
  if (log_n < SEAM_LOG_MIN || log_n > SEAM_LOG_MAX) return fail("unsupported degree (2^6 <= n <= 2^15)");
  if (nc < 1 || nc > 2) return fail("num_challenges must be 1 or 2");
  if (bt[2]->npolys < nc) return fail("zs_pp holds fewer polynomials than challenges");
  const gl::ext z{gl::canon(zeta[0]), gl::canon(zeta[1])};
  if (!(z.c0 | z.c1)) return fail("zeta = 0");
  const gl::ext zn_pow = gl::ext_pow(z, 1ull << log_n);
  if (zn_pow.c0 == 1 && zn_pow.c1 == 0) return fail("zeta^n = 1 (an opening point inside the subgroup)");
  qpk::open_point_words(ch, z, log_n);
  return QP_OK;
}

}  // namespace

struct qp_perm {
  qp_ctx *ctx = nullptr;
  uint32_t R = 0, log_n = 0;
  DevBuf sigmas;  // [R][n] values over H
  DevBuf kis;     // [R]
};

struct qp_fri_layer {
  qp_ctx *ctx = nullptr;
  uint32_t log_values = 0, arity_bits = 0, cap_h = 0;
  DevBuf vals;  // [2][2^log_values] leaf order (c0 row, c1 row)
  DevBuf dig;   // tree digests over 2^(log_values - arity_bits) leaves
};

extern "C" {

int qp_circuit_gate_desc(const qp_circuit *c, qp_gate_desc *g) {
  if (!c || !g) return QP_ERR_ARG;
  const qc::CircuitData &cd = c->cd;
  memset(g, 0, sizeof(*g));
  if (cd.gate_kinds.size() > QP_MAX_GATES || cd.groups.size() > QP_MAX_GATES) return QP_ERR_ARG;
  g->num_gates = (uint32_t)cd.gate_kinds.size();
  for (uint32_t i = 0; i < g->num_gates; i++) {
    g->kind[i] = cd.gate_kinds[i];
    g->param[i] = cd.gate_params[i];
    g->param2[i] = i < cd.gate_params2.size() ? cd.gate_params2[i] : 0;
    g->param3[i] = i < cd.gate_params3.size() ? cd.gate_params3[i] : 0;
    g->selector_index[i] = cd.selector_indices[i];
  }
  g->num_selectors = (uint32_t)cd.groups.size();
  for (uint32_t s = 0; s < g->num_selectors; s++) {
    g->group_lo[s] = cd.groups[s].first;
    g->group_hi[s] = cd.groups[s].second;
  }
  g->num_constants = cd.num_constants;
  g->num_routed_wires = cd.config.num_routed_wires;
  g->num_wires = cd.config.num_wires;
  g->quotient_degree_factor = cd.quotient_degree_factor;
  g->num_challenges = cd.config.num_challenges;
  g->num_gate_constraints = cd.num_gate_constraints;
  return QP_OK;
}

int qp_quotient(qp_ctx *ctx, const qp_batch *cs, const qp_batch *wires, const qp_batch *zs_pp, const qp_gate_desc *g,
                const uint64_t *betas, const uint64_t *gammas, const uint64_t *alphas, const uint64_t pi_hash[4],
                uint64_t *quotient_coeffs_out) {
  if (!ctx || !cs || !wires || !zs_pp || !g || !betas || !gammas || !alphas || !pi_hash || !quotient_coeffs_out)
    return QP_ERR_ARG;
  const uint32_t log_n = cs->log_n, rb = cs->rate_bits, logN = log_n + rb;
  const uint32_t R = g->num_routed_wires, qdf = g->quotient_degree_factor, nc = g->num_challenges;
  const uint32_t nchunks = qdf ? (R + qdf - 1) / qdf : 0;
  const uint32_t nterms = nc + nc * nchunks + g->num_gate_constraints;
  if (nc != 2 || g->num_gates == 0 || g->num_gates > QP_MAX_GATES || g->num_selectors == 0 ||
      g->num_selectors > QP_MAX_GATES || qdf != (1u << rb) || logN > qpk::TW_LOG || log_n < 6 ||
      log_n > qpk::BIG_LOG_MAX - 1 ||
      nterms > qpk::APOW_STRIDE || wires->log_n != log_n || zs_pp->log_n != log_n || wires->rate_bits != rb ||
      zs_pp->rate_bits != rb || cs->nbat != 1 || wires->nbat != 1 || zs_pp->nbat != 1 ||
      cs->npolys != g->num_constants + R || wires->npolys != g->num_wires || zs_pp->npolys != nc * nchunks ||
      wires->nsalt || zs_pp->nsalt || cs->nsalt || R > g->num_wires || rb > 4 ||
      g->num_constants < g->num_selectors) {
    ctx->err = "qp_quotient: unsupported shape (2 challenges, qdf = 2^rate_bits <= 16, 2^6 <= n <= 2^15, unsalted batches of one)";
    return QP_ERR_ARG;
  }
  // per-gate checks: known kind, selector in range, parameters inside the
  // kernels' bounds, every wire a gate reads < num_wires, every gate constant
  // < num_constants - num_selectors, constraint count <= num_gate_constraints
  const uint32_t W = g->num_wires, n_gc = g->num_constants - g->num_selectors;
  for (uint32_t s = 0; s < g->num_selectors; s++)
    if (g->group_lo[s] > g->group_hi[s] || g->group_hi[s] > g->num_gates) {
      ctx->err = "qp_quotient: selector group " + std::to_string(s) + " out of range";
      return QP_ERR_ARG;
    }
  for (uint32_t i = 0; i < g->num_gates; i++) {
    const uint32_t k = g->kind[i];
    const qg::GateShape sh = qg::gate_shape(k, g->param[i], g->param2[i], g->param3[i]);
    // plonky2 places each gate in the selector group it belongs to
    const bool placed = g->selector_index[i] < g->num_selectors && g->group_lo[g->selector_index[i]] <= i &&
                        i < g->group_hi[g->selector_index[i]];
    // the kernels' Reducing gates take the last accumulator from wires 0..1: at least one coefficient
    const bool no_coeffs = (k == qg::G_REDUCING || k == qg::G_REDUCING_EXT) && g->param[i] < 1;
    if (!placed || !sh.ok || no_coeffs || sh.wires > W || sh.consts > n_gc ||
        sh.constraints > g->num_gate_constraints) {
      ctx->err = "qp_quotient: gate " + std::to_string(i) + ": unknown gate kind, selector or parameters";
      return QP_ERR_ARG;
    }
  }
  const uint64_t n = 1ull << log_n, N = 1ull << logN;
  QP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  try {
    std::vector<uint64_t> tab = qpk::quotient_point_tables(log_n, rb);
    std::vector<uint64_t> chal(qpk::CHAL_STRIDE, 0), apow(2 * qpk::APOW_STRIDE, 0);
    for (uint32_t c = 0; c < 2; c++) {
      chal[qpk::CH_BETA + c] = gl::canon(betas[c]);
      chal[qpk::CH_GAMMA + c] = gl::canon(gammas[c]);
      qpk::alpha_powers(apow.data() + c * qpk::APOW_STRIDE, gl::canon(alphas[c]), nterms);
    }
    qpk::perm_challenges(chal.data(), chal.data() + qpk::CH_BETA, chal.data() + qpk::CH_GAMMA, 2, R, qdf);
    for (int i = 0; i < 4; i++) chal[qpk::CH_PIH + i] = gl::canon(pi_hash[i]);
    DevBuf d_tab, d_chal, d_apow, d_q, d_cbuf, d_out;
    QP_HIP_TRY(ctx, d_tab.alloc(tab.size()));
    QP_HIP_TRY(ctx, d_chal.alloc(chal.size()));
    QP_HIP_TRY(ctx, d_apow.alloc(apow.size()));
    QP_HIP_TRY(ctx, d_q.alloc(2 * N));
    QP_HIP_TRY(ctx, d_cbuf.alloc(2 * N));
    QP_HIP_TRY(ctx, d_out.alloc((uint64_t)nc * qdf * n));
    QP_HIP_TRY(ctx, hipMemcpyAsync(d_tab.p, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, s));
    QP_HIP_TRY(ctx, hipMemcpyAsync(d_chal.p, chal.data(), chal.size() * 8, hipMemcpyHostToDevice, s));
    QP_HIP_TRY(ctx, hipMemcpyAsync(d_apow.p, apow.data(), apow.size() * 8, hipMemcpyHostToDevice, s));
    qpk::QuotientArgs a;
    a.cs_lde = cs->d_lde;
    a.w_lde = wires->d_lde;
    a.z_lde = zs_pp->d_lde;
    a.w_bstride = a.z_bstride = 0;
    a.chal = d_chal.p;
    a.tw = ctx->tw.fwd;
    a.apow = d_apow.p;
    a.xtab = d_tab.p;
    a.l0tab = d_tab.p + N;
    qpk::quotient_zh(a, log_n, rb);
    a.q_out = d_q.p;
    a.q_bstride = 2 * N;
    a.log_n = log_n;
    a.rate_bits = rb;
    a.R = R;
    a.qdf = qdf;
    a.num_constants = g->num_constants;
    a.g = qpk::gate_desc_dev(*g);
    // the prover's kernels: the single-read one for the leaf gate set, else
    // the permutation terms and one launch per gate
    qpk::quotient_values(a, qpk::quotient_kernel(a.g, R), 1, s);
    qpk::quotient_coeffs(ctx->tw, d_q.p, d_cbuf.p, d_out.p, log_n, rb, nc, 1, 2 * N, 2 * N, (uint64_t)nc * qdf * n, s);
    QP_HIP_TRY(ctx, hipGetLastError());
    QP_HIP_TRY(ctx, hipMemcpyAsync(quotient_coeffs_out, d_out.p, (uint64_t)nc * qdf * n * 8, hipMemcpyDeviceToHost, s));
    QP_HIP_TRY(ctx, hipStreamSynchronize(s));
  } catch (const std::bad_alloc &) {
    return QP_ERR_OOM;
  }
  return QP_OK;
}

int qp_fri_layer_commit(qp_ctx *ctx, const uint64_t *coeffs, uint32_t log_coeffs, uint32_t log_values, uint64_t shift,
                        uint32_t arity_bits, uint32_t cap_height, uint64_t *cap_out, qp_fri_layer **out) {
  if (!ctx || !coeffs || !cap_out) return QP_ERR_ARG;
  if (out) *out = nullptr;
  if (log_values > qpk::TW_LOG || log_coeffs > log_values || log_coeffs < 1 || arity_bits < 1 || arity_bits > 4 ||
      log_values < arity_bits + cap_height) {
    ctx->err = "qp_fri_layer_commit: unsupported sizes";
    return QP_ERR_ARG;
  }
  // The reference keeps the folded coefficient vector at full length (zero
  // tail, fri/prover.rs fri_committed_trees); transform only the nonzero
  // prefix, rounded up to a power of two.
  uint64_t nz = 0;
  for (uint64_t i = 1ull << log_coeffs; i-- > 0;)
    if (gl::canon(coeffs[i]) | gl::canon(coeffs[(1ull << log_coeffs) + i])) {
      nz = i + 1;
      break;
    }
  uint32_t lc = 1;
  while ((1ull << lc) < nz) lc++;
  if (lc > qpk::BIG_LOG_MAX) {  // the coset LDE's sizes
    ctx->err = "qp_fri_layer_commit: more than 2^16 nonzero coefficients";
    return QP_ERR_ARG;
  }
  lc = std::min(lc, log_coeffs);
  const uint64_t Lin = 1ull << log_coeffs;
  QP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const uint64_t Lc = 1ull << lc, Lv = 1ull << log_values;
  const uint32_t log_leaves = log_values - arity_bits;
  qp_fri_layer *L = new (std::nothrow) qp_fri_layer();
  if (!L) return QP_ERR_OOM;
  L->ctx = ctx;
  L->log_values = log_values;
  L->arity_bits = arity_bits;
  L->cap_h = cap_height;
  DevBuf d_c;
  const uint64_t dbs = qpk::tree_digest_count(log_leaves, cap_height) * 4;
  hipError_t e = d_c.alloc(2 * Lc);
  if (!e) e = L->vals.alloc(2 * Lv);
  if (!e) e = L->dig.alloc(dbs);
  if (e) {
    delete L;
    ctx->err = std::string("qp_fri_layer_commit: ") + hipGetErrorString(e);
    return e == hipErrorOutOfMemory ? QP_ERR_OOM : QP_ERR_HIP;
  }
  e = hipMemcpy2DAsync(d_c.p, Lc * 8, coeffs, Lin * 8, Lc * 8, 2, hipMemcpyHostToDevice, s);
  if (!e) {
    // values = coset_fft(coeffs, shift), leaf (bit-reversed) order, and their tree
    qpk::fri_layer_tree(ctx->tw, d_c.p, Lc, 2 * Lc, lc, L->vals.p, L->dig.p, log_values, arity_bits, cap_height, shift,
                        1, s);
    e = hipGetLastError();
  }
  if (!e)
    e = hipMemcpyAsync(cap_out, L->dig.p + qpk::tree_level_offset(log_leaves, log_leaves - cap_height) * 4,
                       (size_t)32 << cap_height, hipMemcpyDeviceToHost, s);
  if (!e) e = hipStreamSynchronize(s);
  if (e) {
    delete L;
    ctx->err = std::string("qp_fri_layer_commit: ") + hipGetErrorString(e);
    return QP_ERR_HIP;
  }
  if (out) *out = L;
  else delete L;
  return QP_OK;
}

int qp_fri_layer_open(qp_fri_layer *L, const uint32_t *idx, uint32_t nidx, uint64_t *evals_out, uint64_t *siblings_out) {
  if (!L || (!idx && nidx) || (nidx && (!evals_out || !siblings_out))) return QP_ERR_ARG;
  if (!nidx) return QP_OK;
  qp_ctx *ctx = L->ctx;
  const uint32_t log_leaves = L->log_values - L->arity_bits;
  for (uint32_t i = 0; i < nidx; i++)
    if (idx[i] >> log_leaves) {
      ctx->err = "qp_fri_layer_open: leaf index out of range";
      return QP_ERR_ARG;
    }
  QP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const uint32_t W = 2u << L->arity_bits, depth = log_leaves - L->cap_h;
  DevBuf d_idx, d_ev, d_sib;
  QP_HIP_TRY(ctx, d_idx.alloc((nidx + 1) / 2));
  QP_HIP_TRY(ctx, d_ev.alloc((uint64_t)nidx * W));
  QP_HIP_TRY(ctx, d_sib.alloc((uint64_t)nidx * depth * 4));
  QP_HIP_TRY(ctx, hipMemcpyAsync(d_idx.p, idx, nidx * 4ull, hipMemcpyHostToDevice, s));
  qpk::gather_fri_leaf(L->vals.p, 0, L->log_values, L->arity_bits, d_idx.as<uint32_t>(), nidx, 0, d_ev.p, 0, 1, s);
  qpk::gather_paths(L->dig.p, 0, log_leaves, L->cap_h, d_idx.as<uint32_t>(), nidx, 0, d_sib.p, 0, 1, s);
  QP_HIP_TRY(ctx, hipGetLastError());
  QP_HIP_TRY(ctx, hipMemcpyAsync(evals_out, d_ev.p, (uint64_t)nidx * W * 8, hipMemcpyDeviceToHost, s));
  if (depth)
    QP_HIP_TRY(ctx, hipMemcpyAsync(siblings_out, d_sib.p, (uint64_t)nidx * depth * 32, hipMemcpyDeviceToHost, s));
  QP_HIP_TRY(ctx, hipStreamSynchronize(s));
  return QP_OK;
}

void qp_fri_layer_free(qp_fri_layer *L) { delete L; }

int qp_fri_fold(qp_ctx *ctx, const uint64_t *coeffs, uint32_t log_coeffs, uint32_t arity_bits, const uint64_t beta[2],
                uint64_t *coeffs_out) {
  if (!ctx || !coeffs || !beta || !coeffs_out || arity_bits < 1 || arity_bits > log_coeffs || log_coeffs > 20)
    return QP_ERR_ARG;
  QP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const uint64_t L = 1ull << log_coeffs, Lo = L >> arity_bits;
  std::vector<uint64_t> chal(qpk::CHAL_STRIDE, 0);
  chal[qpk::CH_FRI_BETA] = gl::canon(beta[0]);
  chal[qpk::CH_FRI_BETA + 1] = gl::canon(beta[1]);
  DevBuf d_in, d_out, d_chal;
  QP_HIP_TRY(ctx, d_in.alloc(2 * L));
  QP_HIP_TRY(ctx, d_out.alloc(2 * Lo));
  QP_HIP_TRY(ctx, d_chal.alloc(chal.size()));
  QP_HIP_TRY(ctx, hipMemcpyAsync(d_in.p, coeffs, 2 * L * 8, hipMemcpyHostToDevice, s));
  QP_HIP_TRY(ctx, hipMemcpyAsync(d_chal.p, chal.data(), chal.size() * 8, hipMemcpyHostToDevice, s));
  qpk::fold(d_in.p, d_out.p, log_coeffs, arity_bits, 0, d_chal.p, 0, 0, log_coeffs, 1, s);
  QP_HIP_TRY(ctx, hipGetLastError());
  QP_HIP_TRY(ctx, hipMemcpyAsync(coeffs_out, d_out.p, 2 * Lo * 8, hipMemcpyDeviceToHost, s));
  QP_HIP_TRY(ctx, hipStreamSynchronize(s));
  return QP_OK;
}

int qp_pow_grind(qp_ctx *ctx, const uint64_t *states, const uint32_t *pos, uint32_t n, uint32_t pow_bits,
                 uint64_t *witness_out) {
  if (!ctx || !states || !pos || !witness_out || !n || pow_bits == 0 || pow_bits > 32) return QP_ERR_ARG;
  for (uint32_t b = 0; b < n; b++)
    if (pos[b] >= 8) {  // Challenger invariant: input_buffer.len() < RATE when the witness is observed
      ctx->err = "qp_pow_grind: witness position must be < 8";
      return QP_ERR_ARG;
    }
  QP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  try {
    std::vector<uint64_t> pre((size_t)n * 24), found(n);
    for (uint32_t b = 0; b < n; b++) {
      uint64_t st[12];
      for (int i = 0; i < 12; i++) st[i] = gl::canon(states[(size_t)b * 12 + i]);
      qpk::pow_prestate(st, pos[b], pre.data() + (size_t)b * 24);
    }
    DevBuf d_pre, d_pos, d_next, d_found;
    QP_HIP_TRY(ctx, d_pre.alloc(pre.size()));
    QP_HIP_TRY(ctx, d_pos.alloc((n + 1) / 2));
    QP_HIP_TRY(ctx, d_next.alloc(n));
    QP_HIP_TRY(ctx, d_found.alloc(n));
    QP_HIP_TRY(ctx, hipMemcpyAsync(d_pre.p, pre.data(), pre.size() * 8, hipMemcpyHostToDevice, s));
    QP_HIP_TRY(ctx, hipMemcpyAsync(d_pos.p, pos, n * 4ull, hipMemcpyHostToDevice, s));
    // the prover's single-launch minimal-witness search (prover.cpp stage 6)
    QP_HIP_TRY(ctx, qpk::pow_search(d_pre.p, d_pos.as<uint32_t>(), d_found.p, d_next.p, n, pow_bits, s));
    QP_HIP_TRY(ctx, hipMemcpyAsync(found.data(), d_found.p, n * 8ull, hipMemcpyDeviceToHost, s));
    QP_HIP_TRY(ctx, hipStreamSynchronize(s));
    for (uint32_t b = 0; b < n; b++)
      if (found[b] == ~0ull) {
        ctx->err = "qp_pow_grind: no witness below the search limit";
        return QP_ERR_STATE;
      }
    memcpy(witness_out, found.data(), n * 8ull);
  } catch (const std::bad_alloc &) {
    return QP_ERR_OOM;
  }
  return QP_OK;
}

// ---- partial products / Z, the opening set, the initial FRI polynomial ------
// The whole-circuit prover's stages 2, 4 and 5 (prover.cpp) for one proof of
// any circuit: the same kernels, reading a one-proof challenge block
// (CHAL_STRIDE words, proof index 0) that the seam fills from its arguments.
// Every precondition the kernels assume is checked here before a launch.

int qp_perm_new(qp_ctx *ctx, const uint64_t *sigmas, const uint64_t *k_is, uint32_t num_routed, uint32_t log_n,
                qp_perm **out) {
  if (!ctx || !out) return QP_ERR_ARG;
  *out = nullptr;
  if (!sigmas || !k_is) {
    ctx->err = "qp_perm_new: null argument";
    return QP_ERR_ARG;
  }
  if (log_n < SEAM_LOG_MIN || log_n > SEAM_LOG_MAX || num_routed < 1 || num_routed > 16 * PP_MAX_CHUNKS) {
    ctx->err = "qp_perm_new: unsupported shape (2^6 <= n <= 2^15, 1 <= num_routed <= 256)";
    return QP_ERR_ARG;
  }
  QP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  qp_perm *p = new (std::nothrow) qp_perm();
  if (!p) return QP_ERR_OOM;
  p->ctx = ctx;
  p->R = num_routed;
  p->log_n = log_n;
  const uint64_t n = 1ull << log_n;
  std::vector<uint64_t> k(num_routed);
  for (uint32_t j = 0; j < num_routed; j++) k[j] = gl::canon(k_is[j]);
  hipError_t e = p->sigmas.alloc((size_t)num_routed * n);
  if (!e) e = p->kis.alloc(num_routed);
  if (!e) e = hipMemcpyAsync(p->sigmas.p, sigmas, (size_t)num_routed * n * 8, hipMemcpyHostToDevice, ctx->stream);
  if (!e) e = hipMemcpyAsync(p->kis.p, k.data(), (size_t)num_routed * 8, hipMemcpyHostToDevice, ctx->stream);
  if (!e) e = hipStreamSynchronize(ctx->stream);
  if (e) {
    delete p;
    ctx->err = std::string("qp_perm_new: ") + hipGetErrorString(e);
    return e == hipErrorOutOfMemory ? QP_ERR_OOM : QP_ERR_HIP;
  }
  *out = p;
  return QP_OK;
}

void qp_perm_free(qp_perm *p) { delete p; }

int qp_partial_products_and_zs(qp_perm *p, const uint64_t *wires, uint32_t qdf, const uint64_t *betas,
                               const uint64_t *gammas, uint32_t nc, uint64_t *zs_pp_out) {
  if (!p) return QP_ERR_ARG;
  qp_ctx *ctx = p->ctx;
  if (!wires || !betas || !gammas || !zs_pp_out) {
    ctx->err = "qp_partial_products_and_zs: null argument";
    return QP_ERR_ARG;
  }
  const uint32_t R = p->R, log_n = p->log_n;
  const uint32_t nchunks = qdf ? (R + qdf - 1) / qdf : 0;
  // k_pp_rows keeps PP_MAX_CHUNKS chunk products per row; the challenge block holds two challenges
  if (nc < 1 || nc > 2 || qdf < 1 || nchunks > PP_MAX_CHUNKS) {
    ctx->err = "qp_partial_products_and_zs: unsupported shape (1 or 2 challenges, at most 16 chunks of quotient_degree_factor)";
    return QP_ERR_ARG;
  }
  const uint64_t n = 1ull << log_n, pbs = (uint64_t)nc * nchunks * n;
  QP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  std::vector<uint64_t> chal(qpk::CHAL_STRIDE, 0);
  for (uint32_t c = 0; c < nc; c++) {
    chal[qpk::CH_BETA + c] = gl::canon(betas[c]);
    chal[qpk::CH_GAMMA + c] = gl::canon(gammas[c]);
  }
  qpk::perm_challenges(chal.data(), chal.data() + qpk::CH_BETA, chal.data() + qpk::CH_GAMMA, nc, R, qdf);
  DevBuf d_w, d_prods, d_zs, d_chal;
  QP_HIP_TRY(ctx, d_w.alloc((uint64_t)R * n));
  QP_HIP_TRY(ctx, d_prods.alloc(pbs));
  QP_HIP_TRY(ctx, d_zs.alloc(pbs));
  QP_HIP_TRY(ctx, d_chal.alloc(chal.size()));
  QP_HIP_TRY(ctx, hipMemcpyAsync(d_w.p, wires, (uint64_t)R * n * 8, hipMemcpyHostToDevice, s));
  QP_HIP_TRY(ctx, hipMemcpyAsync(d_chal.p, chal.data(), chal.size() * 8, hipMemcpyHostToDevice, s));
  // prover.cpp stage 2
  qpk::partial_products_and_zs(ctx->tw, d_w.p, 0, p->sigmas.p, p->kis.p, d_chal.p, d_prods.p, d_zs.p, 0, log_n, R, qdf,
                               nc, 1, s);
  QP_HIP_TRY(ctx, hipGetLastError());
  QP_HIP_TRY(ctx, hipMemcpyAsync(zs_pp_out, d_zs.p, pbs * 8, hipMemcpyDeviceToHost, s));
  QP_HIP_TRY(ctx, hipStreamSynchronize(s));
  return QP_OK;
}

int qp_opening_set(qp_ctx *ctx, const qp_batch *cs, const qp_batch *wires, const qp_batch *zs_pp,
                   const qp_batch *quotient, uint32_t nc, const uint64_t zeta[2], uint64_t *out) {
  if (!ctx) return QP_ERR_ARG;
  const qp_batch *bt[4] = {cs, wires, zs_pp, quotient};
  std::vector<uint64_t> chal(qpk::CHAL_STRIDE, 0);
  int rc = check_circuit_batches(ctx, "qp_opening_set", bt, nc, zeta, out, chal.data());
  if (rc) return rc;
  const uint32_t log_n = cs->log_n;
  const uint64_t total = (uint64_t)cs->npolys + wires->npolys + zs_pp->npolys + quotient->npolys + nc;
  if (2 * total > qpk::OPEN_STRIDE) {
    ctx->err = "qp_opening_set: more than 260 openings (use qp_batch_eval_ext per batch)";
    return QP_ERR_ARG;
  }
  QP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  DevBuf d_chal, d_out, d_part;
  QP_HIP_TRY(ctx, d_chal.alloc(chal.size()));
  QP_HIP_TRY(ctx, d_out.alloc(qpk::OPEN_STRIDE));
  QP_HIP_TRY(ctx, d_part.alloc((uint64_t)qpk::OPEN_MAX_SLICES * qpk::OPEN_STRIDE));
  QP_HIP_TRY(ctx, hipMemcpyAsync(d_chal.p, chal.data(), chal.size() * 8, hipMemcpyHostToDevice, s));
  // prover.cpp stage 4: the zeta batch in oracle order, then the Zs at g*zeta
  qpk::OpeningsArgs oa;
  uint32_t off = 0;
  for (int i = 0; i < 4; i++) {
    oa.seg[oa.nseg++] = qpk::OpenSeg{bt[i]->d_coeffs, 0, bt[i]->npolys, qpk::CH_ZETA, off, 0};
    off += bt[i]->npolys;
  }
  oa.seg[oa.nseg++] = qpk::OpenSeg{zs_pp->d_coeffs, 0, nc, qpk::CH_ZETA_NEXT, off, 0};
  oa.log_n = log_n;
  oa.pts = d_chal.p;
  oa.out = d_out.p;
  oa.part = d_part.p;
  qpk::openings(oa, 1, s);
  QP_HIP_TRY(ctx, hipGetLastError());
  QP_HIP_TRY(ctx, hipMemcpyAsync(out, d_out.p, total * 16, hipMemcpyDeviceToHost, s));
  QP_HIP_TRY(ctx, hipStreamSynchronize(s));
  return QP_OK;
}

int qp_batch_eval_ext(const qp_batch *b, uint32_t first, uint32_t npolys, const uint64_t *points, uint32_t npts,
                      uint64_t *out) {
  if (!b || !b->ctx) return QP_ERR_ARG;
  qp_ctx *ctx = b->ctx;
  if (!points || !out) {
    ctx->err = "qp_batch_eval_ext: null argument";
    return QP_ERR_ARG;
  }
  if (b->nbat != 1 || !b->d_coeffs || npolys < 1 || npts < 1 || first > b->npolys || npolys > b->npolys - first ||
      (uint64_t)npts * npolys > (1u << 20) || b->log_n > qpk::BIG_LOG_MAX) {
    ctx->err = "qp_batch_eval_ext: unsupported shape (a batch of one proof holding its coefficients, a window "
               "inside it, at most 2^20 values)";
    return QP_ERR_ARG;
  }
  // one segment per (point, window of at most ROW polynomials), packed into launches of at most
  // OPEN_MAX_SEG segments and one OPEN_STRIDE row of results each
  constexpr uint32_t ROW = qpk::OPEN_STRIDE / 2;
  struct Piece { uint32_t launch, row_off, pt, p0, np; };
  std::vector<Piece> pieces;
  std::vector<qpk::OpeningsArgs> launches;
  try {
    uint32_t used = ROW;  // forces the first launch
    for (uint32_t q = 0; q < npts; q++)
      for (uint32_t p0 = 0; p0 < npolys; p0 += ROW) {
        const uint32_t np = std::min(ROW, npolys - p0);
        if (launches.empty() || used + np > ROW || launches.back().nseg == qpk::OPEN_MAX_SEG) {
          launches.emplace_back();
          used = 0;
        }
        qpk::OpeningsArgs &oa = launches.back();
        oa.seg[oa.nseg++] = qpk::OpenSeg{b->d_coeffs + (uint64_t)(first + p0) * b->n(), 0, np, 2 * q, used, 0};
        pieces.push_back(Piece{(uint32_t)launches.size() - 1, used, q, p0, np});
        used += np;
      }
    std::vector<uint64_t> pts(2 * (size_t)npts), res(launches.size() * (size_t)qpk::OPEN_STRIDE);
    for (size_t i = 0; i < pts.size(); i++) pts[i] = gl::canon(points[i]);
    QP_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    DevBuf d_pts, d_out, d_part;
    QP_HIP_TRY(ctx, d_pts.alloc(pts.size()));
    QP_HIP_TRY(ctx, d_out.alloc(res.size()));
    QP_HIP_TRY(ctx, d_part.alloc((uint64_t)qpk::OPEN_MAX_SLICES * qpk::OPEN_STRIDE));
    QP_HIP_TRY(ctx, hipMemcpyAsync(d_pts.p, pts.data(), pts.size() * 8, hipMemcpyHostToDevice, s));
    for (size_t l = 0; l < launches.size(); l++) {
      qpk::OpeningsArgs &oa = launches[l];
      oa.log_n = b->log_n;
      oa.pts = d_pts.p;  // proof index 0: the point of a segment is pts[pt_off], pts[pt_off + 1]
      oa.out = d_out.p + l * (size_t)qpk::OPEN_STRIDE;
      oa.part = d_part.p;  // launches are ordered on the stream: the scratch is free again
      qpk::openings(oa, 1, s);
    }
    QP_HIP_TRY(ctx, hipGetLastError());
    QP_HIP_TRY(ctx, hipMemcpyAsync(res.data(), d_out.p, res.size() * 8, hipMemcpyDeviceToHost, s));
    QP_HIP_TRY(ctx, hipStreamSynchronize(s));
    for (const Piece &pc : pieces)
      memcpy(out + 2 * ((size_t)pc.pt * npolys + pc.p0),
             res.data() + pc.launch * (size_t)qpk::OPEN_STRIDE + 2 * (size_t)pc.row_off, (size_t)pc.np * 16);
  } catch (const std::bad_alloc &) {
    return QP_ERR_OOM;
  }
  return QP_OK;
}

int qp_fri_initial_poly(qp_ctx *ctx, const qp_batch *cs, const qp_batch *wires, const qp_batch *zs_pp,
                        const qp_batch *quotient, uint32_t nc, const uint64_t alpha[2], const uint64_t zeta[2],
                        uint64_t *coeffs_out) {
  if (!ctx) return QP_ERR_ARG;
  const qp_batch *bt[4] = {cs, wires, zs_pp, quotient};
  std::vector<uint64_t> chal(qpk::CHAL_STRIDE, 0);
  int rc = check_circuit_batches(ctx, "qp_fri_initial_poly", bt, nc, zeta, coeffs_out, chal.data());
  if (rc) return rc;
  if (!alpha) {
    ctx->err = "qp_fri_initial_poly: null argument";
    return QP_ERR_ARG;
  }
  const uint32_t log_n = cs->log_n;
  const uint64_t n = 1ull << log_n;
  QP_HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  qpk::fri_alpha_words(chal.data(), gl::ext{gl::canon(alpha[0]), gl::canon(alpha[1])}, nc);
  DevBuf d_chal, d_comp, d_fin;
  QP_HIP_TRY(ctx, d_chal.alloc(chal.size()));
  QP_HIP_TRY(ctx, d_comp.alloc(4 * n));
  QP_HIP_TRY(ctx, d_fin.alloc(2 * n));
  QP_HIP_TRY(ctx, hipMemcpyAsync(d_chal.p, chal.data(), chal.size() * 8, hipMemcpyHostToDevice, s));
  // prover.cpp stage 5
  qpk::FriComposeArgs fa;
  for (int i = 0; i < 4; i++) {
    fa.coeffs[i] = bt[i]->d_coeffs;
    fa.bstride[i] = 0;
    fa.npolys[i] = bt[i]->npolys;
  }
  fa.noracles = 4;
  fa.nnext = nc;
  fa.log_n = log_n;
  fa.chal = d_chal.p;
  fa.comp = d_comp.p;
  qpk::fri_initial_poly(fa, d_fin.p, 0, n, 1, s);
  QP_HIP_TRY(ctx, hipGetLastError());
  QP_HIP_TRY(ctx, hipMemcpyAsync(coeffs_out, d_fin.p, 2 * n * 8, hipMemcpyDeviceToHost, s));
  QP_HIP_TRY(ctx, hipStreamSynchronize(s));
  return QP_OK;
}

}  // extern "C"
