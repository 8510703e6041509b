// prover_kernels.h — argument layouts and launchers of the prover's stage
// files (pp_z.hip, quotient.hip, openings.hip, fri.hip, pow.hip).  Every stage
// of prove() has one launcher, defined next to the kernels it launches: it
// owns the kernel choice and the grid, block and LDS sizes, and both callers
// go through it: prove_batch (prover.cpp: nb proofs, per-proof strides) and
// the seams (seams.cpp, capi.cpp: one proof, strides 0).  The kernels
// themselves are declared nowhere outside their file.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "field.h"
#include "gates.h"
#include "kernels.h"
#include "ntt_device.h"

#include <vector>

namespace qpk {

// host helpers (prover.cpp)
std::vector<uint64_t> quotient_point_tables(uint32_t log_n, uint32_t rate_bits);
void pow_prestate(const uint64_t st12[12], uint32_t pos, uint64_t pre[24]);

// per-proof challenge block (device, u64 words)
enum : uint32_t {
  CH_BETA = 0, CH_GAMMA = 2, CH_ALPHA = 4, CH_PIH = 6, CH_ZETA = 10, CH_ZETA_NEXT = 12, CH_ZETA_INV = 14,
  CH_ZETA_NEXT_INV = 16, CH_FRI_ALPHA = 18, CH_ALPHA_POW_NC = 20, CH_FRI_BETA = 22,
  // the permutation argument scaled by 1 / beta (k_quotient_1r): (w + gamma +
  // beta s) = beta (w / beta + gamma / beta + s), the beta^len of a chunk's
  // products applied once per chunk (len = qdf, or the last chunk's R mod qdf).
  // beta = 0 has no inverse: then the words hold 1, gamma, 1, 1 and CH_S_MASK
  // (all ones otherwise) is 0, which clears the s term: the factor is w + gamma
  CH_BETA_INV = 32, CH_GAMMA_B = 34, CH_BETA_QDF = 36, CH_BETA_LAST = 38, CH_S_MASK = 40, CHAL_STRIDE = 42
};
constexpr uint32_t MAX_FRI_LAYERS = (CH_BETA_INV - CH_FRI_BETA) / 2;
// the permutation-argument words of the challenge block for challenges beta, gamma
void perm_challenges(uint64_t *ch, const uint64_t *beta, const uint64_t *gamma, uint32_t nc, uint32_t R, uint32_t qdf);
// zeta, g * zeta (g = w_n) and their inverses: CH_ZETA .. CH_ZETA_NEXT_INV (zeta != 0)
void open_point_words(uint64_t *ch, gl::ext zeta, uint32_t log_n);
// the FRI alpha and alpha^nc: CH_FRI_ALPHA, CH_ALPHA_POW_NC
void fri_alpha_words(uint64_t *ch, gl::ext alpha, uint32_t nc);
// apow[i] = alpha^i, i < nterms: one challenge's row of the quotient's table (APOW_STRIDE)
void alpha_powers(uint64_t *apow, uint64_t alpha, uint32_t nterms);
constexpr uint32_t OPEN_STRIDE = 520;  // 257 ext openings per proof (+pad)
constexpr uint32_t APOW_STRIDE = 256;  // alpha_c^i, i < #vanishing terms (per challenge)

// ---- pp_z.hip
// wires_permutation_partial_products_and_zs for nb proofs: the chunk products
// of every row (prods: scratch of nc * ceil(R / qdf) * n words per proof; the
// compile-time kernel for the leaf circuits' shape), then their running
// product into zs [nc * ceil(R / qdf)][n] per proof (rows staged in LDS up to
// n = 2^LDS_LOG_MAX, read from HBM above)
void partial_products_and_zs(const Twiddles &tw, const uint64_t *wires, uint64_t w_bstride, const uint64_t *sigmas,
                             const uint64_t *k_is, const uint64_t *chal, uint64_t *prods, uint64_t *zs,
                             uint64_t z_bstride, uint32_t log_n, uint32_t R, uint32_t qdf, uint32_t nc, uint32_t nb,
                             hipStream_t s);

// ---- quotient.hip
using namespace qg;  // gate kinds (gates.h)
// RandomAccessGate width k_quotient_1r evaluates (the recursive verifier's
// RandomAccessGate::new_from_config shape); other widths take the per-gate
// launches (k_quotient_part)
constexpr uint32_t RA_QBITS = 4;
constexpr uint32_t MAX_GATES_DEV = 16;

struct GateDesc {
  uint32_t ngates = 0, nsel = 0;
  uint32_t kind[MAX_GATES_DEV] = {0}, param[MAX_GATES_DEV] = {0}, param2[MAX_GATES_DEV] = {0},
           param3[MAX_GATES_DEV] = {0}, sel_index[MAX_GATES_DEV] = {0}, grp_lo[MAX_GATES_DEV] = {0},
           grp_hi[MAX_GATES_DEV] = {0};
};

static_assert(MAX_GATES_DEV == QP_MAX_GATES, "GateDesc holds an ABI gate description");
// the kernels' form of a gate description
inline GateDesc gate_desc_dev(const qp_gate_desc &g) {
  GateDesc d;
  d.ngates = g.num_gates;
  d.nsel = g.num_selectors;
  for (uint32_t i = 0; i < g.num_gates; i++) {
    d.kind[i] = g.kind[i];
    d.param[i] = g.param[i];
    d.param2[i] = g.param2[i];
    d.param3[i] = g.param3[i];
    d.sel_index[i] = g.selector_index[i];
  }
  for (uint32_t i = 0; i < g.num_selectors; i++) {
    d.grp_lo[i] = g.group_lo[i];
    d.grp_hi[i] = g.group_hi[i];
  }
  return d;
}

struct QuotientArgs {
  const uint64_t *cs_lde, *w_lde, *z_lde;
  uint64_t w_bstride, z_bstride;
  const uint64_t *chal, *tw, *apow;
  const uint64_t *xtab, *l0tab;  // [N] leaf order: x = g w_N^rev(t), L_0(x)
  uint64_t zh[16], zh_inv[16];
  uint64_t *q_out;
  uint64_t q_bstride;
  uint32_t log_n, rate_bits, R, qdf, num_constants;
  GateDesc g;
};
// zh[k] = Z_H on coset k of the LDE domain (x^n - 1 at x = g w_N^k) and its inverse
void quotient_zh(QuotientArgs &a, uint32_t log_n, uint32_t rate_bits);

// compute_quotient_polys (plonk/prover.rs) as launches, shared by the prover's
// stage 3 and the qp_quotient seam: the vanishing-polynomial values at every
// LDE point of nb proofs with the chosen kernel(s) ...
enum QuotientKernel : uint32_t {
  QK_1R,    // k_quotient_1r: the leaf gate set, every column read once
  QK_PARTS  // k_quotient_part: permutation terms, then one launch per gate (any gate list)
};
// the kernel a gate list takes.  k_quotient_1r's precondition: kinds among
// Noop, Constant, PublicInput, BaseSum, Arithmetic, Poseidon and RandomAccess
// of RA_QBITS bits, each at most once, the Constant, PublicInput, BaseSum and
// Arithmetic reads inside the R routed wires it sweeps; anything else, and the
// path hook quotient_parts=1, takes the per-gate launches
QuotientKernel quotient_kernel(const GateDesc &g, uint32_t R);
void quotient_values(const QuotientArgs &a, QuotientKernel k, uint32_t nb, hipStream_t s);
// ... and their coset iNTT into nc * qdf * n coefficients per proof (qvals
// [nb][nc][N] leaf order -> coeffs [nb][nc][qdf * n]; cbuf: scratch of the
// size of qvals); LDS form up to n = 2^LDS_LOG_MAX, HBM levels above
void quotient_coeffs(const Twiddles &tw, const uint64_t *qvals, uint64_t *cbuf, uint64_t *coeffs, uint32_t log_n,
                     uint32_t rate_bits, uint32_t nc, uint32_t nb, uint64_t v_bstride, uint64_t c_bstride,
                     uint64_t o_bstride, hipStream_t s);

// ---- openings.hip
// every opening batch of a proof (OpeningSet::new's zeta and g*zeta
// evaluations) in one launch (+ a reduction when the coefficient range is
// split over S slices); out[b][OPEN_STRIDE] as k_openings writes it
constexpr int OPEN_MAX_SEG = 6, OPEN_MAX_SLICES = 16;
struct OpenSeg {
  const uint64_t *coeffs;
  uint64_t c_bstride;
  uint32_t npolys, pt_off, out_off, g0;
};
struct OpeningsArgs {
  OpenSeg seg[OPEN_MAX_SEG];
  uint32_t nseg = 0, ngroups = 0, log_n = 0, S = 1, ntot = 0;
  const uint64_t *pts = nullptr;
  uint64_t *out = nullptr, *part = nullptr;  // part: nb * OPEN_MAX_SLICES * OPEN_STRIDE words
};
void openings(OpeningsArgs a, uint32_t nb, hipStream_t s);

// ---- fri.hip
struct FriComposeArgs {
  const uint64_t *coeffs[4];
  uint64_t bstride[4];
  uint32_t npolys[4];
  uint32_t noracles, nnext, log_n;
  const uint64_t *chal;
  uint64_t *comp;
};
// the polynomial FRI starts from (PolynomialBatch::prove_openings) for nb
// proofs: a.comp (4 n words per proof) = the alpha-reduced oracles, then
// fin [2][f_cstride] per proof = alpha^nc comp / (X - zeta) + comp_next / (X - g zeta),
// n coefficients each; 2^6 <= n <= 2^16
void fri_initial_poly(const FriComposeArgs &a, uint64_t *fin, uint64_t f_bstride, uint64_t f_cstride, uint32_t nb,
                      hipStream_t s);
// the leaf digests of a FRI layer for nb proofs (row or one-lane form by size)
void fri_leaf(const uint64_t *vals, uint64_t *dig, uint32_t log_len, uint32_t ab, uint64_t v_bstride,
              uint64_t d_bstride, uint32_t nb, hipStream_t s);
// one FRI reduction layer's commitment for nb proofs: values = coset_fft(coef,
// shift) of size 2^log_len in leaf order (coef: [2][coef_cstride] per proof,
// 2^coef_log of them possibly nonzero), the leaf digests of 2^ab values each
// and the tree over them (dig: tree_digest_count(log_len - ab, cap_h) * 4 words per proof)
void fri_layer_tree(const Twiddles &tw, const uint64_t *coef, uint64_t coef_cstride, uint64_t coef_bstride,
                    uint32_t coef_log, uint64_t *vals, uint64_t *dig, uint32_t log_len, uint32_t ab, uint32_t cap_h,
                    uint64_t shift, uint32_t nb, hipStream_t s);
// one FRI fold of nb proofs with beta = the layer's CH_FRI_BETA pair: cin
// [2][2^log_len] -> cout [2][2^(log_len - ab)]; 2^log_nz: the possibly nonzero prefix of cin
void fold(const uint64_t *cin, uint64_t *cout, uint32_t log_len, uint32_t ab, uint32_t layer, const uint64_t *chal,
          uint64_t i_bstride, uint64_t o_bstride, uint32_t log_nz, uint32_t nb, hipStream_t s);
// query openings of nb proofs at leaves idx[b][q] >> shift: rows of an LDE
// matrix (out[b][q][ncols]), Merkle paths (out[b][q][depth][4], depth =
// log_leaves - cap_h) and FRI layer leaves (out[b][q][2 << ab]).  Nothing is
// launched for an empty result (no queries, a tree that is all cap)
void gather_rows(const uint64_t *cols, uint64_t stride, uint64_t bstride, uint32_t ncols, const uint32_t *idx,
                 uint32_t nq, uint32_t shift, uint64_t *out, uint64_t o_bstride, uint32_t nb, hipStream_t s);
void gather_paths(const uint64_t *dig, uint64_t d_bstride, uint32_t log_leaves, uint32_t cap_h, const uint32_t *idx,
                  uint32_t nq, uint32_t shift, uint64_t *out, uint64_t o_bstride, uint32_t nb, hipStream_t s);
void gather_fri_leaf(const uint64_t *vals, uint64_t v_bstride, uint32_t log_len, uint32_t ab, const uint32_t *idx,
                     uint32_t nq, uint32_t shift, uint64_t *out, uint64_t o_bstride, uint32_t nb, hipStream_t s);

// ---- pow.hip
// fri_proof_of_work's minimal witness per proof in one launch: found[b] = the
// least witness below 2^min(bits + 20, 62), all ones if none (found and the
// claim counters next are reset here)
hipError_t pow_search(const uint64_t *states, const uint32_t *pos, uint64_t *found, uint64_t *next, uint32_t nb,
                      uint32_t bits, hipStream_t s);

}  // namespace qpk
