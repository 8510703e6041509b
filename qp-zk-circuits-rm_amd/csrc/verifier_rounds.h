// verifier_rounds.h — the query-round checks of plonky2's verify_fri_proof
// (fri/verifier.rs fri_verifier_query_round, hash/merkle_proofs.rs
// verify_merkle_proof_to_cap), one call per lane, written once for the gfx950
// kernels (verifier.hip) and the host path (verifier.cpp, ctx == NULL).  The
// caller supplies the permutation: H::permute (any 12-element state) and
// H::node (state[8..11] == 0, lanes 0..3 read); values may stay non-canonical
// in [0, 2^64) between permutations, the comparison canonicalises.
//
// All counts, strides and indices in PathJob / FriJob come from the parsed
// CommonCircuitData and the host's own transcript, never from proof bytes; the
// arrays hold canonical field elements repacked to aligned u64.
#pragma once
#include <stdint.h>
#include "field.h"

namespace qv {

constexpr uint32_t MAX_LAYERS = 8, MAX_CLASSES = 4 + MAX_LAYERS;

// one Merkle tree's openings: lane i proves leaves[i] at idx[i] against the cap
// at caps + (i / per_cap) * cap_stride
struct PathClass {
  const uint64_t *leaves;  // [n][width]
  const uint64_t *sibs;    // [n][nsib][4]
  const uint32_t *idx;     // [n]
  const uint64_t *caps;    // [.][2^cap_height][4]
  uint64_t cap_stride;
  uint32_t width, nsib, per_cap, n;
};
struct PathJob {
  PathClass cls[MAX_CLASSES];
  uint32_t ncls, cap_height, total;  // total = sum of cls[].n; lanes are class-major
  uint8_t *ok;                       // [total]
};

// one lane per (proof, query): n = proofs * nq
struct FriJob {
  const uint64_t *leaves[4];  // the initial trees' opened leaves, [n][width[o]]
  uint32_t width[4], unsalted[4];
  const uint64_t *evals[MAX_LAYERS];  // per layer the opened coset, [n][2 << arity_bits]
  uint32_t arity_bits[MAX_LAYERS];
  uint32_t nlayers, nq, log_N, nc, final_len, n;
  // per proof: zeta, g zeta, alpha, alpha^nc, the two reduced openings, the
  // layer betas (extension elements, 2 words each), the final polynomial's
  // coefficients, then the nq query indices
  const uint64_t *pp;
  uint32_t pp_stride;
  uint32_t *code;  // [n]: 0, 8, or 6 | layer << 8
};
constexpr uint32_t PP_ZETA = 0, PP_ZETA_NEXT = 2, PP_ALPHA = 4, PP_ALPHA_NC = 6, PP_RED0 = 8, PP_RED1 = 10, PP_BETAS = 12;

template <class H>
QP_HD bool path_ok(const PathClass &c, uint32_t cap_height, uint32_t i) {
  const uint32_t x = c.idx[i];
  if (((uint64_t)x >> c.nsib) >> cap_height) return false;  // no cap entry
  const uint64_t *leaf = c.leaves + (uint64_t)i * c.width;
  uint64_t s[12];
#pragma unroll
  for (int k = 0; k < 12; k++) s[k] = 0;
  if (c.width <= 4) {  // hash_or_noop: short leaves are padded, not hashed
#pragma unroll
    for (uint32_t k = 0; k < 4; k++)
      if (k < c.width) s[k] = leaf[k];
  } else {
    for (uint32_t off = 0; off < c.width; off += 8) {
#pragma unroll
      for (uint32_t k = 0; k < 8; k++)
        if (off + k < c.width) s[k] = leaf[off + k];
      H::permute(s);
    }
  }
  const uint64_t *sib = c.sibs + (uint64_t)i * c.nsib * 4;
  for (uint32_t k = 0; k < c.nsib; k++, sib += 4) {
    const bool right = (x >> k) & 1;  // this node is the right child
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint64_t h = s[j], o = sib[j];
      s[j] = right ? o : h;
      s[4 + j] = right ? h : o;
    }
    s[8] = s[9] = s[10] = s[11] = 0;
    H::node(s);
  }
  // nsib may be 32 (a 32-bit shift by it is undefined): shift in 64 bits, as the guard above does
  const uint64_t *cap = c.caps + (uint64_t)(i / c.per_cap) * c.cap_stride + ((uint64_t)x >> c.nsib) * 4;
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 4; j++) ok = ok && gl::canon(s[j]) == cap[j];
  return ok;
}

QP_HD gl::ext ld_ext(const uint64_t *p) { return gl::ext{p[0], p[1]}; }

// compute_evaluation: the polynomial through (start ga^i, evals[rev(i)]) at
// beta, barycentric form (the points are base-field, so are the weights)
QP_HD gl::ext interpolate_coset(const uint64_t *evals, uint32_t ab, uint64_t start, uint64_t ga, gl::ext beta) {
  const uint32_t ar = 1u << ab;
  gl::ext res{0, 0};
  uint64_t xi = start;
  for (uint32_t i = 0; i < ar; i++) {
    uint64_t w = 1, xj = start;
    gl::ext num{1, 0};
    for (uint32_t j = 0; j < ar; j++) {
      if (j != i) {
        w = gl::mul(w, gl::sub(xi, xj));
        num = gl::ext_mul(num, gl::ext{gl::sub(beta.c0, xj), beta.c1});
      }
      xj = gl::mul(xj, ga);
    }
    const gl::ext y = ld_ext(evals + 2 * (uint64_t)gl::rev_bits(i, ab));
    res = gl::ext_add(res, gl::ext_mul(gl::ext_scale(y, gl::inv(w)), num));
    xi = gl::mul(xi, ga);
  }
  return res;
}

// the arithmetic of one query round: fri_combine_initial, per layer the
// consistency check and the fold, the final polynomial
QP_HD uint32_t fri_query(const FriJob &f, uint32_t i) {
  const uint64_t *pp = f.pp + (uint64_t)(i / f.nq) * f.pp_stride;
  const gl::ext zeta = ld_ext(pp + PP_ZETA), zeta_next = ld_ext(pp + PP_ZETA_NEXT), a = ld_ext(pp + PP_ALPHA);
  const uint64_t *final_poly = pp + PP_BETAS + 2 * f.nlayers;
  uint32_t xi = (uint32_t)final_poly[2 * f.final_len + (i % f.nq)];
  uint64_t sx = gl::mul(gl::GEN, gl::pow(gl::root_of_unity(f.log_N), gl::rev_bits(xi, f.log_N)));
  // sum_k t_k alpha^k over the unsalted values of the four leaves, Horner from the last
  gl::ext r0{0, 0};
  for (int o = 3; o >= 0; o--) {
    const uint64_t *leaf = f.leaves[o] + (uint64_t)i * f.width[o];
    for (uint32_t k = f.unsalted[o]; k-- > 0;) {
      r0 = gl::ext_mul(r0, a);
      r0.c0 = gl::add(r0.c0, leaf[k]);
    }
  }
  gl::ext r1{0, 0};
  {
    const uint64_t *leaf = f.leaves[2] + (uint64_t)i * f.width[2];
    for (uint32_t k = f.nc; k-- > 0;) {
      r1 = gl::ext_mul(r1, a);
      r1.c0 = gl::add(r1.c0, leaf[k]);
    }
  }
  const gl::ext s0 = gl::ext_mul(gl::ext_sub(r0, ld_ext(pp + PP_RED0)), gl::ext_inv(gl::ext{gl::sub(sx, zeta.c0), gl::neg(zeta.c1)}));
  const gl::ext s1 =
      gl::ext_mul(gl::ext_sub(r1, ld_ext(pp + PP_RED1)), gl::ext_inv(gl::ext{gl::sub(sx, zeta_next.c0), gl::neg(zeta_next.c1)}));
  gl::ext old = gl::ext_add(gl::ext_mul(s0, ld_ext(pp + PP_ALPHA_NC)), s1);
  for (uint32_t l = 0; l < f.nlayers; l++) {
    const uint32_t ab = f.arity_bits[l], ar = 1u << ab;
    const uint64_t *evals = f.evals[l] + (uint64_t)i * 2 * ar;
    const uint32_t within = xi & (ar - 1);
    if (!gl::ext_eq(ld_ext(evals + 2 * within), old)) return 6u | (l << 8);
    const uint64_t ga = gl::root_of_unity(ab);
    const uint64_t start = gl::mul(sx, gl::pow(ga, (ar - gl::rev_bits(within, ab)) % ar));
    old = interpolate_coset(evals, ab, start, ga, ld_ext(pp + PP_BETAS + 2 * l));
    for (uint32_t k = 0; k < ab; k++) sx = gl::sqr(sx);
    xi >>= ab;
  }
  gl::ext fx{0, 0};
  for (uint32_t k = f.final_len; k-- > 0;) fx = gl::ext_add(gl::ext_scale(fx, sx), ld_ext(final_poly + 2 * k));
  return gl::ext_eq(fx, old) ? 0u : 8u;
}

}  // namespace qv
