// poseidon_fast.h — Poseidon (width 12, x^7, 8 full + 22 partial rounds)
// written to the measured gfx950 VALU cost model (tools/isa_rates.hip,
// profiles/r01_isa_rates.log): almost every VALU op issues at one per 4
// cycles per SIMD (add/sub/logic/mov at 2), so the permutation is bound by
// its VALU instruction count and v_mad_u64_u32 — a 32x32+64 product-sum in one
// issue — is the densest instruction there is.
//
// Same function as ps::permute (poseidon.h), on the non-canonical field
// arithmetic of field_nc.h (the general product, the carry hazard rule and
// its QP_CWAIT pad live there); arithmetic discipline:
//   * state NON-canonical in [0, 2^64) (plonky2's GoldilocksField form);
//   * MDS row r = sum_i CIRC[i] * s[(i+r)%12] (+ DIAG) computed on 32-bit
//     halves as 24 explicit v_mad_u64_u32 with the small constants inline
//     (the compiler would otherwise strength-reduce them into longer
//     shift/add carry chains);
//   * the NEXT round's constant is folded into the first mad of each row
//     (addend = the constant's halves), so no round-constant additions are
//     executed except the first round's;
//   * each row reduces in 4 instructions: value = al + 2^32 ah with
//     al, ah < 2^60 (reduce_row) -> t = al + eps*hi32(ah) (one mad),
//     t.hi += lo32(ah) with carry c, t += c*eps; the fourth step of a dense
//     group (al, ah up to 2^63.72) in 5 (reduce_row_wide).
//   * sbox x^7 = x^3 * x^4 on gfn::mul.
// One form of each piece: the code-shape variants that were measured and lost
// (compiler mads, C reductions, rolled rounds, multi-row asm blocks) are rows
// of DESIGN.md §10.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>
#include "field_nc.h"
#include "poseidon.h"
#include "poseidon_dense4_consts.h"
#include "poseidon_dense_consts.h"
#include "poseidon_partial_consts.h"

namespace pf {

using gfn::EPS;
using gfn::canon;
using gfn::hi32;
using gfn::lo32;
using gfn::mul;
using gfn::mul_c;

// acc = x * C + add   (C an inline constant in [0, 64])
template <int C>
__device__ __forceinline__ uint64_t mad_c(uint32_t x, uint64_t add) {
  uint64_t r, cdummy;
  asm("v_mad_u64_u32 %0, %1, %2, %3, %4" : "=v"(r), "=s"(cdummy) : "v"(x), "i"(C), "v"(add));
  return r;
}
// acc = x * C + add, add a scalar (SGPR) 64-bit value
template <int C>
__device__ __forceinline__ uint64_t mad_cs(uint32_t x, uint64_t add) {
  uint64_t r, cdummy;
  asm("v_mad_u64_u32 %0, %1, %2, %3, %4" : "=v"(r), "=s"(cdummy) : "v"(x), "i"(C), "s"(add));
  return r;
}

// value = al + 2^32 ah (al, ah < 2^60)  ->  [0, 2^64), same residue.
// The dense MDS rows stay below 2^41; the sparse partial rounds hand in up to
// 2^58.2 (tests/test_poseidon_sparse.py computes the maxima from the tables).
__device__ __forceinline__ uint64_t reduce_row(uint64_t al, uint64_t ah) {
  uint64_t t, c1, c2;
  uint32_t e;
  // t = al + eps * hi32(ah)   (hi32(ah) < 2^28: t < 2^61, no overflow)
  asm("v_mad_u64_u32 %0, %1, %2, -1, %3" : "=v"(t), "=s"(c1) : "v"(hi32(ah)), "v"(al));
  // t.hi += lo32(ah), carry c2 (worth 2^64 = eps)
  uint32_t t0 = lo32(t), t1 = hi32(t);
  asm("v_add_co_u32_e64 %0, %1, %2, %3" : "=v"(t1), "=s"(c2) : "v"(t1), "v"(lo32(ah)));
  asm(QP_CWAIT "v_cndmask_b32_e64 %0, 0, -1, %1" : "=v"(e) : "s"(c2));
  // t + e: on a carry the new hi32(t) = old + lo32(ah) - 2^32 < old < 2^29, so
  // t < 2^61 and adding eps cannot overflow
  const uint64_t tt = ((uint64_t)t1 << 32) | t0;
  uint64_t r;
  asm("v_mad_u64_u32 %0, %1, %2, 1, %3" : "=v"(r), "=s"(c1) : "v"(e), "v"(tt));
  return r;
}

// value = al + 2^32 ah for any al < 2^64 and ah < 2^64 - 2^32  ->  [0, 2^64),
// same residue: the rows of a dense group's fourth step (al, ah up to 2^63.72,
// tests/test_poseidon_dense4.py computes the maxima from the tables).
// With ah = 2^32 hh + hl: value = lo32(al) + 2^32 (hi32(al) + hl) + 2^64 hh.
// The 33-bit sum hi32(al) + hl = s + 2^32 c2 hands its carry to the multiplier,
// h = hh + c2 <= 2^32 - 1 (hh <= 2^32 - 2), so value = base + 2^64 h with
// base = lo32(al) + 2^32 s < 2^64, and 2^64 = eps mod p: t = base + eps h with
// the mad's carry-out c1.  c2 and c1 can coincide (al = ah = 2^63.7 with
// hi32(al) + hl >= 2^32); c2 costs no correction of its own, it rides in h.
// Only c1 is corrected, by + eps: on c1 the kept word is base + eps h - 2^64
// <= (2^64 - 1) + (2^64 - 2^33 + 1) - 2^64 = 2^64 - 2^33, so adding eps stays
// below 2^64 - 2^32 and cannot wrap.
__device__ __forceinline__ uint64_t reduce_row_wide(uint64_t al, uint64_t ah) {
  uint32_t s1, h, e;
  uint64_t c2, c1, t, r;
  asm("v_add_co_u32_e64 %0, %1, %2, %3" : "=v"(s1), "=s"(c2) : "v"(hi32(al)), "v"(lo32(ah)));
  asm(QP_CWAIT "v_addc_co_u32_e64 %0, %1, %2, 0, %1" : "=v"(h), "+s"(c2) : "v"(hi32(ah)));
  const uint64_t base = ((uint64_t)s1 << 32) | lo32(al);
  asm("v_mad_u64_u32 %0, %1, %2, -1, %3" : "=v"(t), "=s"(c1) : "v"(h), "v"(base));
  asm(QP_CWAIT "v_cndmask_b32_e64 %0, 0, -1, %1" : "=v"(e) : "s"(c1));
  asm("v_mad_u64_u32 %0, %1, %2, 1, %3" : "=v"(r), "=s"(c1) : "v"(e), "v"(t));
  return r;
}

// C forms of the same (compiler-chosen carries)
__device__ __forceinline__ uint64_t reduce_row_c(uint64_t al, uint64_t ah) {
  const uint64_t t = al + (ah >> 32) * EPS;
  const uint32_t t1 = hi32(t) + lo32(ah);
  const uint64_t r = ((uint64_t)t1 << 32) | lo32(t);
  return t1 < lo32(ah) ? r + EPS : r;
}
__device__ __forceinline__ uint64_t sbox_c(uint64_t x) {
  const uint64_t x2 = mul_c(x, x);
  const uint64_t x3 = mul_c(x2, x);
  const uint64_t x4 = mul_c(x2, x2);
  return mul_c(x3, x4);
}

__device__ __forceinline__ uint64_t sbox(uint64_t x) {
  const uint64_t x2 = mul(x, x);
  const uint64_t x3 = mul(x2, x);
  const uint64_t x4 = mul(x2, x2);
  return mul(x3, x4);
}

// the 12 S-boxes of a full round
__device__ __forceinline__ void sbox12(uint64_t s[12]) {
#pragma unroll
  for (int i = 0; i < 12; i++) s[i] = sbox(s[i]);
}

// a + c, a in [0, 2^64), c < p
__device__ __forceinline__ uint64_t add_c(uint64_t a, uint64_t c) {
  const uint64_t s = a + c;
  return s + (s < c ? EPS : 0);
}

// terms I..11 of MDS row R, one mad per half and term
template <int R, int I>
__device__ __forceinline__ void row_terms(uint64_t &al, uint64_t &ah, const uint32_t lo[12], const uint32_t hi[12]) {
  if constexpr (I < 12) {
    constexpr int C = (int)ps::mds_circ(I) + ((R == 0 && I == 0) ? 8 : 0);
    al = mad_c<C>(lo[(I + R) % 12], al);
    ah = mad_c<C>(hi[(I + R) % 12], ah);
    row_terms<R, I + 1>(al, ah, lo, hi);
  }
}

// runtime-constant variant: s <- MDS(s) + k (k[12] wave-uniform, < p)
template <int R>
__device__ __forceinline__ void mds_rows_k(uint64_t s[12], const uint32_t lo[12], const uint32_t hi[12],
                                           const uint64_t k[12]) {
  if constexpr (R < 12) {
    constexpr int C0 = (int)ps::mds_circ(0) + (R == 0 ? 8 : 0);
    uint64_t al = mad_cs<C0>(lo[R], k[R] & EPS);
    uint64_t ah = mad_cs<C0>(hi[R], k[R] >> 32);
    row_terms<R, 1>(al, ah, lo, hi);
    s[R] = reduce_row(al, ah);
    mds_rows_k<R + 1>(s, lo, hi, k);
  }
}

__device__ __forceinline__ void mds_k(uint64_t s[12], const uint64_t k[12]) {
  uint32_t lo[12], hi[12];
#pragma unroll
  for (int i = 0; i < 12; i++) {
    lo[i] = lo32(s[i]);
    hi[i] = hi32(s[i]);
  }
  mds_rows_k<0>(s, lo, hi, k);
}

template <int R>
__device__ __forceinline__ void mds_rows_mads(uint64_t s[12], const uint32_t lo[12], const uint32_t hi[12]) {
  if constexpr (R < 12) {
    constexpr int C0 = (int)ps::mds_circ(0) + (R == 0 ? 8 : 0);
    uint64_t al = mad_c<C0>(lo[R], 0);
    uint64_t ah = mad_c<C0>(hi[R], 0);
    row_terms<R, 1>(al, ah, lo, hi);
    s[R] = reduce_row(al, ah);
    mds_rows_mads<R + 1>(s, lo, hi);
  }
}

// The per-mad MDS, s <- MDS(s) with no constant: every product its own asm
// statement, as in mds_k and capz_mds.  The quotient's Poseidon-gate rounds
// use it.
__device__ __forceinline__ void mds_mads(uint64_t s[12]) {
  uint32_t lo[12], hi[12];
#pragma unroll
  for (int i = 0; i < 12; i++) {
    lo[i] = lo32(s[i]);
    hi[i] = hi32(s[i]);
  }
  mds_rows_mads<0>(s, lo, hi);
}

// One MDS row as a single asm block: 24 v_mad_u64_u32 on the rotated halves
// (x[i] = half[(i+R)%12]) with the circulant constants inline, starting from
// the folded round-constant halves kl/kh.  Inside one asm statement the
// compiler's conservative inline-asm hazard padding (an s_nop after every
// SGPR-writing asm VALU op) disappears; the mads only write the dead carry
// SGPR pair and read none, so no wait state is needed between them.
#define QP_MDS_ROW_ASM(C0)                                                                                  \
  asm("v_mad_u64_u32 %0, %2, %3, " #C0 ", %27\n\t"                                                     \
      "v_mad_u64_u32 %1, %2, %15, " #C0 ", %28\n\t"                                                    \
      "v_mad_u64_u32 %0, %2, %4, 15, %0\n\t"                                                           \
      "v_mad_u64_u32 %1, %2, %16, 15, %1\n\t"                                                          \
      "v_mad_u64_u32 %0, %2, %5, 41, %0\n\t"                                                           \
      "v_mad_u64_u32 %1, %2, %17, 41, %1\n\t"                                                          \
      "v_mad_u64_u32 %0, %2, %6, 16, %0\n\t"                                                           \
      "v_mad_u64_u32 %1, %2, %18, 16, %1\n\t"                                                          \
      "v_mad_u64_u32 %0, %2, %7, 2, %0\n\t"                                                            \
      "v_mad_u64_u32 %1, %2, %19, 2, %1\n\t"                                                           \
      "v_mad_u64_u32 %0, %2, %8, 28, %0\n\t"                                                           \
      "v_mad_u64_u32 %1, %2, %20, 28, %1\n\t"                                                          \
      "v_mad_u64_u32 %0, %2, %9, 13, %0\n\t"                                                           \
      "v_mad_u64_u32 %1, %2, %21, 13, %1\n\t"                                                          \
      "v_mad_u64_u32 %0, %2, %10, 13, %0\n\t"                                                          \
      "v_mad_u64_u32 %1, %2, %22, 13, %1\n\t"                                                          \
      "v_mad_u64_u32 %0, %2, %11, 39, %0\n\t"                                                          \
      "v_mad_u64_u32 %1, %2, %23, 39, %1\n\t"                                                          \
      "v_mad_u64_u32 %0, %2, %12, 18, %0\n\t"                                                          \
      "v_mad_u64_u32 %1, %2, %24, 18, %1\n\t"                                                          \
      "v_mad_u64_u32 %0, %2, %13, 34, %0\n\t"                                                          \
      "v_mad_u64_u32 %1, %2, %25, 34, %1\n\t"                                                          \
      "v_mad_u64_u32 %0, %2, %14, 20, %0\n\t"                                                          \
      "v_mad_u64_u32 %1, %2, %26, 20, %1"                                                                \
      : "=&v"(al), "=&v"(ah), "=&s"(cd)                                                                  \
      : "v"(lo[(0 + R) % 12]), "v"(lo[(1 + R) % 12]), "v"(lo[(2 + R) % 12]), "v"(lo[(3 + R) % 12]),     \
        "v"(lo[(4 + R) % 12]), "v"(lo[(5 + R) % 12]), "v"(lo[(6 + R) % 12]), "v"(lo[(7 + R) % 12]),     \
        "v"(lo[(8 + R) % 12]), "v"(lo[(9 + R) % 12]), "v"(lo[(10 + R) % 12]), "v"(lo[(11 + R) % 12]),   \
        "v"(hi[(0 + R) % 12]), "v"(hi[(1 + R) % 12]), "v"(hi[(2 + R) % 12]), "v"(hi[(3 + R) % 12]),     \
        "v"(hi[(4 + R) % 12]), "v"(hi[(5 + R) % 12]), "v"(hi[(6 + R) % 12]), "v"(hi[(7 + R) % 12]),     \
        "v"(hi[(8 + R) % 12]), "v"(hi[(9 + R) % 12]), "v"(hi[(10 + R) % 12]), "v"(hi[(11 + R) % 12]),   \
        "s"(kl), "s"(kh))

template <int R>
__device__ __forceinline__ void mds_row_block(uint64_t &al, uint64_t &ah, const uint32_t lo[12],
                                              const uint32_t hi[12], uint64_t kl, uint64_t kh) {
  static_assert(ps::mds_circ(0) == 17 && ps::mds_circ(1) == 15 && ps::mds_circ(11) == 20, "MDS constants");
  uint64_t cd;
  if constexpr (R == 0) {
    QP_MDS_ROW_ASM(25);  // circulant 17 + diagonal 8
  } else {
    QP_MDS_ROW_ASM(17);
  }
  (void)cd;
}

template <int R, int RC, uint32_t OUT = 0xFFFu>
__device__ __forceinline__ void mds_rows_block(uint64_t s[12], const uint32_t lo[12], const uint32_t hi[12]) {
  if constexpr (R < 12) {
    if constexpr ((OUT >> R) & 1) {  // rows nobody reads (OUT) are skipped
      constexpr uint64_t k = RC >= 0 ? ps::rc_cx(RC * 12 + R) : 0;
      uint64_t al, ah;
      mds_row_block<R>(al, ah, lo, hi, k & EPS, k >> 32);
      s[R] = reduce_row(al, ah);
    }
    mds_rows_block<R + 1, RC, OUT>(s, lo, hi);
  }
}

// The row-block MDS, s <- MDS(s) + RC[NEXT] (NEXT < 0: no constant), each row
// one asm block; OUT: the output rows needed.  The hashing permutation uses it
// (2.35 against 2.24 Gperm/s for the per-mad form in isolation, e2e 932 -> 942
// proofs/s, profiles/r02_ab_poseidon_mode3.log).
template <int NEXT, uint32_t OUT = 0xFFFu>
__device__ __forceinline__ void mds_block(uint64_t s[12]) {
  uint32_t lo[12], hi[12];
#pragma unroll
  for (int i = 0; i < 12; i++) {
    lo[i] = lo32(s[i]);
    hi[i] = hi32(s[i]);
  }
  mds_rows_block<0, NEXT, OUT>(s, lo, hi);
}

// block-asm MDS with the next round's constants read at run time (uniform
// index: scalar loads into SGPRs) — the body of the rolled partial-round loop
template <int R>
__device__ __forceinline__ void mds_rows_block_dyn(uint64_t s[12], const uint32_t lo[12], const uint32_t hi[12],
                                                   const uint64_t *__restrict__ k) {
  if constexpr (R < 12) {
    const uint64_t kr = k[R];
    uint64_t al, ah;
    mds_row_block<R>(al, ah, lo, hi, kr & EPS, kr >> 32);
    s[R] = reduce_row(al, ah);
    mds_rows_block_dyn<R + 1>(s, lo, hi, k);
  }
}

// one full round (12 S-boxes + MDS folding the next round's constants, read at
// run time) — the body of the witness kernel's rolled full-round loops
__device__ __forceinline__ void full_round_dyn(uint64_t s[12], const uint64_t *__restrict__ knext) {
#pragma unroll
  for (int i = 0; i < 12; i++) s[i] = sbox(s[i]);
  uint32_t lo[12], hi[12];
#pragma unroll
  for (int i = 0; i < 12; i++) {
    lo[i] = lo32(s[i]);
    hi[i] = hi32(s[i]);
  }
  mds_rows_block_dyn<0>(s, lo, hi, knext);
}

// ---- sparse partial rounds (tools/gen_poseidon_partial.py): round 3's MDS
// merged with D_4 (rows 1..11 dense), then per partial round one S-box, one
// dot product for lane 0 and 11 scalar multiply-adds.  Dense constants act on
// 22-bit limbs (x = l0 + 2^22 l1 + 2^44 l2) through precomputed c 2^(22k) mod
// p halves, so every accumulator stays < 2^60 and reduces in 4 instructions.
// Same permutation as the plain rounds.  The quotient's Poseidon gate runs its
// partial rounds this way (its wire checks hook each round's S-box input); the
// hashing permutation runs dense_group below.

__device__ __forceinline__ void limbs22(uint64_t x, uint32_t l[3]) {
  const uint32_t lo = lo32(x), hi = hi32(x);
  l[0] = lo & 0x3FFFFFu;
  l[1] = __builtin_amdgcn_alignbit(hi, lo, 22) & 0x3FFFFFu;
  l[2] = hi >> 12;
}

// the generated tables as compile-time values (every product below has a
// literal constant operand; zero halves emit nothing)
enum { PT_INIT, PT_AHAT, PT_BV, PT_S0C, PT_GAM };
template <int TB, int OFF>
__device__ __forceinline__ constexpr uint32_t ptab() {
  return TB == PT_INIT ? pfp::INIT[OFF] : TB == PT_AHAT ? pfp::AHAT[OFF] : TB == PT_BV ? pfp::BV[OFF]
       : TB == PT_GAM ? pfp::GAM[OFF] : pfp::S0C[OFF];
}

// al/ah += sum_k l[k] * (halves of the constant at table TB, words OFF..OFF+5)
template <int TB, int OFF, int K = 0>
__device__ __forceinline__ void mac_limbs(uint64_t &al, uint64_t &ah, const uint32_t l[3]) {
  if constexpr (K < 3) {
    constexpr uint32_t cl = ptab<TB, OFF + 2 * K>(), ch = ptab<TB, OFF + 2 * K + 1>();
    // explicit mads with the (dead) carry-out sunk into VCC: as C the compiler
    // hands the carry the SGPR pair holding the constant, and the next
    // constant's s_mov into it then costs a hazard s_nop per product
    if constexpr (cl != 0) asm("v_mad_u64_u32 %0, vcc, %1, %2, %0" : "+v"(al) : "v"(l[K]), "s"(cl) : "vcc");
    if constexpr (ch != 0) asm("v_mad_u64_u32 %0, vcc, %1, %2, %0" : "+v"(ah) : "v"(l[K]), "s"(ch) : "vcc");
    mac_limbs<TB, OFF, K + 1>(al, ah, l);
  }
}

// row I (1..11) of D_4 M over the limbs of all 12 lanes
template <int I, int J = 0>
__device__ __forceinline__ void init_row(uint64_t &al, uint64_t &ah, const uint32_t L[12][3]) {
  if constexpr (J < 12) {
    mac_limbs<PT_INIT, ((I - 1) * 12 + J) * 6>(al, ah, L[J]);
    init_row<I, J + 1>(al, ah, L);
  }
}
template <int I = 1>
__device__ __forceinline__ void init_rows(uint64_t out[12], const uint32_t L[12][3]) {
  if constexpr (I < 12) {
    uint64_t al = pfp::INIT_K[2 * I], ah = pfp::INIT_K[2 * I + 1];
    init_row<I>(al, ah, L);
    out[I] = reduce_row(al, ah);
    init_rows<I + 1>(out, L);
  }
}

// s <- D_4 M s + D_4 c_4  (s = the S-box outputs of round 3)
__device__ __forceinline__ void mds_init_sparse(uint64_t s[12]) {
  uint32_t lo[12], hi[12], L[12][3];
#pragma unroll
  for (int j = 0; j < 12; j++) {
    lo[j] = lo32(s[j]);
    hi[j] = hi32(s[j]);
    limbs22(s[j], L[j]);
  }
  uint64_t out[12];
  {
    uint64_t al, ah;
    mds_row_block<0>(al, ah, lo, hi, pfp::INIT_K[0], pfp::INIT_K[1]);
    out[0] = reduce_row(al, ah);
  }
  init_rows(out, L);
#pragma unroll
  for (int i = 0; i < 12; i++) s[i] = out[i];
}

// lane-0 dot product on the 32-bit halves of lanes 1..11 (AH2 pieces of
// weights 1, 2^22, 2^44; each accumulator < 2^59)
template <int T, int J = 1, int H = 0, int K = 0>
__device__ __forceinline__ void sparse_row0_h(uint64_t S[3], const uint64_t s[12]) {
  if constexpr (J < 12) {
    constexpr uint32_t c = pfp::AH2[((T * 11 + J - 1) * 2 + H) * 3 + K];
    const uint32_t v = H ? hi32(s[J]) : lo32(s[J]);
    if constexpr (c != 0) asm("v_mad_u64_u32 %0, vcc, %1, %2, %0" : "+v"(S[K]) : "v"(v), "s"(c) : "vcc");
    if constexpr (K < 2) sparse_row0_h<T, J, H, K + 1>(S, s);
    else if constexpr (H == 0) sparse_row0_h<T, J, 1, 0>(S, s);
    else sparse_row0_h<T, J + 1, 0, 0>(S, s);
  }
}

// r - y for y < 2^40: a borrow means r - y + 2^64 (>= 2^64 - 2^40) was kept,
// so subtracting eps = 2^64 mod p cannot borrow again
__device__ __forceinline__ uint64_t sub_small(uint64_t r, uint32_t y0, uint32_t y1) {
  uint32_t r0 = lo32(r), r1 = hi32(r), e;
  uint64_t c;
  asm("v_sub_co_u32_e64 %0, %1, %2, %3" : "=v"(r0), "=s"(c) : "v"(r0), "v"(y0));
  asm(QP_CWAIT "v_subb_co_u32_e64 %0, %1, %2, %3, %4" : "=v"(r1), "=s"(c) : "v"(r1), "v"(y1), "s"(c));
  asm(QP_CWAIT "v_cndmask_b32_e64 %0, 0, -1, %1" : "=v"(e) : "s"(c));
  asm("v_sub_co_u32_e64 %0, %1, %2, %3" : "=v"(r0), "=s"(c) : "v"(r0), "v"(e));
  asm(QP_CWAIT "v_subb_co_u32_e64 %0, %1, %2, 0, %3" : "=v"(r1), "=s"(c) : "v"(r1), "s"(c));
  return ((uint64_t)r1 << 32) | r0;
}

// ---- groups of G partial rounds (tools/gen_poseidon_partial.py
// permute_fast_grouped): lanes 1..11 only change by b_i x0 per round, so their
// updates are deferred to the end of the group (one reduction per lane per
// group instead of per round); round t's lane-0 dot then reads the group-start
// lanes and adds gamma[t][l] x_l for the group's earlier S-box outputs x_l.
constexpr int PF_GROUP = 4;  // partial rounds per group (profiles/r02_ab_poseidon_group4.log)
struct NoHook {
  __device__ __forceinline__ uint64_t operator()(int, uint64_t v) const { return v; }
};

template <int T0, int M, int L = 0>
__device__ __forceinline__ void group_gammas(uint64_t &al, uint64_t &ah, const uint32_t (*l)[3]) {
  if constexpr (L < M) {
    mac_limbs<PT_GAM, ((T0 + M) * 22 + T0 + L) * 6>(al, ah, l[L]);
    group_gammas<T0, M, L + 1>(al, ah, l);
  }
}

template <int T0, int G, int M = 0, class HK>
__device__ __forceinline__ void group_lane0(const uint64_t s[12], uint64_t &s0, uint32_t (*l)[3], const HK &hook) {
  if constexpr (M < G) {
    constexpr int T = T0 + M;
    const uint64_t x = sbox(hook(T, s0));
    limbs22(x, l[M]);
    constexpr uint32_t kl = pfp::K0[2 * T], kh = pfp::K0[2 * T + 1];
    uint64_t S[3];
    asm("v_mad_u64_u32 %0, vcc, %1, 25, %2" : "=v"(S[0]) : "v"(lo32(x)), "s"((uint64_t)kl) : "vcc");
    S[1] = (uint64_t)hi32(x) * 25600u;
    S[2] = 0;
    sparse_row0_h<T>(S, s);
    uint64_t al = S[0] + (uint64_t)lo32(S[1]) * (1u << 22);
    uint64_t ah = (uint64_t)kh + (uint64_t)hi32(S[1]) * (1u << 22);
    ah += (uint64_t)lo32(S[2]) * (1u << 12);
    ah += (uint64_t)hi32(S[2]) * (1u << 12);
    group_gammas<T0, M>(al, ah, l);
    s0 = sub_small(reduce_row(al, ah), hi32(S[2]) << 12, hi32(S[2]) >> 20);
    group_lane0<T0, G, M + 1>(s, s0, l, hook);
  }
}

template <int T0, int G, int I, int M>
__device__ __forceinline__ void group_col_macs(uint64_t &bl, uint64_t &bh, const uint32_t (*l)[3]) {
  if constexpr (M < G) {
    mac_limbs<PT_BV, ((T0 + M) * 11 + I - 1) * 6>(bl, bh, l[M]);
    group_col_macs<T0, G, I, M + 1>(bl, bh, l);
  }
}

template <int T0, int G, int I = 1>
__device__ __forceinline__ void group_cols(uint64_t s[12], const uint32_t (*l)[3]) {
  if constexpr (I < 12) {
    constexpr bool last = T0 + G == 22;
    uint64_t bl = (uint64_t)lo32(s[I]) + (last ? pfp::KLAST[2 * I] : 0u);
    uint64_t bh = (uint64_t)hi32(s[I]) + (last ? pfp::KLAST[2 * I + 1] : 0u);
    group_col_macs<T0, G, I, 0>(bl, bh, l);
    s[I] = reduce_row(bl, bh);
    group_cols<T0, G, I + 1>(s, l);
  }
}

template <int T0, int G, class HK = NoHook>
__device__ __forceinline__ void partial_group(uint64_t s[12], const HK &hook = HK{}) {
  uint32_t l[G][3];
  uint64_t s0 = s[0];
  group_lane0<T0, G>(s, s0, l, hook);
  group_cols<T0, G>(s, l);
  s[0] = s0;
}

// ---- dense groups of G <= 4 partial rounds (tools/gen_poseidon_dense.py): a
// partial round is v <- M (Z v + e_0 v_0^7) + c with Z zeroing lane 0, so G of
// them are rows of (MZ)^m over the group-start lanes 1..11 plus columns
// (MZ)^k M e_0 for the group's S-box outputs x_l, all exact small integers.
// Every term is one mad per 32-bit half, as in the dense MDS rows, where the
// sparse form pays six for a full-width constant.  For m <= 3 the entries are
// below 2^22 and the row sums below 2^23.85: al, ah stay below 2^56
// (tests/test_poseidon_dense.py) and reduce with reduce_row.  For m = 4 the
// entries reach 2^28.3 and the row sums 2^31.72: al, ah reach 2^63.72
// (tests/test_poseidon_dense4.py) and reduce with reduce_row_wide.  The
// hashing permutation runs the partial rounds in the groups of pfd4 (4,4,4,4,
// 3,3: 2 524 mads, 88 reduced rows); the pfd tables (3,3,3,3,3,3,2,2: 2 988,
// 110) stay for the probe.

// the generated tables of a plan as compile-time values
struct TabG3 {
  static constexpr int GMAX = 3;
  static constexpr int glen(int t) { return pfd::GLEN[t]; }
  static constexpr uint32_t pow(int i) { return pfd::POW[i]; }
  static constexpr uint32_t col(int i) { return pfd::COL[i]; }
  static constexpr uint32_t k(int i) { return pfd::K[i]; }
};
struct TabG4 {
  static constexpr int GMAX = 4;
  static constexpr int glen(int t) { return pfd4::GLEN[t]; }
  static constexpr uint32_t pow(int i) { return pfd4::POW[i]; }
  static constexpr uint32_t col(int i) { return pfd4::COL[i]; }
  static constexpr uint32_t k(int i) { return pfd4::K[i]; }
};

// Row I of step M sums to rs over the integers, so with the constant's half
// each accumulator is at most (rs + 1)(2^32 - 1): past reduce_row's 2^60 the
// row reduces wide (the generator's row_is_wide)
template <class TB, int M, int I>
constexpr bool dg_wide() {
  uint64_t rs = 0;
  for (int j = 0; j < 11; j++) rs += TB::pow(((M - 1) * 12 + I) * 11 + j);
  for (int l = 0; l < M; l++) rs += TB::col(l * 12 + I);
  return (rs + 1) * 0xFFFFFFFFull >= (1ull << 60);
}

// al += lo * C, ah += hi * C: one constant for the pair of mads (inline up to
// 64, else an SGPR), the dead carry-outs sunk into VCC as in mac_limbs
template <uint32_t C>
__device__ __forceinline__ void mac_pair(uint64_t &al, uint64_t &ah, uint32_t lo, uint32_t hi) {
  static_assert(C != 0, "the integer rows have no zero entry");
  if constexpr (C <= 64)
    asm("v_mad_u64_u32 %0, vcc, %2, %4, %0\n\tv_mad_u64_u32 %1, vcc, %3, %4, %1"
        : "+v"(al), "+v"(ah) : "v"(lo), "v"(hi), "i"(C) : "vcc");
  else
    asm("v_mad_u64_u32 %0, vcc, %2, %4, %0\n\tv_mad_u64_u32 %1, vcc, %3, %4, %1"
        : "+v"(al), "+v"(ah) : "v"(lo), "v"(hi), "s"(C) : "vcc");
}

// row I of step M (1..G) of the group starting at partial round T0:
//   K[T0+M-1][I] + sum_(l<M) COL[M-1-l][I] x_l + sum_(j=1..11) POW[M][I][j] v_j
// The newest x's column is M's column 0 (inline constants): its pair of mads
// opens the row with the halves of K as addends (an SGPR addend leaves the
// constant bus no room for an SGPR factor).
template <class TB, int M, int I, int J = 1>
__device__ __forceinline__ void dg_lane_terms(uint64_t &al, uint64_t &ah, const uint32_t lo[12], const uint32_t hi[12]) {
  if constexpr (J < 12) {
    mac_pair<TB::pow(((M - 1) * 12 + I) * 11 + J - 1)>(al, ah, lo[J], hi[J]);
    dg_lane_terms<TB, M, I, J + 1>(al, ah, lo, hi);
  }
}
template <class TB, int M, int I, int L>
__device__ __forceinline__ void dg_x_terms(uint64_t &al, uint64_t &ah, const uint32_t *xl, const uint32_t *xh) {
  if constexpr (L >= 0) {
    mac_pair<TB::col((M - 1 - L) * 12 + I)>(al, ah, xl[L], xh[L]);
    dg_x_terms<TB, M, I, L - 1>(al, ah, xl, xh);
  }
}
template <class TB, int T0, int M, int I>
__device__ __forceinline__ uint64_t dg_row(const uint32_t lo[12], const uint32_t hi[12], const uint32_t *xl,
                                           const uint32_t *xh) {
  constexpr uint32_t C0 = TB::col(I);
  static_assert(C0 <= 64, "M's column 0 is inline");
  constexpr uint64_t kl = TB::k(((T0 + M - 1) * 12 + I) * 2), kh = TB::k(((T0 + M - 1) * 12 + I) * 2 + 1);
  uint64_t al, ah;
  asm("v_mad_u64_u32 %0, vcc, %2, %4, %5\n\tv_mad_u64_u32 %1, vcc, %3, %4, %6"
      : "=&v"(al), "=&v"(ah) : "v"(xl[M - 1]), "v"(xh[M - 1]), "i"(C0), "s"(kl), "s"(kh) : "vcc");
  dg_x_terms<TB, M, I, M - 2>(al, ah, xl, xh);
  dg_lane_terms<TB, M, I>(al, ah, lo, hi);
  if constexpr (dg_wide<TB, M, I>()) return reduce_row_wide(al, ah);
  else return reduce_row(al, ah);
}

// x_0 = v_0^7, then y_M (row 0 of step M) and x_M = y_M^7 for M = 1..G-1
template <class TB, int T0, int G, int M = 1>
__device__ __forceinline__ void dg_lane0(const uint32_t lo[12], const uint32_t hi[12], uint32_t *xl, uint32_t *xh) {
  if constexpr (M < G) {
    const uint64_t x = sbox(dg_row<TB, T0, M, 0>(lo, hi, xl, xh));
    xl[M] = lo32(x);
    xh[M] = hi32(x);
    dg_lane0<TB, T0, G, M + 1>(lo, hi, xl, xh);
  }
}
template <class TB, int T0, int G, int I = 0>
__device__ __forceinline__ void dg_out(uint64_t s[12], const uint32_t lo[12], const uint32_t hi[12], const uint32_t *xl,
                                       const uint32_t *xh) {
  if constexpr (I < 12) {
    s[I] = dg_row<TB, T0, G, I>(lo, hi, xl, xh);
    dg_out<TB, T0, G, I + 1>(s, lo, hi, xl, xh);
  }
}

// partial rounds T0..T0+G-1 on the state entering round 4 + T0 (its constants
// added); leaves the state entering round 4 + T0 + G.  TB: the tables whose
// constants K were pushed through this group (T0 a group start of TB's plan)
template <int T0, int G, class TB = TabG3>
__device__ __forceinline__ void dense_group(uint64_t s[12]) {
  static_assert(G >= 1 && G <= 4 && G <= TB::GMAX && T0 >= 0 && T0 + G <= 22, "the tables hold (MZ)^1..GMAX");
  uint32_t lo[12], hi[12], xl[G], xh[G];
#pragma unroll
  for (int j = 1; j < 12; j++) {
    lo[j] = lo32(s[j]);
    hi[j] = hi32(s[j]);
  }
  const uint64_t x0 = sbox(s[0]);
  xl[0] = lo32(x0);
  xh[0] = hi32(x0);
  dg_lane0<TB, T0, G>(lo, hi, xl, xh);
  dg_out<TB, T0, G>(s, lo, hi, xl, xh);
}

// rounds R..29.  OUT: bit mask of the output lanes the caller reads (the last
// MDS computes only those rows; digests need lanes 0..3, the PoW lane 7)
template <int R, uint32_t OUT = 0xFFFu>
__device__ __forceinline__ void rounds(uint64_t s[12]) {
  if constexpr (R >= 4 && R < 26) {
    // the partial rounds, in the groups of pfd4::GLEN
    constexpr int T0 = R - 4, G = pfd4::GLEN[T0];
    static_assert(G > 0, "partial rounds are entered at a group start");
    dense_group<T0, G, TabG4>(s);
    rounds<R + G, OUT>(s);
  } else if constexpr (R < 30) {
    sbox12(s);
    if constexpr (R == 29) mds_block<-1, OUT>(s);
    else mds_block<R + 1>(s);
    rounds<R + 1, OUT>(s);
  }
}

// round 0 of a state whose lanes 8..11 enter as zero (two_to_one, the first
// absorption of a sponge): their S-box outputs are constants, so only lanes
// 0..7 are S-boxed and each MDS row takes 16 mads on them, starting from the
// folded constant CAPZ_K[r] = RC[1][r] + sum_(j>=8) M[r][j] sbox(RC[0][j])
template <int R, int I = 0>
__device__ __forceinline__ void capz_row_terms(uint64_t &al, uint64_t &ah, const uint32_t lo[12], const uint32_t hi[12]) {
  if constexpr (I < 12) {
    constexpr int J = (I + R) % 12;
    if constexpr (J < 8) {
      constexpr int C = (int)ps::mds_circ(I) + ((R == 0 && I == 0) ? 8 : 0);
      al = mad_c<C>(lo[J], al);
      ah = mad_c<C>(hi[J], ah);
    }
    capz_row_terms<R, I + 1>(al, ah, lo, hi);
  }
}
template <int R = 0>
__device__ __forceinline__ void capz_mds(uint64_t s[12], const uint32_t lo[12], const uint32_t hi[12]) {
  if constexpr (R < 12) {
    uint64_t al = pfp::CAPZ_K[2 * R], ah = pfp::CAPZ_K[2 * R + 1];
    capz_row_terms<R>(al, ah, lo, hi);
    s[R] = reduce_row(al, ah);
    capz_mds<R + 1>(s, lo, hi);
  }
}

// permute_nc for s[8..11] == 0 on entry, reading only lanes OUT
// (profiles/r02_ab_capz.log)
template <uint32_t OUT = 0xFFFu>
__device__ __forceinline__ void permute_nc_capz(uint64_t s[12]) {
  uint32_t lo[12], hi[12];
#pragma unroll
  for (int i = 0; i < 8; i++) {
    s[i] = sbox(add_c(s[i], ps::rc_cx(i)));
    lo[i] = lo32(s[i]);
    hi[i] = hi32(s[i]);
  }
  capz_mds(s, lo, hi);
  rounds<1, OUT>(s);
}

// permutation; inputs in [0, 2^64), outputs in [0, 2^64) (canon() lanes read out)
__device__ __forceinline__ void permute_nc(uint64_t s[12]) {
#pragma unroll
  for (int i = 0; i < 12; i++) s[i] = add_c(s[i], ps::rc_cx(i));
  rounds<0>(s);
}

__device__ __forceinline__ void permute(uint64_t s[12]) {
  permute_nc(s);
#pragma unroll
  for (int i = 0; i < 12; i++) s[i] = canon(s[i]);
}

}  // namespace pf
