// field_nc.h — Goldilocks arithmetic for the throughput kernels, in the
// non-canonical representation [0, 2^64) (plonky2's own GoldilocksField
// representation; canonicalise with canon() before values leave a kernel).
// The one home of that arithmetic: the NTT core (ntt16.h, nt::) and the
// Poseidon permutation (poseidon_fast.h, pf::) are built on it and take its
// names with using declarations; it includes neither.
//
// gfx950 runs 64-bit VALU ops (v_lshl_add_u64, v_cmp_*_u64, 64-bit shifts,
// v_mad_u64_u32) at a fraction of the 32-bit rate (PMC: SQ_INSTS_VALU_INT64),
// so everything except the 32x32->64 partial products is written as 32-bit
// carry chains (v_add_co/v_addc/v_sub_co/v_subb), by the compiler (add, sub,
// reduce) or as inline asm whose carries come straight from the mad/sub
// carry-outs (mul, mulk, Acc3).
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>
#include "field.h"

// Hazard rule (gfx950): a VALU instruction reading a carry/mask SGPR written
// by the previous VALU instruction needs 2 wait states (hipcc puts s_nop 1
// between its own v_add_co/v_addc pairs).  Around inline asm hipcc adds only a
// fixed 1-state pad, so every asm statement that reads a carry written by the
// preceding one opens with its own s_nop 0.
// (Dropping it measured no faster, profiles/r02_ab_carry_wait.log.)
#define QP_CWAIT "s_nop 0\n\t"

namespace gfn {

using gl::P;
using gl::EPS;  // 2^64 mod p

__device__ __forceinline__ uint32_t lo32(uint64_t x) { return (uint32_t)x; }
__device__ __forceinline__ uint32_t hi32(uint64_t x) { return (uint32_t)(x >> 32); }
__device__ __forceinline__ uint64_t pack(uint32_t lo, uint32_t hi) { return ((uint64_t)hi << 32) | lo; }

__device__ __forceinline__ uint64_t canon(uint64_t x) { return x >= P ? x - P : x; }

// a + b, any a, b in [0, 2^64)
__device__ __forceinline__ uint64_t add(uint64_t a, uint64_t b) {
  uint32_t c0, c1, c2, c3, c4;
  uint32_t lo = __builtin_addc((uint32_t)a, (uint32_t)b, 0u, &c0);
  uint32_t hi = __builtin_addc((uint32_t)(a >> 32), (uint32_t)(b >> 32), c0, &c1);
  lo = __builtin_addc(lo, 0u - c1, 0u, &c2);  // wrapped: + eps
  hi = __builtin_addc(hi, 0u, c2, &c3);
  lo = __builtin_addc(lo, 0u - c3, 0u, &c4);  // wrapped again (both inputs > p): + eps
  hi += c4;
  return pack(lo, hi);
}

// a + b with b < p: the second wrap cannot happen
__device__ __forceinline__ uint64_t add_c(uint64_t a, uint64_t b) {
  uint32_t c0, c1, c2, c3;
  uint32_t lo = __builtin_addc((uint32_t)a, (uint32_t)b, 0u, &c0);
  uint32_t hi = __builtin_addc((uint32_t)(a >> 32), (uint32_t)(b >> 32), c0, &c1);
  lo = __builtin_addc(lo, 0u - c1, 0u, &c2);
  hi = __builtin_addc(hi, 0u, c2, &c3);
  return pack(lo, hi);
}

// a - b, any a, b in [0, 2^64)
__device__ __forceinline__ uint64_t sub(uint64_t a, uint64_t b) {
  uint32_t b0, b1, b2, b3, b4;
  uint32_t lo = __builtin_subc((uint32_t)a, (uint32_t)b, 0u, &b0);
  uint32_t hi = __builtin_subc((uint32_t)(a >> 32), (uint32_t)(b >> 32), b0, &b1);
  lo = __builtin_subc(lo, 0u - b1, 0u, &b2);  // wrapped below 0: - eps
  hi = __builtin_subc(hi, 0u, b2, &b3);
  lo = __builtin_subc(lo, 0u - b3, 0u, &b4);  // wrapped again (b - a > p): - eps
  hi -= b4;
  return pack(lo, hi);
}

// lo + 2^64 hi -> [0, 2^64)
__device__ __forceinline__ uint64_t reduce(uint64_t lo, uint64_t hi) {
  const uint32_t hl = (uint32_t)hi, hh = (uint32_t)(hi >> 32);
  uint32_t l0 = (uint32_t)lo, l1 = (uint32_t)(lo >> 32), c, bo, bo2;
  l0 = __builtin_subc(l0, hh, 0u, &bo);  // lo - hh; borrow: - eps (= + 1 - 2^32)
  l1 = __builtin_subc(l1, 0u, bo, &bo2);
  l0 = __builtin_addc(l0, bo2, 0u, &c);
  l1 = l1 - bo2 + c;
  const uint32_t t0 = __builtin_subc(0u, hl, 0u, &bo);  // hl * eps = (hl << 32) - hl
  const uint32_t t1 = hl - bo;
  l0 = __builtin_addc(l0, t0, 0u, &c);
  l1 = __builtin_addc(l1, t1, c, &c);
  l0 = __builtin_addc(l0, 0u - c, 0u, &bo);  // carry out: + eps
  l1 = l1 + bo;
  return pack(l0, l1);
}

// a * b mod p, a, b in [0, 2^64), result in [0, 2^64): 5 mads and an
// 8-instruction reduction
__device__ __forceinline__ uint64_t mul(uint64_t a, uint64_t b) {
  const uint32_t a0 = lo32(a), a1 = hi32(a), b0 = lo32(b), b1 = hi32(b);
  // middle column as one 65-bit sum: T = a0 b1 + L.hi, U = a1 b0 + T with its
  // carry-out c (worth 2^96), W = a1 b1 + (U.hi | c << 32): one zero-extension
  // and no separate 64-bit add (the textbook four-product form, mul_c below,
  // needs three and a v_lshl_add_u64; profiles/r02_ab_mul_form_dot_halves.log)
  const uint64_t L = (uint64_t)a0 * b0;
  const uint64_t T = (uint64_t)a0 * b1 + hi32(L);
  uint64_t U, cu;
  uint32_t ce;
  asm("v_mad_u64_u32 %0, %1, %2, %3, %4" : "=v"(U), "=s"(cu) : "v"(a1), "v"(b0), "v"(T));
  asm(QP_CWAIT "v_cndmask_b32_e64 %0, 0, 1, %1" : "=v"(ce) : "s"(cu));
  const uint64_t W = (uint64_t)a1 * b1 + (((uint64_t)ce << 32) | hi32(U));  // < 2^64 (high half)
  const uint64_t X = ((uint64_t)lo32(U) << 32) | lo32(L);
  // 128-bit product = X + 2^64 W, X = (L0, U0);  ≡ X + eps*w2 - w3
  uint64_t t, c1, c2, c3;
  uint32_t e;
  asm("v_mad_u64_u32 %0, %1, %2, -1, %3" : "=v"(t), "=s"(c1) : "v"(lo32(W)), "v"(X));
  asm(QP_CWAIT "v_cndmask_b32_e64 %0, 0, -1, %1" : "=v"(e) : "s"(c1));
  // carry: true value t + 2^64 ≡ t + eps; t < 2^64 - 2^33 then, no overflow
  asm("v_mad_u64_u32 %0, %1, %2, 1, %3" : "=v"(t), "=s"(c2) : "v"(e), "v"(t));
  // t - w3, borrow b (worth -2^64 ≡ -eps)
  uint32_t r0 = lo32(t), r1 = hi32(t);
  asm("v_sub_co_u32_e64 %0, %1, %2, %3" : "=v"(r0), "=s"(c3) : "v"(r0), "v"(hi32(W)));
  asm(QP_CWAIT "v_subb_co_u32_e64 %0, %1, %2, 0, %3" : "=v"(r1), "=s"(c3) : "v"(r1), "s"(c3));
  asm(QP_CWAIT "v_cndmask_b32_e64 %0, 0, -1, %1" : "=v"(e) : "s"(c3));
  // borrow: t - w3 + 2^64 >= 2^64 - 2^32, minus eps stays >= 0
  asm("v_sub_co_u32_e64 %0, %1, %2, %3" : "=v"(r0), "=s"(c3) : "v"(r0), "v"(e));
  asm(QP_CWAIT "v_subb_co_u32_e64 %0, %1, %2, 0, %3" : "=v"(r1), "=s"(c3) : "v"(r1), "s"(c3));
  return ((uint64_t)r1 << 32) | r0;
}

// C form of the same (compiler-chosen carries)
__device__ __forceinline__ uint64_t mul_c(uint64_t a, uint64_t b) {
  const uint32_t a0 = lo32(a), a1 = hi32(a), b0 = lo32(b), b1 = hi32(b);
  const uint64_t L = (uint64_t)a0 * b0;
  const uint64_t T = (uint64_t)a0 * b1 + hi32(L);
  const uint64_t U = (uint64_t)a1 * b0 + lo32(T);
  const uint64_t V = (uint64_t)a1 * b1 + hi32(T);
  const uint64_t W = V + hi32(U);
  const uint64_t X = ((uint64_t)lo32(U) << 32) | lo32(L);
  uint64_t t = X + (uint64_t)lo32(W) * EPS;
  t = t < X ? t + EPS : t;
  const uint64_t w3 = hi32(W);
  const uint64_t r = t - w3;
  return t < w3 ? r - EPS : r;
}

// ---- K independent products with their carry steps interleaved (K = 2, 3):
// each asm statement below issues one step of every product, so a carry SGPR
// written by product i's instruction is read K - 1 instructions (plus the
// compiler's one-state pad after an asm statement) later — the gfx950 carry
// hazard's two wait states are met by the other products' work instead of
// s_nop (one product alone needs ~14 pad states).  Same arithmetic as mul():
// U = a1 b0 + T with carry, W = a1 b1 + (U.hi | c << 32), X = (U.lo, L.lo),
// then the 8-step reduction.  The NTT passes use it (nt::mul_rows); in the
// Poseidon S-boxes it measured slower (leaf hash +4 %, e2e -2 %,
// profiles/r02_ab_mulk.log): at 7 waves/SIMD the pads it removes (8.0k -> 2.9k
// s_nop per permutation) were nearly free and it adds ~500 register-pair
// moves, so the S-boxes keep one product at a time.
#define QP_W2 QP_CWAIT  // K = 2: one explicit wait state before each carry read
template <int K>
__device__ __forceinline__ void mulk(const uint64_t *a, const uint64_t *b, uint64_t *r) {
  static_assert(K == 2 || K == 3, "K");
  uint64_t T[K], U[K], W[K], X[K], t[K], cs[K];
  uint32_t ce[K], e[K], r0[K], r1[K];
#pragma unroll
  for (int i = 0; i < K; i++) {
    const uint64_t L = (uint64_t)lo32(a[i]) * lo32(b[i]);
    T[i] = (uint64_t)lo32(a[i]) * hi32(b[i]) + hi32(L);
    X[i] = lo32(L);
  }
  if constexpr (K == 3) {
    asm("v_mad_u64_u32 %0, %3, %6, %9, %12\n\t"
        "v_mad_u64_u32 %1, %4, %7, %10, %13\n\t"
        "v_mad_u64_u32 %2, %5, %8, %11, %14"
        : "=&v"(U[0]), "=&v"(U[1]), "=&v"(U[2]), "=&s"(cs[0]), "=&s"(cs[1]), "=&s"(cs[2])
        : "v"(hi32(a[0])), "v"(hi32(a[1])), "v"(hi32(a[2])), "v"(lo32(b[0])), "v"(lo32(b[1])), "v"(lo32(b[2])),
          "v"(T[0]), "v"(T[1]), "v"(T[2]));
    asm("v_cndmask_b32_e64 %0, 0, 1, %3\n\t"
        "v_cndmask_b32_e64 %1, 0, 1, %4\n\t"
        "v_cndmask_b32_e64 %2, 0, 1, %5"
        : "=v"(ce[0]), "=v"(ce[1]), "=v"(ce[2]) : "s"(cs[0]), "s"(cs[1]), "s"(cs[2]));
  } else {
    asm("v_mad_u64_u32 %0, %2, %4, %6, %8\n\t"
        "v_mad_u64_u32 %1, %3, %5, %7, %9"
        : "=&v"(U[0]), "=&v"(U[1]), "=&s"(cs[0]), "=&s"(cs[1])
        : "v"(hi32(a[0])), "v"(hi32(a[1])), "v"(lo32(b[0])), "v"(lo32(b[1])), "v"(T[0]), "v"(T[1]));
    asm(QP_W2 "v_cndmask_b32_e64 %0, 0, 1, %2\n\t"
        "v_cndmask_b32_e64 %1, 0, 1, %3"
        : "=v"(ce[0]), "=v"(ce[1]) : "s"(cs[0]), "s"(cs[1]));
  }
#pragma unroll
  for (int i = 0; i < K; i++) {
    W[i] = (uint64_t)hi32(a[i]) * hi32(b[i]) + (((uint64_t)ce[i] << 32) | hi32(U[i]));
    X[i] |= (uint64_t)lo32(U[i]) << 32;
  }
  if constexpr (K == 3) {
    // t = X + eps w2 (carry c1); e = c1 ? eps : 0; t += e
    asm("v_mad_u64_u32 %0, %3, %6, -1, %9\n\t"
        "v_mad_u64_u32 %1, %4, %7, -1, %10\n\t"
        "v_mad_u64_u32 %2, %5, %8, -1, %11"
        : "=&v"(t[0]), "=&v"(t[1]), "=&v"(t[2]), "=&s"(cs[0]), "=&s"(cs[1]), "=&s"(cs[2])
        : "v"(lo32(W[0])), "v"(lo32(W[1])), "v"(lo32(W[2])), "v"(X[0]), "v"(X[1]), "v"(X[2]));
    asm("v_cndmask_b32_e64 %0, 0, -1, %3\n\t"
        "v_cndmask_b32_e64 %1, 0, -1, %4\n\t"
        "v_cndmask_b32_e64 %2, 0, -1, %5"
        : "=v"(e[0]), "=v"(e[1]), "=v"(e[2]) : "s"(cs[0]), "s"(cs[1]), "s"(cs[2]));
    asm("v_mad_u64_u32 %0, vcc, %3, 1, %0\n\t"
        "v_mad_u64_u32 %1, vcc, %4, 1, %1\n\t"
        "v_mad_u64_u32 %2, vcc, %5, 1, %2"
        : "+v"(t[0]), "+v"(t[1]), "+v"(t[2]) : "v"(e[0]), "v"(e[1]), "v"(e[2]) : "vcc");
    // r = t - w3 (borrow b); e = b ? eps : 0; r -= e
    asm("v_sub_co_u32_e64 %0, %3, %6, %9\n\t"
        "v_sub_co_u32_e64 %1, %4, %7, %10\n\t"
        "v_sub_co_u32_e64 %2, %5, %8, %11"
        : "=&v"(r0[0]), "=&v"(r0[1]), "=&v"(r0[2]), "=&s"(cs[0]), "=&s"(cs[1]), "=&s"(cs[2])
        : "v"(lo32(t[0])), "v"(lo32(t[1])), "v"(lo32(t[2])), "v"(hi32(W[0])), "v"(hi32(W[1])), "v"(hi32(W[2])));
    asm("v_subb_co_u32_e64 %0, %3, %6, 0, %3\n\t"
        "v_subb_co_u32_e64 %1, %4, %7, 0, %4\n\t"
        "v_subb_co_u32_e64 %2, %5, %8, 0, %5"
        : "=&v"(r1[0]), "=&v"(r1[1]), "=&v"(r1[2]), "+s"(cs[0]), "+s"(cs[1]), "+s"(cs[2])
        : "v"(hi32(t[0])), "v"(hi32(t[1])), "v"(hi32(t[2])));
    asm("v_cndmask_b32_e64 %0, 0, -1, %3\n\t"
        "v_cndmask_b32_e64 %1, 0, -1, %4\n\t"
        "v_cndmask_b32_e64 %2, 0, -1, %5"
        : "=v"(e[0]), "=v"(e[1]), "=v"(e[2]) : "s"(cs[0]), "s"(cs[1]), "s"(cs[2]));
    asm("v_sub_co_u32_e64 %0, %3, %0, %6\n\t"
        "v_sub_co_u32_e64 %1, %4, %1, %7\n\t"
        "v_sub_co_u32_e64 %2, %5, %2, %8"
        : "+v"(r0[0]), "+v"(r0[1]), "+v"(r0[2]), "=&s"(cs[0]), "=&s"(cs[1]), "=&s"(cs[2])
        : "v"(e[0]), "v"(e[1]), "v"(e[2]));
    asm("v_subb_co_u32_e64 %0, vcc, %0, 0, %3\n\t"
        "v_subb_co_u32_e64 %1, vcc, %1, 0, %4\n\t"
        "v_subb_co_u32_e64 %2, vcc, %2, 0, %5"
        : "+v"(r1[0]), "+v"(r1[1]), "+v"(r1[2]) : "s"(cs[0]), "s"(cs[1]), "s"(cs[2]) : "vcc");
  } else {
    asm("v_mad_u64_u32 %0, %2, %4, -1, %6\n\t"
        "v_mad_u64_u32 %1, %3, %5, -1, %7"
        : "=&v"(t[0]), "=&v"(t[1]), "=&s"(cs[0]), "=&s"(cs[1])
        : "v"(lo32(W[0])), "v"(lo32(W[1])), "v"(X[0]), "v"(X[1]));
    asm(QP_W2 "v_cndmask_b32_e64 %0, 0, -1, %2\n\t"
        "v_cndmask_b32_e64 %1, 0, -1, %3"
        : "=v"(e[0]), "=v"(e[1]) : "s"(cs[0]), "s"(cs[1]));
    asm("v_mad_u64_u32 %0, vcc, %2, 1, %0\n\t"
        "v_mad_u64_u32 %1, vcc, %3, 1, %1"
        : "+v"(t[0]), "+v"(t[1]) : "v"(e[0]), "v"(e[1]) : "vcc");
    asm("v_sub_co_u32_e64 %0, %2, %4, %6\n\t"
        "v_sub_co_u32_e64 %1, %3, %5, %7"
        : "=&v"(r0[0]), "=&v"(r0[1]), "=&s"(cs[0]), "=&s"(cs[1])
        : "v"(lo32(t[0])), "v"(lo32(t[1])), "v"(hi32(W[0])), "v"(hi32(W[1])));
    asm(QP_W2 "v_subb_co_u32_e64 %0, %2, %4, 0, %2\n\t"
        "v_subb_co_u32_e64 %1, %3, %5, 0, %3"
        : "=&v"(r1[0]), "=&v"(r1[1]), "+s"(cs[0]), "+s"(cs[1])
        : "v"(hi32(t[0])), "v"(hi32(t[1])));
    asm(QP_W2 "v_cndmask_b32_e64 %0, 0, -1, %2\n\t"
        "v_cndmask_b32_e64 %1, 0, -1, %3"
        : "=v"(e[0]), "=v"(e[1]) : "s"(cs[0]), "s"(cs[1]));
    asm("v_sub_co_u32_e64 %0, %2, %0, %4\n\t"
        "v_sub_co_u32_e64 %1, %3, %1, %5"
        : "+v"(r0[0]), "+v"(r0[1]), "=&s"(cs[0]), "=&s"(cs[1])
        : "v"(e[0]), "v"(e[1]));
    asm(QP_W2 "v_subb_co_u32_e64 %0, vcc, %0, 0, %2\n\t"
        "v_subb_co_u32_e64 %1, vcc, %1, 0, %3"
        : "+v"(r1[0]), "+v"(r1[1]) : "s"(cs[0]), "s"(cs[1]) : "vcc");
  }
#pragma unroll
  for (int i = 0; i < K; i++) r[i] = ((uint64_t)r1[i] << 32) | r0[i];
}

// Lazily reduced sum of products (the quotient's alpha-weighted constraint
// sums): sum_i a_i b_i held as lo + 2^64 hi + 2^128 top, top counting the
// carries out of 2^128 (fewer than 2^32 terms), reduced once by value().  One
// product-accumulate is 4 mads + 1 cndmask + 3 addc, against a reduced
// product and a reduced add (13 + 6) per term.
struct Acc3 {
  uint64_t lo = 0, hi = 0;
  uint32_t top = 0;
  __device__ __forceinline__ void mac(uint64_t a, uint64_t b) {
    const uint32_t a0 = lo32(a), a1 = hi32(a), b0 = lo32(b), b1 = hi32(b);
    // L = a0 b0 + lo, carry-out cl worth 2^64; the rest of the product is then
    // the exact high part of a b + lo - cl 2^64 < 2^128, so W < 2^64
    uint64_t L, cl, U, cu, c;
    asm("v_mad_u64_u32 %0, %1, %2, %3, %4" : "=v"(L), "=s"(cl) : "v"(a0), "v"(b0), "v"(lo));
    const uint64_t T = (uint64_t)a0 * b1 + hi32(L);
    asm("v_mad_u64_u32 %0, %1, %2, %3, %4" : "=v"(U), "=s"(cu) : "v"(a1), "v"(b0), "v"(T));
    uint32_t ce;
    asm(QP_CWAIT "v_cndmask_b32_e64 %0, 0, 1, %1" : "=v"(ce) : "s"(cu));
    const uint64_t W = (uint64_t)a1 * b1 + (((uint64_t)ce << 32) | hi32(U));
    lo = ((uint64_t)lo32(U) << 32) | lo32(L);
    // hi += W + cl; top += the carry out
    uint32_t h0 = lo32(hi), h1 = hi32(hi);
    asm("v_addc_co_u32_e64 %0, %1, %2, %3, %4" : "=v"(h0), "=s"(c) : "v"(h0), "v"(lo32(W)), "s"(cl));
    asm(QP_CWAIT "v_addc_co_u32_e64 %0, %1, %2, %3, %1" : "=v"(h1), "+s"(c) : "v"(h1), "v"(hi32(W)));
    asm(QP_CWAIT "v_addc_co_u32_e64 %0, %1, %2, 0, %1" : "=v"(top), "+s"(c) : "v"(top));
    hi = ((uint64_t)h1 << 32) | h0;
  }
  // += x 2^e (0 <= e < 64) as the 128-bit integer it is: no reduction
  __device__ __forceinline__ void add_shifted(uint64_t x, uint32_t e) {
    const uint64_t xl = x << e, xh = e ? x >> (64 - e) : 0;
    uint32_t c0, c1, c2, c3, c4;
    const uint32_t l0 = __builtin_addc(lo32(lo), lo32(xl), 0u, &c0);
    const uint32_t l1 = __builtin_addc(hi32(lo), hi32(xl), c0, &c1);
    const uint32_t h0 = __builtin_addc(lo32(hi), lo32(xh), c1, &c2);
    const uint32_t h1 = __builtin_addc(hi32(hi), hi32(xh), c2, &c3);
    top = __builtin_addc(top, 0u, c3, &c4);
    lo = ((uint64_t)l1 << 32) | l0;
    hi = ((uint64_t)h1 << 32) | h0;
  }
  // 2^128 = 2^96 2^32 = -2^32 (mod p)
  __device__ __forceinline__ uint64_t value() const { return sub(reduce(lo, hi), (uint64_t)top << 32); }
};

}  // namespace gfn
