// gate_constraints.h — gates/*::eval_unfiltered at one point, written once over
// the arithmetic GG: the recursive verifier instantiates it on circuit targets
// (recursion.cpp, the operations land on ArithmeticExtension / MulExtension /
// PoseidonMds rows in the order written here), the native verifier on plain
// quadratic-extension values (verifier.cpp).  GG provides E (an extension
// element), Alg (a pair of them, the extension algebra a + b Y) and the
// operations used below.
#pragma once
#include <algorithm>
#include <stdexcept>
#include <vector>
#include "field.h"
#include "poseidon.h"
#include "recursion.h"

namespace qr {

// ExtensionAlgebra<2> over E on GG's operations (gadgets/arithmetic_extension.rs):
// mul_add is the W-weighted inner product first, then the plain one
template <class D, class EE>
struct AlgOps {
  struct Alg {
    EE a, b;
  };
  D &self() { return *static_cast<D *>(this); }
  Alg alg(const std::vector<EE> &w, uint32_t i) { return {w[i], w[i + 1]}; }
  Alg alg_zero() { return {self().ext_zero(), self().ext_zero()}; }
  Alg alg_sub(Alg x, Alg y) { return {self().sub(x.a, y.a), self().sub(x.b, y.b)}; }
  Alg alg_mul_add(Alg x, Alg y, Alg z) {
    EE r0 = self().arithmetic_extension(gl::EXT_W, 1, x.b, y.b, z.a);
    r0 = self().mul_add(x.a, y.a, r0);
    EE r1 = self().mul_add(x.a, y.b, z.b);
    r1 = self().mul_add(x.b, y.a, r1);
    return {r0, r1};
  }
  Alg alg_mul(Alg x, Alg y) { return alg_mul_add(x, y, alg_zero()); }
  Alg alg_scalar_mul_add(EE c, Alg x, Alg z) { return {self().mul_add(c, x.a, z.a), self().mul_add(c, x.b, z.b)}; }
  Alg alg_scalar_mul(EE c, Alg x) { return alg_scalar_mul_add(c, x, alg_zero()); }
  void push(std::vector<EE> &out, Alg x) {
    out.push_back(x.a);
    out.push_back(x.b);
  }
};

// MDS layer on ext states: one PoseidonMdsGate row (mds_layer_circuit with
// num_routed_wires >= 48)
template <class GG>
void mds_ext(GG &g, typename GG::E s[12]) {
  std::vector<typename GG::E> v(s, s + 12);
  v = g.poseidon_mds(v);
  for (int r = 0; r < 12; r++) s[r] = v[r];
}

// sbox_monomial_circuit: exp_u64_extension(x, 7)
template <class GG>
typename GG::E sbox_ext(GG &g, typename GG::E x) { return g.exp_u64(x, 7); }

// gates/*::eval_unfiltered_circuit (values at zeta), in upstream plonky2's
// operation forms (values pinned by SURVEY.md A.5 for the leaf gates; the
// recursion gates' formulas restate upstream, parity unpinned)
template <class GG, class PI>
std::vector<typename GG::E> gate_constraints(GG &g, const InnerCommon::Gate &gate,
                                             const std::vector<typename GG::E> &w, const typename GG::E *gc,
                                             const std::vector<PI> &pi_hash) {
  using ExtT = typename GG::E;
  using Alg = typename GG::Alg;
  std::vector<ExtT> out;
  switch (gate.kind) {
    case qc::G_NOOP:
      break;
    case qc::G_CONSTANT:
      for (uint32_t i = 0; i < gate.p[0]; i++) out.push_back(g.sub(gc[i], w[i]));
      break;
    case qc::G_PUBLIC_INPUT:
      for (uint32_t i = 0; i < 4; i++) out.push_back(g.sub(w[i], g.ext(pi_hash[i])));
      break;
    case qc::G_BASE_SUM: {  // BaseSum<2>: the recomposed sum, then limb (limb - 1) per limb
      const uint32_t L = (uint32_t)gate.p[0];
      std::vector<ExtT> limbs(w.begin() + 1, w.begin() + 1 + L);
      out.push_back(g.sub(g.reduce(g.ext_const(2), limbs), w[0]));
      for (ExtT l : limbs) out.push_back(g.mul_sub(l, l, l));
      break;
    }
    case qc::G_ARITHMETIC: {  // out - (c0 m0 m1 + c1 addend)
      for (uint32_t i = 0; i < gate.p[0]; i++) {
        ExtT scaled = g.mul_many({gc[0], w[4 * i], w[4 * i + 1]});
        ExtT comp = g.mul_add(gc[1], w[4 * i + 2], scaled);
        out.push_back(g.sub(w[4 * i + 3], comp));
      }
      break;
    }
    case qc::G_ARITH_EXT:  // ArithmeticExtension{num_ops}: out - (c0 m0 m1 + c1 addend), algebra
    case qc::G_MUL_EXT: {  // MulExtension{num_ops}: out - c0 m0 m1
      const bool ae = gate.kind == qc::G_ARITH_EXT;
      for (uint32_t i = 0; i < gate.p[0]; i++) {
        const uint32_t o = ae ? 8 * i : 6 * i;
        Alg scaled = g.alg_scalar_mul(gc[0], g.alg_mul(g.alg(w, o), g.alg(w, o + 2)));
        if (ae) scaled = g.alg_scalar_mul_add(gc[1], g.alg(w, o + 4), scaled);
        g.push(out, g.alg_sub(g.alg(w, ae ? o + 6 : o + 4), scaled));
      }
      break;
    }
    case qc::G_REDUCING:  // Reducing{num_coeffs}: acc_i - (acc_{i-1} alpha + coeff_i), base coefficients
    case qc::G_REDUCING_EXT: {  // ReducingExtension{num_coeffs}: ext coefficients
      const uint32_t nc = (uint32_t)gate.p[0], cw = gate.kind == qc::G_REDUCING ? 1 : 2;
      const Alg alpha = g.alg(w, 2);
      Alg acc = g.alg(w, 4);
      for (uint32_t i = 0; i < nc; i++) {
        const Alg coeff = cw == 1 ? Alg{w[6 + i], g.ext_zero()} : g.alg(w, 6 + 2 * i);
        const Alg next = g.alg(w, i + 1 == nc ? 0 : 6 + cw * nc + 2 * i);
        g.push(out, g.alg_sub(g.alg_mul_add(acc, alpha, coeff), next));
        acc = next;
      }
      break;
    }
    case qc::G_POSEIDON_MDS: {  // out_r - (sum_i CIRC[i] in_{i+r} + DIAG[r] in_r), algebra
      for (uint32_t r = 0; r < 12; r++) {
        Alg res = g.alg_zero();
        for (uint32_t i = 0; i < 12; i++)
          res = g.alg_scalar_mul_add(g.ext_const(ps::mds_circ(i)), g.alg(w, 2 * ((i + r) % 12)), res);
        res = g.alg_scalar_mul_add(g.ext_const(r == 0 ? 8 : 0), g.alg(w, 2 * r), res);
        g.push(out, g.alg_sub(g.alg(w, 24 + 2 * r), res));
      }
      break;
    }
    case qc::G_COSET_INTERP: {  // CosetInterpolation{subgroup_bits, degree}
      const uint32_t nbits = (uint32_t)gate.p[0], deg = (uint32_t)gate.p[1], np = 1u << nbits;
      const uint32_t nint = (np - 2) / (deg - 1);
      const uint32_t sv = 1, sep = sv + 2 * np, sev = sep + 2, si = sev + 2, ssh = si + 4 * nint;
      const ExtT shift = w[0];
      const Alg ep = g.alg(w, sep), sp = g.alg(w, ssh);
      g.push(out, g.alg_scalar_mul_add(g.scale(shift, gl::P - 1), sp, ep));
      const F om = gl::root_of_unity(nbits), ninv = gl::inv(np);
      Alg ev = g.alg_zero(), pr{g.ext_const(1), g.ext_zero()};
      uint32_t lo = 0, hi = deg;
      for (uint32_t it = 0;; it++) {
        for (uint32_t i = lo; i < hi; i++) {
          const F x = gl::pow(om, i);
          const Alg term{g.sub(sp.a, g.ext_const(x)), sp.b};
          const Alg wv = g.alg_scalar_mul(g.ext_const(gl::mul(x, ninv)), g.alg(w, sv + 2 * i));
          ev = g.alg_mul_add(wv, pr, g.alg_mul(ev, term));
          pr = g.alg_mul(pr, term);
        }
        if (it == nint) break;
        const Alg ie = g.alg(w, si + 2 * it), ip = g.alg(w, si + 2 * (nint + it));
        g.push(out, g.alg_sub(ie, ev));
        g.push(out, g.alg_sub(ip, pr));
        ev = ie;
        pr = ip;
        lo = 1 + (deg - 1) * (it + 1);
        hi = std::min(lo + deg - 1, np);
      }
      g.push(out, g.alg_sub(g.alg(w, sev), ev));
      break;
    }
    case qc::G_RANDOM_ACCESS: {  // RandomAccess{bits, copies, extra}
      const uint32_t bits = (uint32_t)gate.p[0], copies = (uint32_t)gate.p[1], extra = (uint32_t)gate.p[2];
      const uint32_t vec = 1u << bits, routed = (2 + vec) * copies + extra;
      for (uint32_t cp = 0; cp < copies; cp++) {
        const uint32_t base = (2 + vec) * cp;
        std::vector<ExtT> bw(bits);
        for (uint32_t i = 0; i < bits; i++) bw[i] = w[routed + cp * bits + i];
        for (uint32_t i = 0; i < bits; i++) out.push_back(g.mul_sub(bw[i], bw[i], bw[i]));
        ExtT idx = g.ext_zero();
        for (uint32_t i = bits; i-- > 0;) idx = g.mul_const_add(2, idx, bw[i]);
        out.push_back(g.sub(idx, w[base]));
        std::vector<ExtT> list(w.begin() + base + 2, w.begin() + base + 2 + vec);
        for (uint32_t i = 0; i < bits; i++) {
          std::vector<ExtT> nx(list.size() / 2);
          // select_ext_generalized(b, y, x) = b y - (b x - x)
          for (size_t j = 0; j < nx.size(); j++)
            nx[j] = g.mul_sub(bw[i], list[2 * j + 1], g.mul_sub(bw[i], list[2 * j], list[2 * j]));
          list = nx;
        }
        out.push_back(g.sub(list[0], w[base + 1]));
      }
      for (uint32_t i = 0; i < extra; i++) out.push_back(g.sub(gc[i], w[(2 + vec) * copies + i]));
      break;
    }
    case qc::G_POSEIDON: {  // constant layers, x^7 S-boxes, PoseidonMdsGate layers, wire checks
      ExtT swap = w[24];
      out.push_back(g.mul_sub(swap, swap, swap));
      for (int i = 0; i < 4; i++) out.push_back(g.mul_sub(swap, g.sub(w[i + 4], w[i]), w[25 + i]));
      ExtT s[12];
      for (int i = 0; i < 4; i++) {
        ExtT delta = w[25 + i];
        s[i] = g.add(w[i], delta);
        s[i + 4] = g.sub(w[i + 4], delta);
      }
      for (int i = 8; i < 12; i++) s[i] = w[i];
      int rc = 0;
      for (int r = 0; r < 4; r++, rc++) {
        for (int i = 0; i < 12; i++) s[i] = g.add_const(s[i], ps::RC_HOST[rc * 12 + i]);
        if (r)
          for (int i = 0; i < 12; i++) {
            ExtT wi = w[29 + (r - 1) * 12 + i];
            out.push_back(g.sub(s[i], wi));
            s[i] = wi;
          }
        for (int i = 0; i < 12; i++) s[i] = sbox_ext(g, s[i]);
        mds_ext(g, s);
      }
      for (int r = 0; r < 22; r++, rc++) {
        for (int i = 0; i < 12; i++) s[i] = g.add_const(s[i], ps::RC_HOST[rc * 12 + i]);
        ExtT wi = w[65 + r];
        out.push_back(g.sub(s[0], wi));
        s[0] = sbox_ext(g, wi);
        mds_ext(g, s);
      }
      for (int r = 0; r < 4; r++, rc++) {
        for (int i = 0; i < 12; i++) s[i] = g.add_const(s[i], ps::RC_HOST[rc * 12 + i]);
        for (int i = 0; i < 12; i++) {
          ExtT wi = w[87 + r * 12 + i];
          out.push_back(g.sub(s[i], wi));
          s[i] = sbox_ext(g, wi);
        }
        mds_ext(g, s);
      }
      for (int i = 0; i < 12; i++) out.push_back(g.sub(s[i], w[12 + i]));
      break;
    }
    default:
      throw std::runtime_error("unsupported inner gate");
  }
  return out;
}

}  // namespace qr
