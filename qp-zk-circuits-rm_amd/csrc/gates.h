// gates.h — the one table of plonky2 gates (host only): the kind numbering the
// whole library uses (= the ABI's QP_GATE_*), the DefaultGateSerializer ids
// both ways, the number of serialized parameters and the shape of a gate given
// its parameters.  The builder, the prover, the routine-level seams, the
// common-data parser and the verifiers read it; the CPU oracle (oracle/) keeps
// its own table on purpose: it is the checker.
#pragma once
#include <stdint.h>
#include "../../include/qpgpu.h"

namespace qg {

// parameters p0, p1, p2 in serialization order
enum GateKind : uint8_t {
  G_NOOP = 0, G_CONSTANT,  // {num_consts}
  G_PUBLIC_INPUT,
  G_BASE_SUM,         // BaseSumGate<2>{num_limbs}
  G_ARITHMETIC,       // {num_ops}: out = c0 m0 m1 + c1 addend
  G_POSEIDON,
  // the recursive verifier's gates (plonky2 verify_proof; aggregation circuits)
  G_ARITH_EXT,        // ArithmeticExtensionGate{num_ops}: out = c0 m0 m1 + c1 addend (ext)
  G_MUL_EXT,          // MulExtensionGate{num_ops}: out = c0 m0 m1 (ext)
  G_RANDOM_ACCESS,    // RandomAccessGate{bits, num_copies, num_extra_constants}
  G_EXPONENTIATION,   // ExponentiationGate{num_power_bits} (seams only: neither built nor parsed)
  G_REDUCING,         // ReducingGate{num_coeffs}: Horner of base coefficients by an ext alpha
  G_REDUCING_EXT,     // ReducingExtensionGate{num_coeffs}: the same over ext coefficients
  G_POSEIDON_MDS,     // PoseidonMdsGate: the 12x12 MDS layer on ext values
  G_COSET_INTERP,     // CosetInterpolationGate{subgroup_bits, degree}
  G_NKINDS
};
static_assert(int(G_NOOP) == QP_GATE_NOOP && int(G_CONSTANT) == QP_GATE_CONSTANT &&
                  int(G_PUBLIC_INPUT) == QP_GATE_PUBLIC_INPUT && int(G_BASE_SUM) == QP_GATE_BASE_SUM &&
                  int(G_ARITHMETIC) == QP_GATE_ARITHMETIC && int(G_POSEIDON) == QP_GATE_POSEIDON &&
                  int(G_ARITH_EXT) == QP_GATE_ARITHMETIC_EXTENSION && int(G_MUL_EXT) == QP_GATE_MUL_EXTENSION &&
                  int(G_RANDOM_ACCESS) == QP_GATE_RANDOM_ACCESS && int(G_EXPONENTIATION) == QP_GATE_EXPONENTIATION &&
                  int(G_REDUCING) == QP_GATE_REDUCING && int(G_REDUCING_EXT) == QP_GATE_REDUCING_EXTENSION &&
                  int(G_POSEIDON_MDS) == QP_GATE_POSEIDON_MDS && int(G_COSET_INTERP) == QP_GATE_COSET_INTERPOLATION,
              "GateKind is the ABI's QP_GATE_*");

// per kind: plonky2 DefaultGateSerializer id, serialized u64 parameters
// (CosetInterpolation's barycentric weight vector follows its two)
constexpr struct { uint8_t serial, nparams; } GATE_SERIAL[G_NKINDS] = {
    {9, 0}, {3, 1}, {12, 0}, {2, 1}, {0, 1}, {11, 0}, {1, 1}, {8, 1}, {13, 3}, {5, 1}, {15, 1}, {14, 1}, {10, 0}, {4, 2}};
constexpr uint32_t serial_id(GateKind k) { return GATE_SERIAL[k].serial; }
constexpr uint32_t serial_params(GateKind k) { return GATE_SERIAL[k].nparams; }
// G_NKINDS for an id outside the table
constexpr GateKind kind_from_serial(uint32_t id) {
  for (uint32_t k = 0; k < G_NKINDS; k++)
    if (GATE_SERIAL[k].serial == id) return (GateKind)k;
  return G_NKINDS;
}

// wires and gate constants a gate reads and constraints it emits (64-bit: the
// parameters may be raw words of a caller's description), its degree for the
// selector groups, and whether the parameters are inside the bounds the
// evaluators support (RandomAccess bits 1..6, CosetInterpolation bits 2..6
// with 2 <= degree <= 2^bits, Exponentiation >= 1 bit); all zero if not
struct GateShape {
  uint64_t wires = 0, consts = 0, constraints = 0;
  uint32_t degree = 0;
  bool ok = false;
};
inline GateShape gate_shape(uint32_t kind, uint64_t p0, uint64_t p1 = 0, uint64_t p2 = 0) {
  auto shape = [](uint64_t w, uint64_t k, uint64_t c, uint64_t deg) { return GateShape{w, k, c, (uint32_t)deg, true}; };
  switch (kind) {
    case G_NOOP: return shape(0, 0, 0, 0);
    case G_CONSTANT: return shape(p0, p0, p0, 1);
    case G_PUBLIC_INPUT: return shape(4, 0, 4, 1);
    case G_BASE_SUM: return shape(1 + p0, 0, 1 + p0, 2);
    case G_ARITHMETIC: return shape(4 * p0, 2, p0, 3);
    case G_POSEIDON: return shape(135, 0, 123, 7);
    case G_ARITH_EXT: return shape(8 * p0, 2, 2 * p0, 3);
    case G_MUL_EXT: return shape(6 * p0, 1, 2 * p0, 3);
    case G_RANDOM_ACCESS:
      if (p0 < 1 || p0 > 6) break;
      return shape((2 + (1ull << p0)) * p1 + p2 + p1 * p0, p2, (p0 + 2) * p1 + p2, p0 + 1);
    case G_EXPONENTIATION:
      if (p0 < 1) break;
      return shape(2 + 2 * p0, 0, p0 + 1, 4);
    case G_REDUCING: return shape(6 + p0 + 2 * (p0 ? p0 - 1 : 0), 0, 2 * p0, 2);
    case G_REDUCING_EXT: return shape(6 + 2 * p0 + 2 * (p0 ? p0 - 1 : 0), 0, 2 * p0, 2);
    case G_POSEIDON_MDS: return shape(48, 0, 24, 1);
    case G_COSET_INTERP: {
      if (p0 < 2 || p0 > 6 || p1 < 2 || p1 > (1ull << p0)) break;
      const uint64_t np = 1ull << p0, nint = (np - 2) / (p1 - 1);
      // shift, values, evaluation point and value, intermediate evals and products, shifted point
      return shape(1 + 2 * np + 4 + 4 * nint + 2, 0, 4 + 4 * nint, p1);
    }
    default: break;
  }
  return GateShape{};
}

}  // namespace qg
