// witness_probe.cpp — TEST-ONLY probe of device witness generation
// (qp_debug_witness_program, include/qpgpu.h).  A caller's generator program,
// validated first (witness_program.h), goes through the production kernels of
// witness.hip with the launches of the prover's gen_witness_batch
// (witness_launch.h): k_witness_init, k_witness_inputs, then k_witness_gen or
// the k_witness_level loop, and witness_expand on request.  Nothing here
// restates a generator; tests/test_gpu_witness_program.py compares the slot
// values with a Python-integer model.
#include "../../include/qpgpu.h"
#include <string>
#include "ctx.h"
#include "witness_kernels.h"
#include "witness_launch.h"
#include "witness_program.h"

namespace {

qpk::WitnessForm form_of(uint32_t form) {
  switch (form) {
    case QP_WFORM_PROOF_256: return {256u, false, true};
    case QP_WFORM_PROOF_512: return {512u, false, true};
    case QP_WFORM_LEVEL_ROW: return {256u, true, true};
    case QP_WFORM_LEVEL_WAVE: return {256u, true, false};
    case QP_WFORM_PROOF_256_WAVE: return {256u, false, false};
    default: return {512u, false, false};  // QP_WFORM_PROOF_512_WAVE
  }
}

// n 32-bit words (at least one) to the device
hipError_t up32(DevBuf &d, const uint32_t *src, size_t n, hipStream_t s) {
  hipError_t e = d.alloc((n + 1) / 2);
  if (!e && n) e = hipMemcpyAsync(d.p, src, n * 4, hipMemcpyHostToDevice, s);
  return e;
}
hipError_t up64(DevBuf &d, const uint64_t *src, size_t n, hipStream_t s) {
  hipError_t e = d.alloc(n);
  if (!e && n) e = hipMemcpyAsync(d.p, src, n * 8, hipMemcpyHostToDevice, s);
  return e;
}

}  // namespace

extern "C" int qp_debug_witness_program(qp_ctx *c, const qp_witness_program *prog, uint64_t *vals, uint32_t *err,
                                        uint64_t *wires, uint64_t *pis) {
  if (!c) return QP_ERR_ARG;
  if (!prog || !vals || !err) { c->err = "qp_debug_witness_program: null argument"; return QP_ERR_ARG; }
  const qp_witness_program &p = *prog;
  const std::string fault = qwp::validate(p);
  if (!fault.empty()) { c->err = "qp_debug_witness_program: " + fault; return QP_ERR_ARG; }
  if (p.wslot_cm && (!wires || (p.npis && !pis))) { c->err = "qp_debug_witness_program: null argument"; return QP_ERR_ARG; }
  hipStream_t s = c->stream;
  const size_t nw = (size_t)p.nrows * p.W;
  DevBuf dgens, dlvl, dlpos, dwslot, din_slots, din, dvals, derr, dwcm, dpi, dwires, dpis;
  hipError_t e = hipSetDevice(c->device);
  if (!e) e = up64(dgens, p.gens, 5 * (size_t)p.ngens, s);
  if (!e) e = up32(dlvl, p.level_off, (size_t)p.nlevels + 1, s);
  if (!e) e = up32(dlpos, p.level_pos, 2 * (size_t)p.nlevels, s);
  if (!e) e = up32(dwslot, p.wslot, nw, s);
  if (!e) e = up32(din_slots, p.in_slots, p.nin, s);
  if (!e) e = up64(din, p.in_vals, (size_t)p.B * p.nin, s);
  if (!e) e = dvals.alloc((size_t)p.B * p.nslots);
  if (!e) e = derr.alloc(((size_t)p.B + 1) / 2);
  if (!e && p.wslot_cm) {
    e = up32(dwcm, p.wslot_cm, nw, s);
    if (!e) e = up32(dpi, p.pi_slots, p.npis, s);
    if (!e) e = dwires.alloc((size_t)p.B * nw);
    if (!e) e = dpis.alloc((size_t)p.B * p.npis);
  }
  if (!e) {
    qpk::witness_launch_init(dvals.p, p.nslots, din_slots.as<uint32_t>(), din.p, p.nin, p.B, s);
    e = hipMemsetAsync(derr.p, 0, (size_t)p.B * 4, s);
  }
  if (!e) {
    qpk::WitnessGenArgs a;
    a.vals = dvals.p;
    a.v_bstride = p.nslots;
    a.gens = dgens.p;
    a.level_off = dlvl.as<uint32_t>();
    a.level_pos = dlpos.as<uint32_t>();
    a.nlevels = p.nlevels;
    a.coop_max = 0;  // set by witness_launch_gens
    a.row = 0;
    a.wslot = dwslot.as<uint32_t>();
    a.W = p.W;
    a.limbs = p.limbs;
    a.zero_slot = p.zero_slot;
    a.num_consts = p.num_consts;
    a.err = derr.as<uint32_t>();
    qpk::witness_launch_gens(a, form_of(p.form), p.level_off, p.level_pos, p.B, s);
    if (p.wslot_cm)
      qpk::witness_expand(dvals.p, p.nslots, dwcm.as<uint32_t>(), nw, dwires.p, nw, dpi.as<uint32_t>(), p.npis, dpis.p,
                          p.B, s);
    e = hipGetLastError();
  }
  if (!e) e = hipMemcpyAsync(vals, dvals.p, (size_t)p.B * p.nslots * 8, hipMemcpyDeviceToHost, s);
  if (!e) e = hipMemcpyAsync(err, derr.p, (size_t)p.B * 4, hipMemcpyDeviceToHost, s);
  if (!e && p.wslot_cm) e = hipMemcpyAsync(wires, dwires.p, (size_t)p.B * nw * 8, hipMemcpyDeviceToHost, s);
  if (!e && p.wslot_cm && p.npis) e = hipMemcpyAsync(pis, dpis.p, (size_t)p.B * p.npis * 8, hipMemcpyDeviceToHost, s);
  if (!e) e = hipStreamSynchronize(s);
  if (e) {
    c->err = std::string("qp_debug_witness_program: ") + hipGetErrorString(e);
    return e == hipErrorOutOfMemory ? QP_ERR_OOM : QP_ERR_HIP;
  }
  return QP_OK;
}
