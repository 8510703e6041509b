// input_screen.cpp — C ABI of the Wormhole input screen (include/qpgpu.h):
// the host path (ctx == NULL: input_screen.h's rules over the host Poseidon)
// and the device path's host side: statuses 1..3 and the packing into one
// pinned buffer, one upload, the two launches of input_screen.hip, one
// download.  The buffers belong to the call: every return path frees them.
#include <chrono>
#include <new>
#include <string>
#include <vector>
#include "../../include/qpgpu.h"
#include "ctx.h"
#include "field.h"
#include "input_screen.h"
#include "input_screen_kernels.h"
#include "poseidon.h"

namespace {

struct HostHash {
  static void permute(uint64_t s[12]) {
    for (int j = 0; j < 12; j++) s[j] = gl::canon(s[j]);
    ps::permute(s);
  }
  static uint64_t canon(uint64_t x) { return gl::canon(x); }
};

// inputs per upload: 1024 records are 16 MB of pinned memory
constexpr uint32_t SCREEN_CHUNK = 1024;

struct PinnedBuf {
  uint8_t *p = nullptr;
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf &) = delete;
  ~PinnedBuf() {
    if (p) (void)hipHostFree(p);
  }
};

thread_local double g_times[4] = {0, 0, 0, 0};

// a packed record's statuses 4..7 on the host: the same two steps the device runs as two launches
uint32_t host_rules(const uint8_t *rec, uint32_t *witness) {
  const uint64_t *hdr = qis::rec_hdr(rec);
  const uint32_t proof_len = (uint32_t)hdr[qis::H_PROOF_LEN];
  uint64_t dig[qis::MAX_NODES * 4], child[qis::MAX_NODES * 4];
  for (uint32_t i = 0; i < proof_len; i++) {
    const uint32_t *limbs = qis::rec_nodes(rec) + (size_t)i * qis::NODE_STRIDE;
    qis::node_digest<HostHash>(limbs, dig + 4 * i);
    qis::child_digest(limbs, qis::rec_start(rec)[i], child + 4 * i);
  }
  return qis::resolve<HostHash>(hdr, dig, child, witness);
}

int screen_host(const qp_wormhole_inputs *in, uint32_t n, uint32_t *status, uint32_t *witness) {
  std::vector<uint64_t> rec(qis::REC_BYTES / 8);  // 8-byte words: the record's alignment on the host
  uint8_t *r = reinterpret_cast<uint8_t *>(rec.data());
  for (uint32_t i = 0; i < n; i++) {
    status[i] = qis::pack_input(in[i], r, &witness[i]);
    if (status[i] == qis::OK) status[i] = host_rules(r, &witness[i]);
  }
  return QP_OK;
}

int screen_device_chunk(qp_ctx *c, const qp_wormhole_inputs *in, uint32_t n, uint32_t *status, uint32_t *witness,
                        uint8_t *pinned, DevBuf &din, DevBuf &dout, TimingEvents<4> &ev) {
  hipStream_t s = c->stream;
  // the pinned buffer and its device copy: work [n * 20] u32 (n * 80 bytes, a multiple of 16), then the records
  const size_t work_bytes = (size_t)n * qis::MAX_NODES * 4;
  uint32_t *work = reinterpret_cast<uint32_t *>(pinned);
  uint8_t *recs = pinned + work_bytes;
  std::vector<uint32_t> pos;
  pos.reserve(n);
  uint32_t m = 0, nwork = 0;
  const auto t0 = std::chrono::steady_clock::now();
  for (uint32_t i = 0; i < n; i++) {
    status[i] = qis::pack_input(in[i], recs + (size_t)m * qis::REC_BYTES, &witness[i]);
    if (status[i] != qis::OK) continue;
    for (uint32_t k = 0; k < in[i].num_nodes; k++) work[nwork++] = m * qis::MAX_NODES + k;
    pos.push_back(i);
    m++;
  }
  g_times[0] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (!m) return QP_OK;  // the device never sees an input the host refused
  // the outputs: err (16 bytes), res [m][2] u32 (rounded up to 16 bytes: the digests are stored 16 bytes at a
  // time), dig and child [m][20][4] u64
  const size_t res_off = 16, dig_off = res_off + (((size_t)m * 8 + 15) & ~(size_t)15);
  const size_t dig_bytes = (size_t)m * qis::MAX_NODES * 32;
  uint8_t *o = dout.as<uint8_t>();
  qpk::ScreenDev d;
  d.work = din.as<uint32_t>();
  d.rec = din.as<uint8_t>() + work_bytes;
  d.err = reinterpret_cast<uint32_t *>(o);
  d.res = reinterpret_cast<uint32_t *>(o + res_off);
  d.dig = reinterpret_cast<uint64_t *>(o + dig_off);
  d.child = reinterpret_cast<uint64_t *>(o + dig_off + dig_bytes);
  d.nwork = nwork;
  d.m = m;
  QP_HIP_TRY(c, hipEventRecord(ev.e[0], s));
  QP_HIP_TRY(c, hipMemcpyAsync(din.p, pinned, work_bytes + (size_t)m * qis::REC_BYTES, hipMemcpyHostToDevice, s));
  QP_HIP_TRY(c, hipMemsetAsync(o, 0, 16, s));
  QP_HIP_TRY(c, hipEventRecord(ev.e[1], s));
  qpk::screen_nodes(d, s);
  QP_HIP_TRY(c, hipGetLastError());
  QP_HIP_TRY(c, hipEventRecord(ev.e[2], s));
  qpk::screen_resolve(d, s);
  QP_HIP_TRY(c, hipGetLastError());
  QP_HIP_TRY(c, hipEventRecord(ev.e[3], s));
  std::vector<uint32_t> back(4 + (size_t)m * 2);
  QP_HIP_TRY(c, hipMemcpyAsync(back.data(), o, 16 + (size_t)m * 8, hipMemcpyDeviceToHost, s));
  QP_HIP_TRY(c, hipStreamSynchronize(s));
  for (int k = 0; k < 3; k++) {
    float ms = 0;
    QP_HIP_TRY(c, hipEventElapsedTime(&ms, ev.e[k], ev.e[k + 1]));
    g_times[1 + k] += ms;
  }
  if (back[0]) {
    c->err = "input screen: device error word " + std::to_string(back[0]) + " (a branch that cannot be reached)";
    return QP_ERR_STATE;
  }
  for (uint32_t j = 0; j < m; j++) {
    status[pos[j]] = back[4 + 2 * j];
    witness[pos[j]] = back[4 + 2 * j + 1];
  }
  return QP_OK;
}

int screen_device(qp_ctx *c, const qp_wormhole_inputs *in, uint32_t n, uint32_t *status, uint32_t *witness) {
  QP_HIP_TRY(c, hipSetDevice(c->device));
  const uint32_t cap = n < SCREEN_CHUNK ? n : SCREEN_CHUNK;
  const size_t in_bytes = (size_t)cap * (qis::MAX_NODES * 4 + qis::REC_BYTES);
  const size_t out_bytes = 16 + 16 + (size_t)cap * (8 + 2 * qis::MAX_NODES * 32);
  PinnedBuf pinned;
  DevBuf din, dout;
  TimingEvents<4> ev;
  QP_HIP_TRY(c, hipHostMalloc((void **)&pinned.p, in_bytes, hipHostMallocDefault));
  QP_HIP_TRY(c, din.alloc((in_bytes + 7) / 8));
  QP_HIP_TRY(c, dout.alloc((out_bytes + 7) / 8));
  for (hipEvent_t &e : ev.e) QP_HIP_TRY(c, hipEventCreate(&e));
  for (uint32_t done = 0; done < n; done += cap) {
    const uint32_t nb = n - done < cap ? n - done : cap;
    const int rc = screen_device_chunk(c, in + done, nb, status + done, witness + done, pinned.p, din, dout, ev);
    if (rc) return rc;
  }
  return QP_OK;
}

}  // namespace

extern "C" {

int qp_wormhole_inputs_screen(qp_ctx *ctx, const qp_wormhole_inputs *in, uint32_t n, uint32_t *status,
                              uint32_t *witness) {
  if (!n) return QP_OK;
  if (!in || !status || !witness) {
    if (ctx) ctx->err = "input screen: null inputs, status or witness array";
    return QP_ERR_ARG;
  }
  for (uint32_t i = 0; i < n; i++)
    if (!qis::pointers_ok(in[i])) {
      if (ctx) ctx->err = "input screen: input " + std::to_string(i) + " has a null storage-proof array or node";
      return QP_ERR_ARG;
    }
  for (double &t : g_times) t = 0;
  try {
    return ctx ? screen_device(ctx, in, n, status, witness) : screen_host(in, n, status, witness);
  } catch (const std::bad_alloc &) {
    return QP_ERR_OOM;
  }
}

const char *qp_input_status_text(uint32_t status) { return qis::status_text(status); }

int qp_wormhole_inputs_screen_times(double ms[4]) {
  if (!ms) return QP_ERR_ARG;
  for (int k = 0; k < 4; k++) ms[k] = g_times[k];
  return QP_OK;
}

}  // extern "C"
