// ctx.h — internal definitions behind the C ABI handles (qpgpu.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <utility>
#include "kernels.h"

struct qp_ctx {
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  qpk::Twiddles tw;
  std::string err;
};

struct qp_batch {
  qp_ctx *ctx = nullptr;
  uint32_t nbat = 1, npolys = 0, nsalt = 0, log_n = 0, rate_bits = 0, cap_h = 0;
  uint64_t *d_coeffs = nullptr;  // [nbat][npolys][n]
  uint64_t *d_lde = nullptr;     // [nbat][npolys][N] leaf order
  uint64_t *d_salt = nullptr;    // [nbat][N][nsalt]
  uint64_t *d_dig = nullptr;     // [nbat][tree digests][4]
  uint64_t n() const { return (uint64_t)1 << log_n; }
  uint64_t N() const { return (uint64_t)1 << (log_n + rate_bits); }
  uint64_t ndig() const { return qpk::tree_digest_count(log_n + rate_bits, cap_h); }
};

// A device allocation of 64-bit words, owned by a handle or by one ABI call:
// every return path of the owner frees it.
struct DevBuf {
  uint64_t *p = nullptr;
  size_t words = 0;
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  DevBuf(DevBuf &&o) noexcept : p(o.p), words(o.words) { o.p = nullptr; }
  DevBuf &operator=(DevBuf &&o) noexcept {  // a swap: o frees what this one held
    std::swap(p, o.p);
    std::swap(words, o.words);
    return *this;
  }
  hipError_t alloc(size_t w) {  // at least one word: p is non-null after a successful alloc(0)
    release();
    words = w;
    return hipMalloc(&p, (w ? w : 1) * 8);
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    words = 0;
  }
  template <class T>
  T *as() const {
    return reinterpret_cast<T *>(p);
  }
  // hipFree waits for the device, so freeing while launches on the context's
  // stream are still running is safe.
  ~DevBuf() { release(); }
};

// The HIP timing events of a handle or of one ABI call: the owner creates the
// null ones before it records them; every return path of the owner destroys them.
template <int N>
struct TimingEvents {
  hipEvent_t e[N] = {};
  TimingEvents() = default;
  TimingEvents(const TimingEvents &) = delete;
  ~TimingEvents() {
    for (hipEvent_t x : e)
      if (x) (void)hipEventDestroy(x);
  }
};

// ctx: any handle with a std::string err (qp_ctx, qp_verifier)
#define QP_HIP_TRY(ctx, expr)                                                    \
  do {                                                                           \
    hipError_t _e = (expr);                                                      \
    if (_e != hipSuccess) {                                                      \
      (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(_e);            \
      return _e == hipErrorOutOfMemory ? QP_ERR_OOM : QP_ERR_HIP;                \
    }                                                                            \
  } while (0)
