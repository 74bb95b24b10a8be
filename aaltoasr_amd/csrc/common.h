// common.h -- shared host-side helpers for libaasr (error state, HIP checks).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <type_traits>

#include "../../include/aasr.h"

// Environment variables.  The product library reads the few that INTEGRATION.md lists (AASR_PREC, AASR_PCGMM_AS_WRITTEN,
// AASR_WRITER_THREADS, AASR_RECIPE_TIMING and the test hooks AASR_F16_PROBE_TOL / AASR_PG_PIVOT_COST) with plain getenv.
// Every other switch is an EXPERIMENT switch -- it selects a kernel variant, a layout or an arithmetic for an A/B
// measurement -- and exists only in a build made with AASR_BUILD_ABLATION=1 (-DAASR_ABLATION=1, into lib_ablation/): in
// the product library the expression below is a null pointer and the name is not even in the object's strings
// (tests/test_env_switches.py checks exactly that).
#ifndef AASR_ABLATION
#define AASR_ABLATION 0
#endif
#if AASR_ABLATION
#define AASR_EXPERIMENT_ENV(name) getenv(name)
#else
#define AASR_EXPERIMENT_ENV(name) ((const char *)nullptr)
#endif

namespace aasr {

// thread-local message behind aasr_last_error()
std::string &last_error();
aasr_status fail(aasr_status code, const char *fmt, ...);

// Thrown inside the library, converted to a status at the C boundary.
struct Error {
  aasr_status code;
  std::string msg;
};

[[noreturn]] void raise(aasr_status code, const char *fmt, ...);

#define AASR_HIP(expr)                                                        \
  do {                                                                        \
    hipError_t _e = (expr);                                                   \
    if (_e != hipSuccess)                                                     \
      ::aasr::raise(AASR_ERR_NO_DEVICE, "%s failed: %s (%s:%d)", #expr,       \
                    hipGetErrorString(_e), __FILE__, __LINE__);               \
  } while (0)

// Runs body, maps exceptions to status codes.
template <class F>
aasr_status guarded(F &&body) {
  try {
    body();
    return AASR_OK;
  } catch (const Error &e) {
    last_error() = e.msg;
    return e.code;
  } catch (const std::exception &e) {
    last_error() = e.what();
    return AASR_ERR_INVALID;
  } catch (const std::string &s) {
    last_error() = s;
    return AASR_ERR_INVALID;
  }
}

// device buffer with RAII
template <class T>
struct DevBuf {
  T *p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  DevBuf(DevBuf &&o) noexcept : p(o.p), n(o.n) {
    o.p = nullptr;
    o.n = 0;
  }
  DevBuf &operator=(DevBuf &&o) noexcept {
    if (this != &o) {
      release();
      p = o.p;
      n = o.n;
      o.p = nullptr;
      o.n = 0;
    }
    return *this;
  }
  ~DevBuf() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
  void alloc(size_t count) {
    release();
    if (count == 0) return;
    AASR_HIP(hipMalloc((void **)&p, count * sizeof(T)));
    n = count;
  }
  void ensure(size_t count) {
    if (count > n) alloc(count);
  }
  void upload(const T *src, size_t count) {
    alloc(count);
    if (count) AASR_HIP(hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice));
  }
};

void require_device();

// Kernel instances chosen by a run-time value: f(std::integral_constant<int, N>()) for the N among Ns that equals v.
// false: v is none of them (the caller raises its own message).
template <int... Ns, class F>
bool dispatch_among(int v, F &&f) {
  return ((v == Ns && (f(std::integral_constant<int, Ns>()), true)) || ...);
}
// the padded dimensions the statistics item kernels are instantiated for
template <class F>
bool dispatch_dimp(int dimp, F &&f) {
  return dispatch_among<8, 16, 24, 32, 40, 48, 64, 96, 128, 192>(dimp, f);
}
// the 16-blocks of a padded [1, x] row the triangular tile kernels are instantiated for (d <= 127)
template <class F>
bool dispatch_pb(int pb, F &&f) {
  return dispatch_among<1, 2, 3, 4, 5, 6, 7, 8>(pb, f);
}

}  // namespace aasr
