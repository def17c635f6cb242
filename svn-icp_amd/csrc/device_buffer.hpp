// device_buffer.hpp — host-only: the owning handles (device buffer, pinned block, stream, event) and the one error path of
// the three objects of the C ABI (svnicp_ctx, svnicp_map, svnicp_prep).  Every handle frees in its destructor and cannot be
// copied: an object is torn down by `delete` alone, once its device is bound and its streams have drained.  Members are
// destroyed in reverse order of declaration: declare streams BEFORE the buffers.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <string>

#include "../../include/svnicp_hip.h"

namespace svnicp_host {

struct NoCopy {
  NoCopy() = default;
  NoCopy(const NoCopy&) = delete;
  NoCopy& operator=(const NoCopy&) = delete;
};

// Exact: allocate what is asked (svnicp_ctx).  Half: half as much again whenever an existing buffer must grow (map and
// pre-processor: sizes follow the scans, and a hipFree + hipMalloc per call costs more than the kernels of a query)
enum class Growth { Exact, Half };

template <typename T, Growth G = Growth::Exact>
struct DevBuf : NoCopy {
  T* p = nullptr;
  size_t cap = 0;  // elements
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {   // the source is left empty
    if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
    return *this;
  }
  ~DevBuf() { release(); }
  hipError_t ensure(size_t n) {
    if (n <= cap && p) return hipSuccess;
    if (G == Growth::Half && cap > 0) n += n / 2;
    release();
    if (n == 0) n = 1;
    const hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), n * sizeof(T));
    if (e == hipSuccess) cap = n;
    return e;
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};
template <typename T> using GrowBuf = DevBuf<T, Growth::Half>;

// pinned host block of exactly n elements (alloc replaces what was there)
template <typename T>
struct PinnedBuf : NoCopy {
  T* p = nullptr;
  size_t cap = 0;  // elements
  ~PinnedBuf() { release(); }
  hipError_t alloc(size_t n) {
    release();
    const hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&p), n * sizeof(T), hipHostMallocDefault);
    if (e == hipSuccess) cap = n;
    return e;
  }
  void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
};

struct Stream : NoCopy {
  hipStream_t s = nullptr;
  ~Stream() { if (s) (void)hipStreamDestroy(s); }
  hipError_t create(unsigned int flags) { return hipStreamCreateWithFlags(&s, flags); }
  operator hipStream_t() const { return s; }
};

struct Event : NoCopy {
  hipEvent_t e = nullptr;
  Event() = default;
  Event(Event&& o) noexcept : e(o.e) { o.e = nullptr; }
  ~Event() { if (e) (void)hipEventDestroy(e); }
  hipError_t create(unsigned int flags = hipEventDefault) { return hipEventCreateWithFlags(&e, flags); }
  operator hipEvent_t() const { return e; }
};

// the error path: the message goes into the object's own `err`, or — no object yet — into its type's creation-error string
// (Obj::create_error(), thread_local), which svnicp_*_last_error(nullptr) returns
template <typename Obj>
int fail(Obj* o, int code, const std::string& msg) {
  if (o) o->err = msg; else Obj::create_error() = msg;
  return code;
}
#define HIPCHK(obj, expr)                                                                                  \
  do {                                                                                                     \
    const hipError_t _e = (expr);                                                                          \
    if (_e != hipSuccess)                                                                                  \
      return svnicp_host::fail((obj), _e == hipErrorOutOfMemory ? SVNICP_ERR_NOMEM : SVNICP_ERR_HIP,      \
                               std::string(#expr) + ": " + hipGetErrorString(_e));                         \
  } while (0)

}  // namespace svnicp_host
using svnicp_host::fail;   // the three objects are global-namespace structs
using svnicp_host::GrowBuf;
