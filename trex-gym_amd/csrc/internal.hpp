// Shared by the translation units of libtrex_hip.so (not installed, not part of the C-ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "host_tables.hpp"

// last-error plumbing of trex_last_error(): sets the thread-local message, returns `code`
int trex_fail(int code, const std::string &msg);

// caller allocations already validated as memory of a device (base address, bytes known to be good)
struct TrexSeen { const void *p; size_t bytes; };
int trex_check_device_buffer(int device, std::vector<TrexSeen> &seen, const void *p, size_t bytes, const char *what);

// a mirror table (include/trex_symmetry.h, capi_symmetry.cpp) as another unit's launch reads it: its device words, width and device
struct TrexMirrorTable;
const uint32_t *trex_mirror_table_words(const TrexMirrorTable *table, int *width, int *device);

struct TrexDeviceGuard {
  int prev = -1;
  bool ok;
  explicit TrexDeviceGuard(int dev) {
    ok = hipGetDevice(&prev) == hipSuccess && (prev == dev || hipSetDevice(dev) == hipSuccess);
    if (prev == dev) prev = -1;
  }
  ~TrexDeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// One device allocation and its owner: move-only, freed by the destructor under the device it was made on. Every allocation a handle
// owns is a DeviceBuf member of the handle (or an element of the batch's `state`), so that an error path frees by returning.
struct DeviceBuf {
  void *p = nullptr;
  size_t bytes = 0;
  int device = 0;
  DeviceBuf() = default;
  DeviceBuf(DeviceBuf &&o) noexcept : p(o.p), bytes(o.bytes), device(o.device) { o.p = nullptr; o.bytes = 0; }
  DeviceBuf &operator=(DeviceBuf &&o) noexcept {   // frees what it held
    if (this != &o) { release(); p = o.p; bytes = o.bytes; device = o.device; o.p = nullptr; o.bytes = 0; }
    return *this;
  }
  ~DeviceBuf() { release(); }
  void release() {
    if (!p) return;
    TrexDeviceGuard guard(device);
    (void)hipFree(p);
    p = nullptr; bytes = 0;
  }
  // `n` bytes on the CURRENT device (the caller holds a DeviceGuard), zeroed if asked; frees what it held first
  hipError_t alloc(size_t n, bool zero) {
    release();
    hipError_t e = hipGetDevice(&device);
    if (e == hipSuccess) e = hipMalloc(&p, n);
    if (e != hipSuccess) { p = nullptr; return e; }
    bytes = n;
    return zero ? hipMemset(p, 0, n) : hipSuccess;
  }
  template <class T> T *as() const { return (T *)p; }
  explicit operator bool() const { return p != nullptr; }
};

inline int fail(int code, const std::string &msg) { return trex_fail(code, msg); }
inline int hip_fail(hipError_t e, const char *what) { return fail(TREX_E_HIP, std::string(what) + ": " + hipGetErrorString(e)); }
#define HIP_TRY(expr)                                  \
  do {                                                 \
    hipError_t _e = (expr);                            \
    if (_e != hipSuccess) return hip_fail(_e, #expr);  \
  } while (0)
// a caller's buffer `p` as memory of the device of the handle `h` - a batch or a policy: either has `device` and the cache `seen`
// (trex_check_device_buffer)
#define BUF_TRY(h, p, bytes, what)                                                                               \
  do {                                                                                                           \
    if (int _c = trex_check_device_buffer((h)->device, (h)->seen, (p), (size_t)(bytes), (what))) return _c;      \
  } while (0)

// runs a table builder, a layout or a check of host_tables.cpp: its refusal - message and code - becomes the call's
template <class F> int built(F &&build) {
  try {
    build();
    return TREX_OK;
  } catch (const trex::Refusal &r) {
    return fail(r.code, r.what());
  }
}

// the member at byte `offset` of a state allocation, as a layout of host_tables.cpp places it
template <class T> T *member_at(const DeviceBuf &buf, size_t offset) { return (T *)(buf.as<char>() + offset); }
