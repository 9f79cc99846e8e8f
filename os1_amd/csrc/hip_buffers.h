// hip_buffers.h -- the host-side helpers every matcher-side file needs: the HIP error check, grow-only device and page-locked
// buffers, the scratch a file keeps on a handle, the arena alignment and the wait for a kernel's completion word.
// (orbfe_extractor.hip keeps buffers of its own: its page-locked ones are hipHostMallocDefault, a different thing.)
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <cstddef>
#include <memory>

#include "../../include/orbfe.h"

namespace orbfe {
void set_err(const char* fmt, ...);
}

#define HIP_TRY(expr)                                                                               \
  do {                                                                                              \
    hipError_t e_ = (expr);                                                                         \
    if (e_ != hipSuccess) {                                                                         \
      orbfe::set_err("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__);    \
      return ORBFE_ERR_HIP;                                                                         \
    }                                                                                               \
  } while (0)

namespace orbfe {

// Grow-only buffers.  An owner whose device may not be current when it dies calls release() itself after hipSetDevice; the
// destructor then finds nothing to free.
template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  int ensure(size_t count) {
    if (count <= n) return ORBFE_OK;
    release();
    HIP_TRY(hipMalloc((void**)&p, count * sizeof(T)));
    n = count;
    return ORBFE_OK;
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
};
template <class T>
struct PinBuf {
  T* p = nullptr;
  size_t n = 0;
  PinBuf() = default;
  PinBuf(const PinBuf&) = delete;
  PinBuf& operator=(const PinBuf&) = delete;
  ~PinBuf() { release(); }
  int ensure(size_t count) {
    if (count <= n) return ORBFE_OK;
    release();
    // Coherent (fine-grained, uncached on the GPU side) EXPLICITLY: kernels store results and completion words here and the
    // host polls them while the kernel runs; with hipHostMallocDefault that property would hang on HIP_HOST_COHERENT.
    HIP_TRY(hipHostMalloc((void**)&p, count * sizeof(T), hipHostMallocCoherent));
    n = count;
    return ORBFE_OK;
  }
  void release() { if (p) (void)hipHostFree(p); p = nullptr; n = 0; }
};

// A file's scratch (buffers, events, counters of its own) kept in a slot of the handle that outlives its calls: made on
// first use, destroyed with the handle -- whose destructor makes the device current first.  One slot holds one type.
template <class T>
T* scratch_in(std::shared_ptr<void>& slot) {
  if (!slot) slot = std::make_shared<T>();
  return static_cast<T*>(slot.get());
}

// parts of an upload arena start on 256-byte boundaries
inline size_t al(size_t v) { return (v + 255) & ~(size_t)255; }

// wait until *word == seq (the kernel's release store), polling for at most 2 ms, then on the stream
inline int wait_for_word(const volatile int* word, int seq, hipStream_t st, bool poll = true) {
  bool seen = false;
  if (poll) {
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned spin = 1;; spin++) {
      if (*word == seq) { seen = true; break; }
      if ((spin & 255u) == 0 && std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() > 2.0) break;
      __builtin_ia32_pause();
    }
    std::atomic_thread_fence(std::memory_order_acquire);
  }
  if (!seen) HIP_TRY(hipStreamSynchronize(st));
  return ORBFE_OK;
}

}  // namespace orbfe
using orbfe::al;
using orbfe::DevBuf;
using orbfe::PinBuf;
using orbfe::scratch_in;
using orbfe::wait_for_word;
