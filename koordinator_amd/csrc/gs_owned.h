// gs_owned.h — move-only owners of the HIP resources the host side holds: a device buffer, a pinned host buffer, an
// event and a stream. The allocating call returns the hipError_t of the HIP call it makes, reset() releases, and so
// does the destructor; these are the only callers of hipFree, hipHostFree, hipEventDestroy and hipStreamDestroy.
// A raw pointer beside an owner is a view into its allocation.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

namespace gs {

// The part the four owners share: a handle H (null = nothing held) released by Release. Move-only: the move
// operations below leave no copy operations.
template <class H, void (*Release)(H)>
class Owned {
 public:
  Owned() = default;
  Owned(Owned&& o) noexcept : h_(std::exchange(o.h_, H{})) {}
  Owned& operator=(Owned&& o) noexcept {
    if (this != &o) {
      reset();
      h_ = std::exchange(o.h_, H{});
    }
    return *this;
  }
  ~Owned() { reset(); }
  H get() const { return h_; }
  explicit operator bool() const { return h_ != H{}; }
  void reset() {
    if (h_ != H{}) Release(h_);
    h_ = H{};
  }

 protected:
  H h_{};
};

inline void release_device(void* p) { (void)hipFree(p); }
inline void release_pinned(void* p) { (void)hipHostFree(p); }
inline void release_event(hipEvent_t e) { (void)hipEventDestroy(e); }
inline void release_stream(hipStream_t s) { (void)hipStreamDestroy(s); }

// alloc() first releases what the buffer held (a re-allocation site waits for the device work that used it first)
template <class T>
class DevBuf : public Owned<void*, release_device> {
 public:
  hipError_t alloc(size_t bytes) {
    reset();
    return hipMalloc(&h_, bytes);
  }
  T* get() const { return static_cast<T*>(h_); }
};

template <class T>
class PinnedBuf : public Owned<void*, release_pinned> {
 public:
  hipError_t alloc(size_t bytes) {
    reset();
    return hipHostMalloc(&h_, bytes, hipHostMallocDefault);
  }
  T* get() const { return static_cast<T*>(h_); }
};

class Event : public Owned<hipEvent_t, release_event> {
 public:
  hipError_t create(unsigned flags = hipEventDefault) {
    reset();
    return hipEventCreateWithFlags(&h_, flags);
  }
};

class Stream : public Owned<hipStream_t, release_stream> {
 public:
  hipError_t create(unsigned flags) {
    reset();
    return hipStreamCreateWithFlags(&h_, flags);
  }
  hipError_t create(unsigned flags, int priority) {
    reset();
    return hipStreamCreateWithPriority(&h_, flags, priority);
  }
};

}  // namespace gs
