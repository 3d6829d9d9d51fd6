// Ownership of what the C-ABI layer takes from the HIP runtime: device buffers, pinned host buffers, events and streams.
// An Owned records every resource it hands out and gives all of them back in release() (its destructor calls it); the
// pointers and handles it writes into the caller's structs are views that nothing else frees. Host-only; no kernel sees it.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstring>
#include <mutex>
#include <vector>

namespace rh {

// Resources held by every Owned of the process together (rebvio_hip_test_live_resources): +1 per buffer, event or stream
// handed out, -1 per one given back. Touched only where a resource is created or destroyed.
inline std::atomic<long> g_live_resources{0};

class Owned {
 public:
  Owned() = default;
  Owned(const Owned&) = delete;
  Owned& operator=(const Owned&) = delete;
  Owned(Owned&& o) noexcept { held_.swap(o.held_); }
  Owned& operator=(Owned&& o) noexcept {
    if (this != &o) {
      release();
      held_.swap(o.held_);
    }
    return *this;
  }
  ~Owned() { release(); }

  // count elements of T in device memory; fill_byte >= 0: followed by a hipMemset of the whole buffer (which, like every
  // hipMemset, may still be running on the null stream when this returns).
  // The size follows the declared type of *out: changing a field's type changes its allocation. Where the size is not
  // count * sizeof(T) (paddings, a struct behind a byte pointer), use the _bytes form.
  template <class T>
  hipError_t device(T** out, size_t count, int fill_byte = -1) {
    return device_bytes(out, count * sizeof(T), fill_byte);
  }
  template <class T>
  hipError_t device_bytes(T** out, size_t bytes, int fill_byte = -1) {
    std::lock_guard<std::mutex> lk(mu_);
    if (!room()) return hipErrorOutOfMemory;
    void* p = nullptr;
    const hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) return e;
    keep(kDevice, p);
    *out = static_cast<T*>(p);
    return fill_byte >= 0 ? hipMemset(p, fill_byte, bytes) : hipSuccess;
  }
  // count elements of T in pinned host memory, zeroed on request
  template <class T>
  hipError_t pinned(T** out, size_t count, bool zero) {
    return pinned_bytes(out, count * sizeof(T), zero);
  }
  template <class T>
  hipError_t pinned_bytes(T** out, size_t bytes, bool zero) {
    std::lock_guard<std::mutex> lk(mu_);
    if (!room()) return hipErrorOutOfMemory;
    void* p = nullptr;
    const hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocDefault);
    if (e != hipSuccess) return e;
    keep(kPinned, p);
    if (zero) std::memset(p, 0, bytes);
    *out = static_cast<T*>(p);
    return hipSuccess;
  }
  hipError_t event(hipEvent_t* out) {
    std::lock_guard<std::mutex> lk(mu_);
    if (!room()) return hipErrorOutOfMemory;
    hipEvent_t ev{};
    const hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (e != hipSuccess) return e;
    keep(kEvent, ev);
    *out = ev;
    return hipSuccess;
  }
  hipError_t stream(hipStream_t* out, unsigned flags, int priority = 0) {  // (0: the default priority)
    std::lock_guard<std::mutex> lk(mu_);
    if (!room()) return hipErrorOutOfMemory;
    hipStream_t s{};
    const hipError_t e = hipStreamCreateWithPriority(&s, flags, priority);
    if (e != hipSuccess) return e;
    keep(kStream, s);
    *out = s;
    return hipSuccess;
  }

  // gives one device buffer back early and nulls the view
  template <class T>
  void drop(T** p) {
    std::lock_guard<std::mutex> lk(mu_);
    for (size_t i = 0; i < held_.size(); ++i)
      if (held_[i].kind == kDevice && held_[i].h == static_cast<void*>(*p)) {
        give_back(held_[i]);
        held_.erase(held_.begin() + (std::ptrdiff_t)i);
        break;
      }
    *p = nullptr;
  }

  // gives everything back, newest first; a second call finds nothing left to do
  void release() {
    std::lock_guard<std::mutex> lk(mu_);
    for (size_t i = held_.size(); i-- > 0;) give_back(held_[i]);
    std::vector<Held>().swap(held_);
  }

 private:
  enum Kind { kDevice, kPinned, kEvent, kStream };
  struct Held {
    Kind kind;
    void* h;
  };
  // Makes room for one more entry before the resource is taken (mu_ held from here to keep()), so that keep() cannot
  // throw with a resource in hand: nothing leaks and no exception leaves a C entry point.
  bool room() noexcept {
    if (held_.size() < held_.capacity()) return true;
    try {
      held_.reserve(held_.size() + 64);
    } catch (...) {
      return false;
    }
    return true;
  }
  void keep(Kind k, void* h) noexcept {  // (mu_ held, room() made)
    held_.push_back({k, h});
    g_live_resources.fetch_add(1, std::memory_order_relaxed);
  }
  static void give_back(const Held& r) {
    switch (r.kind) {
      case kDevice: (void)hipFree(r.h); break;
      case kPinned: (void)hipHostFree(r.h); break;
      case kEvent: (void)hipEventDestroy(static_cast<hipEvent_t>(r.h)); break;
      case kStream: (void)hipStreamDestroy(static_cast<hipStream_t>(r.h)); break;
    }
    g_live_resources.fetch_sub(1, std::memory_order_relaxed);
  }
  // Buffers allocated on first use are taken by entries of different thread rules (the pinned ring by the acquisition thread, a
  // pair's counters and the cloud scratch by the tracking thread): the list has a lock of its own. Nothing on a per-frame or
  // per-pair path takes it - only a creation or a destruction does.
  std::mutex mu_;
  std::vector<Held> held_;
};

}  // namespace rh
