// batch_host.hpp — the host round trip of one batched call, shared by the batched solve (nos_batch.hip), the batched
// registrations (register_host.hpp) and the score batch (nos_score.hip): what goes up through the slot's pinned block,
// one pooled device block for the whole call, what comes down, one synchronisation.  The callers keep what
// is theirs: which sections they declare, their descriptors, their launches, the copy into the caller's arrays.
#pragma once

#include "nos_internal.hpp"

namespace nosd {

// section()…, open(), fill host<>() of the up sections, send(), launch, launched(), fetch(), close(), read host<>() of the
// down sections.  Every step after open() may be skipped on a failure: close() — the destructor if the caller returns
// before it — waits for the stream and only then gives the block back to the pool.
class BatchTrip {
 public:
  enum Dir { kUp = 0, kDown = 1, kDeviceOnly = 2 };  // host → device, device → host, never copied; the block's order
  struct Section {
    Dir dir;
    size_t offset;  // within its direction
  };

  explicit BatchTrip(DeviceSlot& slot) : slot_(slot) {}
  BatchTrip(const BatchTrip&) = delete;
  BatchTrip& operator=(const BatchTrip&) = delete;
  ~BatchTrip() { settle(); }

  // `bytes` of the block, 256-byte aligned.  Before open(): where a direction starts follows from the ones before it.
  Section section(Dir dir, size_t bytes) {
    const Section s{dir, bytes_[dir]};
    bytes_[dir] += (bytes + 255) & ~size_t(255);
    return s;
  }

  // The pinned block grown to up + down (grows only; freed with the context), one pool_alloc of up + down + device-only.
  int open() {
    const size_t pinned_total = bytes_[kUp] + bytes_[kDown];
    NOS_HIP_CHECK(hipSetDevice(slot_.device));
    if (slot_.batch_pinned_bytes < pinned_total) {
      if (slot_.batch_pinned != nullptr) (void)hipHostFree(slot_.batch_pinned);
      slot_.batch_pinned = nullptr;
      slot_.batch_pinned_bytes = 0;
      NOS_HIP_CHECK(hipHostMalloc(&slot_.batch_pinned, pinned_total, hipHostMallocDefault));
      NOS_HIP_CHECK(debug_fill(slot_, slot_.batch_pinned, pinned_total, /*host=*/true));
      slot_.batch_pinned_bytes = pinned_total;
    }
    void* dev = nullptr;
    const int rc = pool_alloc(slot_, pinned_total + bytes_[kDeviceOnly], &dev, &dev_capacity_);
    if (rc == NOS_OK) dev_ = static_cast<unsigned char*>(dev);
    return rc;
  }

  template <typename T>
  T* host(Section s) const {  // up and down sections only
    return reinterpret_cast<T*>(static_cast<unsigned char*>(slot_.batch_pinned) + start(s));
  }
  template <typename T>
  T* dev(Section s) const {
    return reinterpret_cast<T*>(dev_ + start(s));
  }

  // The first HIP failure of the trip is the one close() reports; → whether the trip is still good.
  bool check(hipError_t e) {
    if (e_ == hipSuccess) e_ = e;
    return e_ == hipSuccess;
  }
  bool send() { return check(hipMemcpyAsync(dev_, slot_.batch_pinned, bytes_[kUp], hipMemcpyHostToDevice, slot_.stream)); }
  bool launched() { return check(hipGetLastError()); }
  bool fetch() {
    return check(hipMemcpyAsync(static_cast<unsigned char*>(slot_.batch_pinned) + bytes_[kUp], dev_ + bytes_[kUp], bytes_[kDown],
                                hipMemcpyDeviceToHost, slot_.stream));
  }

  // → the trip's status; a failure reads "<what> failed: <HIP's text>".
  int close(const char* what) {
    settle();
    return e_ == hipSuccess ? NOS_OK : hip_fail(e_, what);
  }

 private:
  void settle() {
    if (dev_ == nullptr) return;  // never opened, or closed already
    check(hipStreamSynchronize(slot_.stream));  // before the buffer goes back to the pool, after a failure too
    pool_release(slot_, dev_, dev_capacity_);
    dev_ = nullptr;
  }
  size_t start(Section s) const {
    return (s.dir > kUp ? bytes_[kUp] : 0) + (s.dir > kDown ? bytes_[kDown] : 0) + s.offset;
  }
  DeviceSlot& slot_;
  size_t bytes_[3] = {0, 0, 0};
  unsigned char* dev_ = nullptr;
  size_t dev_capacity_ = 0;
  hipError_t e_ = hipSuccess;
};

}  // namespace nosd
