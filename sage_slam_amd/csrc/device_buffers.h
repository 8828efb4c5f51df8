// device_buffers.h -- the two owners of raw HIP allocations: DevBuf (device memory) and PinnedBuf (pinned host memory the
// device reads and writes over PCIe).  Both release what they hold when they go out of scope; they move, never copy.
// Neither zeroes what it allocates.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

namespace sage_rt
{

struct DeviceMemory
{
  static hipError_t alloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
  static void free(void *p) { (void)hipFree(p); }
};
struct PinnedMemory
{
  static hipError_t alloc(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
  static void free(void *p) { (void)hipHostFree(p); }
};

template <class Memory>
struct OwnedBuf
{
  void *p = nullptr;
  size_t cap = 0;
  OwnedBuf() = default;
  OwnedBuf(const OwnedBuf &) = delete;
  OwnedBuf &operator=(const OwnedBuf &) = delete;
  OwnedBuf(OwnedBuf &&o) noexcept { swap(o); }
  OwnedBuf &operator=(OwnedBuf &&o) noexcept
  {
    OwnedBuf(std::move(o)).swap(*this); // (what this one held goes with the temporary)
    return *this;
  }
  ~OwnedBuf() { release(); }
  void swap(OwnedBuf &o) noexcept
  {
    std::swap(p, o.p);
    std::swap(cap, o.cap);
  }
  // keeps an allocation that is large enough; otherwise frees it and allocates anew (the contents are not carried over)
  int reserve(size_t bytes)
  {
    if (bytes <= cap)
      return 0;
    release();
    hipError_t e = Memory::alloc(&p, bytes);
    if (e != hipSuccess)
    {
      p = nullptr;
      return (int)e;
    }
    cap = bytes;
    return 0;
  }
  void release()
  {
    if (p)
      Memory::free(p);
    p = nullptr;
    cap = 0;
  }
  template <class T>
  T *as() const { return reinterpret_cast<T *>(p); }
};

using DevBuf = OwnedBuf<DeviceMemory>;
using PinnedBuf = OwnedBuf<PinnedMemory>;

} // namespace sage_rt
