// devbuf.h — one allocation of the engine's host side (engine.hip) and its owner: device memory or pinned host memory, grown on
// demand and never shrunk.  Uses nothing of HIP beyond the four allocation calls, so the host tests compile it against a stub.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

struct DevBuf {
  enum Kind { DEVICE, PINNED };
  void *p = nullptr;
  size_t cap = 0;            // bytes
  Kind kind = DEVICE;
  // at least `bytes` of capacity.  A failed allocation leaves the buffer EMPTY (null, capacity 0), never the freed pointer with the
  // old capacity: the next, smaller request allocates afresh instead of passing the capacity check
  hipError_t reserve(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    hipError_t rc = release();
    if (rc != hipSuccess) return rc;
    rc = kind == PINNED ? hipHostMalloc(&p, bytes) : hipMalloc(&p, bytes);
    if (rc != hipSuccess) { p = nullptr; return rc; }
    cap = bytes;
    return hipSuccess;
  }
  hipError_t release() {
    void *q = p;
    p = nullptr; cap = 0;
    if (!q) return hipSuccess;
    return kind == PINNED ? hipHostFree(q) : hipFree(q);
  }
};
