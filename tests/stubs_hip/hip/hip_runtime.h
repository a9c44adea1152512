// Stand-in for <hip/hip_runtime.h> (TEST INFRASTRUCTURE ONLY, tests/host/devbuf_main.cpp): the four allocation calls csrc/devbuf.h uses,
// over malloc, with book-keeping the test reads: live allocations, addresses freed twice or never handed out, and an allocation
// that fails on request.
#pragma once
#include <stddef.h>
#include <stdlib.h>
#include <set>

typedef int hipError_t;
#define hipSuccess 0
#define hipErrorOutOfMemory 2
#define hipErrorInvalidValue 1

namespace fake_hip {
struct State {
  std::set<void *> live[2];          // [0] device, [1] pinned
  std::set<void *> freed;            // remembered (and the memory held until exit: no address comes back), so a second free shows
  int allocs = 0, frees = 0, bad_frees = 0;
  int fail_at = 0;                   // the n-th allocation from now fails (1 = the next one); 0: none
  ~State() { for (void *p : freed) free(p); }
};
inline State &state() { static State s; return s; }
inline hipError_t alloc(int kind, void **p, size_t bytes) {
  State &s = state();
  if (s.fail_at > 0 && --s.fail_at == 0) { *p = (void *)0x1;  return hipErrorOutOfMemory; }      // (a failed call may leave rubbish behind)
  *p = malloc(bytes ? bytes : 1);
  s.live[kind].insert(*p); s.allocs++;
  return hipSuccess;
}
inline hipError_t release(int kind, void *p) {
  State &s = state();
  if (!s.live[kind].erase(p)) { s.bad_frees++; return hipErrorInvalidValue; }      // freed twice, never allocated, or by the wrong call
  s.freed.insert(p); s.frees++;
  return hipSuccess;
}
}  // namespace fake_hip

inline hipError_t hipMalloc(void **p, size_t bytes) { return fake_hip::alloc(0, p, bytes); }
inline hipError_t hipFree(void *p) { return fake_hip::release(0, p); }
inline hipError_t hipHostMalloc(void **p, size_t bytes) { return fake_hip::alloc(1, p, bytes); }
inline hipError_t hipHostFree(void *p) { return fake_hip::release(1, p); }
