// Host test of csrc/devbuf.h against the fake allocation calls of tests/stubs_hip (tests/test_devbuf.py compiles and runs it):
// exit status 0 and "devbuf ok" when every property holds, otherwise the failed line.
#include <stdio.h>
#include <string.h>

#include "devbuf.h"

static int failures = 0;
#define CHECK(x) do { if (!(x)) { printf("line %d: %s\n", __LINE__, #x); failures++; } } while (0)

int main() {
  fake_hip::State &s = fake_hip::state();
  for (int kind = 0; kind < 2; kind++) {
    DevBuf b;
    b.kind = kind ? DevBuf::PINNED : DevBuf::DEVICE;
    const int a0 = s.allocs, f0 = s.frees;
    // first allocation: nothing to free
    CHECK(b.reserve(100) == hipSuccess && b.p && b.cap == 100 && s.allocs == a0 + 1 && s.frees == f0);
    CHECK(s.live[kind].count(b.p) == 1 && s.live[1 - kind].empty());
    memset(b.p, 0xAB, 100);
    // within capacity: no call at all, same pointer
    void *p0 = b.p;
    CHECK(b.reserve(100) == hipSuccess && b.reserve(1) == hipSuccess && b.reserve(0) == hipSuccess);
    CHECK(b.p == p0 && b.cap == 100 && s.allocs == a0 + 1 && s.frees == f0);
    // growing: exactly one free and one allocation
    CHECK(b.reserve(101) == hipSuccess && b.p && b.cap == 101 && s.allocs == a0 + 2 && s.frees == f0 + 1);
    CHECK(s.live[kind].size() == 1 && s.live[kind].count(b.p) == 1);
    // a failed allocation leaves the buffer empty, not the freed pointer with the old capacity ...
    s.fail_at = 1;
    CHECK(b.reserve(1000) != hipSuccess);
    CHECK(b.p == nullptr && b.cap == 0 && s.live[kind].empty() && s.frees == f0 + 2 && s.allocs == a0 + 2);
    // ... so the next, smaller request allocates afresh
    CHECK(b.reserve(50) == hipSuccess && b.p && b.cap == 50 && s.allocs == a0 + 3 && s.frees == f0 + 2 && s.live[kind].count(b.p) == 1);
    memset(b.p, 0xCD, 50);
    // release twice frees once
    CHECK(b.release() == hipSuccess && b.p == nullptr && b.cap == 0 && s.frees == f0 + 3);
    CHECK(b.release() == hipSuccess && s.frees == f0 + 3 && s.bad_frees == 0);
    // and an empty buffer can be used again
    CHECK(b.reserve(8) == hipSuccess && b.cap == 8 && b.release() == hipSuccess);
  }
  // a set of buffers of both kinds, some grown, one failed, one never used: releasing all of them leaves nothing live, frees nothing twice
  {
    DevBuf set[6];
    set[4].kind = set[5].kind = DevBuf::PINNED;
    for (int i = 0; i < 5; i++) CHECK(set[i].reserve(16 * (i + 1)) == hipSuccess);
    CHECK(set[1].reserve(4096) == hipSuccess && set[4].reserve(4096) == hipSuccess);
    s.fail_at = 1;
    CHECK(set[2].reserve(1 << 20) != hipSuccess && set[2].p == nullptr);
    CHECK(s.live[0].size() == 3 && s.live[1].size() == 1);
    for (int pass = 0; pass < 2; pass++) for (DevBuf &b : set) CHECK(b.release() == hipSuccess);
    CHECK(s.live[0].empty() && s.live[1].empty() && s.bad_frees == 0 && s.allocs == s.frees);
  }
  if (!failures) printf("devbuf ok\n");
  return failures ? 1 : 0;
}
