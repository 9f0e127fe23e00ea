// tests/cpp/host_mem_host.cpp — taichi_mpm_amd/csrc/host_mem.h (DevBuf / PinnedBuf) on the host, without the HIP runtime: the six
// runtime functions the header calls are defined HERE over malloc, count their calls, keep the set of live arrays (a release of
// anything else is a double free) and can be told to fail the n-th allocation.  Every scenario returns 0 or the line of the first
// check that failed; tests/test_host_mem_cpu.py runs them.
#include "../../taichi_mpm_amd/csrc/host_mem.h"

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <set>

namespace {
struct Fake {
  std::set<void *> live[2];  // [0] device, [1] pinned
  long allocs = 0, frees = 0, bad_frees = 0, memsets = 0, memcpys = 0;
  long fail_at = 0;  // fail the fail_at-th allocation from now (1 = the next); 0 = never
} F;

hipError_t fake_alloc(int kind, void **p, size_t bytes) {
  if (F.fail_at && --F.fail_at == 0) { *p = nullptr; return hipErrorOutOfMemory; }
  *p = std::malloc(bytes ? bytes : 1);
  std::memset(*p, 0xCD, bytes);  // (a fresh array is NOT zero: zero-fill has to come from hipMemset)
  F.live[kind].insert(*p);
  F.allocs++;
  return hipSuccess;
}
hipError_t fake_free(int kind, void *p) {
  if (!p) return hipSuccess;
  if (!F.live[kind].erase(p)) { F.bad_frees++; return hipErrorInvalidValue; }
  std::free(p);
  F.frees++;
  return hipSuccess;
}
long live_total() { return (long)(F.live[0].size() + F.live[1].size()); }
}  // namespace

extern "C" {
hipError_t hipMalloc(void **p, size_t bytes) { return fake_alloc(0, p, bytes); }
hipError_t hipFree(void *p) { return fake_free(0, p); }
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned int) { return fake_alloc(1, p, bytes); }
hipError_t hipHostFree(void *p) { return fake_free(1, p); }
hipError_t hipMemset(void *dst, int value, size_t bytes) { F.memsets++; std::memset(dst, value, bytes); return hipSuccess; }
hipError_t hipMemcpy(void *dst, const void *src, size_t bytes, hipMemcpyKind) { F.memcpys++; std::memcpy(dst, src, bytes); return hipSuccess; }
}

#define CHECK(cond) do { if (!(cond)) return __LINE__; } while (0)
// what every scenario ends on: the counter agrees with the fake's own set, nothing was released twice, every allocation was released
#define BALANCED() CHECK(hostmem::g_live_buffers.load() == 0 && live_total() == 0 && F.bad_frees == 0 && F.allocs == F.frees)

template <class B>
static int release_once() {
  F = Fake();
  {
    B a;
    CHECK(!a && a.get() == nullptr);
    CHECK(a.alloc(10) == hipSuccess && a && hostmem::g_live_buffers.load() == 1 && live_total() == 1);
  }  // destruction
  CHECK(F.allocs == 1 && F.frees == 1);
  B b;
  CHECK(b.alloc(4) == hipSuccess);
  b.reset();
  CHECK(!b && F.frees == 2 && hostmem::g_live_buffers.load() == 0);
  b.reset();  // (of an empty buffer: nothing)
  CHECK(F.frees == 2);
  CHECK(b.alloc(4) == hipSuccess);
  auto *first = b.get();
  CHECK(b.alloc(8) == hipSuccess);  // over a held buffer: the old array goes first
  CHECK(F.allocs == 4 && F.frees == 3 && !F.live[0].count(first) && !F.live[1].count(first));
  CHECK(hostmem::g_live_buffers.load() == 1 && live_total() == 1);
  b.reset();
  BALANCED();
  return 0;
}

template <class B>
static int failed_alloc() {
  F = Fake();
  B a;
  F.fail_at = 1;
  CHECK(a.alloc(16) != hipSuccess && !a && hostmem::g_live_buffers.load() == 0 && live_total() == 0);
  CHECK(a.alloc(16) == hipSuccess);
  F.fail_at = 1;
  CHECK(a.alloc(32) != hipSuccess);  // alloc releases what it held first: on failure the buffer holds nothing
  CHECK(!a && hostmem::g_live_buffers.load() == 0 && live_total() == 0);
  BALANCED();
  return 0;
}

template <class B>
static int regrow_cases() {
  F = Fake();
  {
    B a;
    CHECK(a.regrow(0, 6, true) == hipSuccess);  // from nothing: an allocation, zero-filled
    for (int i = 0; i < 6; i++) CHECK(a[i] == 0);
    for (int i = 0; i < 6; i++) a[i] = 100 + i;
    auto *old = a.get();
    F.fail_at = 1;
    CHECK(a.regrow(6, 12, true) != hipSuccess);  // failed: the old array and its contents stay
    CHECK(a.get() == old && hostmem::g_live_buffers.load() == 1 && live_total() == 1);
    for (int i = 0; i < 6; i++) CHECK(a[i] == 100 + i);
    CHECK(a.regrow(4, 12, true) == hipSuccess);  // the first `keep` elements, zeros behind them, the old array released
    CHECK(a.get() != old && !F.live[0].count(old) && !F.live[1].count(old));
    CHECK(hostmem::g_live_buffers.load() == 1 && live_total() == 1);
    for (int i = 0; i < 4; i++) CHECK(a[i] == 100 + i);
    for (int i = 4; i < 12; i++) CHECK(a[i] == 0);
    const long sets = F.memsets;
    CHECK(a.regrow(2, 5, false) == hipSuccess);  // not asked to zero: no memset, the kept elements still arrive
    CHECK(F.memsets == sets && a[0] == 100 && a[1] == 101);
    const long copies = F.memcpys;
    CHECK(a.regrow(0, 3, false) == hipSuccess);  // keep = 0: nothing is copied
    CHECK(F.memcpys == copies);
  }
  BALANCED();
  return 0;
}

template <class B>
static int move_and_swap() {
  F = Fake();
  {
    B a, b;
    CHECK(a.alloc(3) == hipSuccess && b.alloc(5) == hipSuccess);
    auto *pa = a.get(), *pb = b.get();
    std::swap(a, b);
    CHECK(a.get() == pb && b.get() == pa && F.frees == 0 && hostmem::g_live_buffers.load() == 2);
    B c(std::move(a));  // move construction leaves the source empty
    CHECK(!a && c.get() == pb && F.frees == 0);
    b = std::move(c);  // move assignment releases what the target held
    CHECK(!c && b.get() == pb && F.frees == 1 && !F.live[0].count(pa) && !F.live[1].count(pa));
    B &self = b;
    b = std::move(self);  // onto itself: nothing happens
    CHECK(b.get() == pb && F.frees == 1);
    B arr[2];  // the record sets of a ctx are swapped as array elements too
    CHECK(arr[0].alloc(2) == hipSuccess);
    std::swap(arr[0], arr[1]);
    CHECK(!arr[0] && arr[1]);
  }
  BALANCED();
  return 0;
}

static int kinds_do_not_mix() {  // a DevBuf goes back through hipFree, a PinnedBuf through hipHostFree, both count in one counter
  F = Fake();
  {
    DevBuf<uint8_t> d;
    PinnedBuf<uint8_t> h;
    CHECK(d.alloc(7) == hipSuccess && h.alloc(7) == hipSuccess);
    CHECK(F.live[0].count(d.get()) && F.live[1].count(h.get()) && hostmem::g_live_buffers.load() == 2);
    uint8_t *raw = d;  // the implicit conversion
    CHECK(raw == d.get() && d + 1 == raw + 1);
  }
  BALANCED();
  return 0;
}

extern "C" {
int hm_release_once(int pinned) { return pinned ? release_once<PinnedBuf<int>>() : release_once<DevBuf<int>>(); }
int hm_failed_alloc(int pinned) { return pinned ? failed_alloc<PinnedBuf<int>>() : failed_alloc<DevBuf<int>>(); }
int hm_regrow(int pinned) { return pinned ? regrow_cases<PinnedBuf<int>>() : regrow_cases<DevBuf<int>>(); }
int hm_move_and_swap(int pinned) { return pinned ? move_and_swap<PinnedBuf<int>>() : move_and_swap<DevBuf<int>>(); }
int hm_kinds_do_not_mix(void) { return kinds_do_not_mix(); }
long hm_live(void) { return (long)hostmem::g_live_buffers.load(); }
}
