// tests/cpp/async_store_host.cpp — the host's arithmetic over the container store of a resident asynchronous stepper
// (taichi_mpm_amd/csrc/async_sched.h: AsyncStoreCount), the header alone compiled for the host: what a read-back means, when the
// store is compacted, how far it grows.  A stand-alone program (tests/test_async_store_cpu.py builds it under ASan + UBSan).
#include "../../taichi_mpm_amd/csrc/async_sched.h"

#include <cstdio>
#include <cstdlib>

using mpm::AsyncStoreCount;

static int cases = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    cases++;                                                            \
    if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); exit(1); } \
  } while (0)

static AsyncStoreCount store(uint32_t cap, uint32_t size, uint32_t live) {
  AsyncStoreCount s;
  s.cap = cap; s.size = s.size_ub = size; s.live = live;
  return s;
}

int main() {
  {  // counter folds: appends join the live containers, frees leave them, the cursor is the size and its bound
    AsyncStoreCount s;
    s.fold(100, 0, 100);
    CHECK(s.live == 100 && s.size == 100 && s.size_ub == 100);
    s.size_ub = 150;  // (an advance filed up to 50 more)
    s.fold(40, 30, 140);
    CHECK(s.live == 110 && s.size == 140 && s.size_ub == 140);
    s.fold(0, 110, 140);
    CHECK(s.live == 0 && s.size == 140);
    s.fold(5, 9, 145);  // n_freed > live: the count stops at zero, it does not wrap
    CHECK(s.live == 0 && s.size == 145 && s.size_ub == 145);
    s.fold(3, 1000, 148);  // (the appends of the same read-back are counted first)
    CHECK(s.live == 0);
    s.fold(0xffffffffu, 0, 0xffffffffu);
    CHECK(s.live == 0xffffffffu && s.size == 0xffffffffu);
  }
  {  // first clause: dead > live + 65536, whatever the room
    CHECK(!store(1u << 20, 200000, 67232).wants_compaction(0));   // dead 132768 = live + 65536
    CHECK(store(1u << 20, 200000, 67231).wants_compaction(0));    // dead 132769 = live + 65537
    CHECK(!store(1u << 20, 65536, 0).wants_compaction(0));
    CHECK(store(1u << 20, 65537, 0).wants_compaction(0));
    CHECK(!store(0xffffffffu, 0xffffffffu, 0xfffffff0u).wants_compaction(0));  // (live + 65536 is formed in 64 bits)
    CHECK(!store(4096, 100, 200).wants_compaction(0));  // live above the size (a fold yet to come): no dead containers
  }
  {  // second clause: the incoming containers do not fit AND more than a quarter of the store is dead
    CHECK(!store(4096, 4000, 2999).wants_compaction(96));   // fits exactly (4096): no
    CHECK(store(4096, 4000, 2999).wants_compaction(97));    // one too many, dead 1001 > 1000
    CHECK(!store(4096, 4000, 3000).wants_compaction(97));   // dead 1000 = size / 4: no
    CHECK(!store(4096, 4000, 3000).wants_compaction(5000));
    CHECK(store(4096, 4001, 3000).wants_compaction(96));    // 4097 > 4096, dead 1001 > 1000
    CHECK(!store(0xffffffffu, 0xfffffff0u, 0xbffffff0u).wants_compaction(0xfu));  // fits exactly (2^32 - 1); dead = 2^30 < live + 65536
    CHECK(store(0xffffffffu, 0xfffffff0u, 0xbffffff0u).wants_compaction(0x20u));  // size + incoming passes 2^32: formed in 64 bits
  }
  {  // growth of the store: half as much again, 4096 at the least, never past 2^32 - 1 (and never below the need)
    CHECK(AsyncStoreCount::grown(0) == 4096 && AsyncStoreCount::grown(1) == 4096);
    CHECK(AsyncStoreCount::grown(2730) == 4096 && AsyncStoreCount::grown(2731) == 4096 && AsyncStoreCount::grown(2732) == 4098);
    CHECK(AsyncStoreCount::grown(4095) == 6142 && AsyncStoreCount::grown(4096) == 6144);
    CHECK(AsyncStoreCount::grown(2863311530u) == 4294967295u);  // 2^32 / 1.5: need + need / 2 = 2^32 - 1
    CHECK(AsyncStoreCount::grown(2863311531u) == 4294967295u);  // the first need whose half-again passes 2^32
    CHECK(AsyncStoreCount::grown(0xfffffffeu) == 0xffffffffu && AsyncStoreCount::grown(0xffffffffu) == 0xffffffffu);
    for (uint32_t need : {0u, 1u, 4095u, 4096u, 2863311530u, 2863311531u, 0xfffffffeu, 0xffffffffu}) CHECK(AsyncStoreCount::grown(need) >= need);
    CHECK(AsyncStoreCount::sum(1, 2) == 3 && AsyncStoreCount::sum(0xfffffff0u, 0x10u) == 0xffffffffu && AsyncStoreCount::sum(0xffffffffu, 0xffffffffu) == 0xffffffffu);
  }
  {  // one dedup word per creation id handed out, half as many again and 1024
    CHECK(AsyncStoreCount::ids_grown(0) == 1024 && AsyncStoreCount::ids_grown(1) == 1025 && AsyncStoreCount::ids_grown(4096) == 7168);
    CHECK(AsyncStoreCount::ids_grown(0x7fffffffull) == 0x7fffffffull + 0x3fffffffull + 1024);
  }
  printf("%d cases ok\n", cases);
  return 0;
}
