// tests/cpp/cpic_job_host.cpp — the arithmetic of the impulse rows of a tiled job with CPIC rigid bodies (csrc/tiled_plan.h:
// rows_table_float4, rows_extra_cap, rows_node_cap, rows_off, rows_flag_word) compiled for the host, the header alone: hand-written
// cases, then by enumeration that the row regions of both parities and both exchanges never overlap the nodes or each other, and
// that Arena(halo_cap, inbox) itself is what it was.  A program of its own (tests/test_cpic_job_cpu.py runs it under
// -fsanitize=address,undefined).
#include <cstdio>
#include <utility>
#include <vector>

#include "../../taichi_mpm_amd/csrc/tiled_plan.h"

using namespace tplan;

#define CHECK(c) do { if (!(c)) return __LINE__; } while (0)

// the numbers written out by hand
static int by_hand() {
  CHECK(IMP_ROW_FLOATS == 72 && IMP_ROW_FLOAT4 == 18 && ROW_EXCHANGES == 2 && MAX_WORLD == 64);
  CHECK(IMP_ROW_FLOATS * sizeof(float) == 288);  // the bytes of a row on the wire, per peer and exchange
  CHECK(rows_table_float4(1) == 18 && rows_table_float4(2) == 36 && rows_table_float4(8) == 144 && rows_table_float4(64) == 1152);
  CHECK(rows_extra_cap(1) == 36 && rows_extra_cap(2) == 72 && rows_extra_cap(8) == 288 && rows_extra_cap(64) == 2304);
  // a job of 8 ranks whose boxes need 1000 nodes asks for 1288; without bodies for 1000
  CHECK(rows_node_cap(1288, 8, true) == 1000 && rows_node_cap(1000, 8, false) == 1000);
  CHECK(rows_off(1288, 8, 0, 0) == 1000 && rows_off(1288, 8, 0, 7) == 1126 && rows_off(1288, 8, 1, 0) == 1144 && rows_off(1288, 8, 1, 7) == 1270);
  CHECK(rows_off(1288, 8, 1, 7) + IMP_ROW_FLOAT4 == 1288);  // the last row ends where the capacity ends
  // epoch words: behind the halo, table, record and reduction epochs of [64] each
  CHECK(rows_flag_word(0, 0) == 256 && rows_flag_word(0, 63) == 319 && rows_flag_word(1, 0) == 320 && rows_flag_word(1, 63) == 383);
  CHECK((rows_flag_word(1, 63) + 1) * sizeof(uint32_t) <= FLAG_BYTES);
  return 0;
}

// every region as bytes [begin, end) of the arena: nodes and rows of both receive buffers; none overlaps another, all inside recv[p]
static int no_overlap() {
  const int worlds[4] = {1, 2, 8, 64};
  const uint64_t node_caps[4] = {1, 1000, 25350, 2141184510ull};
  for (int wi = 0; wi < 4; wi++)
    for (int ci = 0; ci < 4; ci++) {
      const int world = worlds[wi];
      const uint64_t nodes = node_caps[ci], cap = nodes + rows_extra_cap(world);
      const Arena A(cap, 65536);
      CHECK(rows_node_cap(cap, world, true) == nodes);
      std::vector<std::pair<uint64_t, uint64_t>> reg;
      for (int par = 0; par < 2; par++) {
        reg.push_back({A.recv[par], A.recv[par] + NODE_BYTES * nodes});  // the nodes of the halo boxes
        for (int x = 0; x < ROW_EXCHANGES; x++)
          for (int r = 0; r < world; r++) {
            const uint64_t b = A.recv[par] + NODE_BYTES * rows_off(cap, world, x, r);
            reg.push_back({b, b + sizeof(float) * IMP_ROW_FLOATS});
            CHECK(b % 16 == 0);                                    // a row begins on a float4
            CHECK(b >= A.recv[par] && b + sizeof(float) * IMP_ROW_FLOATS <= A.recv[par] + A.recv_bytes);  // inside its receive buffer
          }
      }
      CHECK(A.recv[0] + A.recv_bytes <= A.recv[1] && A.recv[1] + A.recv_bytes <= A.inbox);
      for (size_t i = 0; i < reg.size(); i++)
        for (size_t j = i + 1; j < reg.size(); j++) CHECK(reg[i].second <= reg[j].first || reg[j].second <= reg[i].first);
      // the rows of one table lie back to back in rank order: the sum reads table[r * IMP_ROW_FLOATS + ...]
      for (int x = 0; x < ROW_EXCHANGES; x++)
        for (int r = 1; r < world; r++) CHECK(rows_off(cap, world, x, r) == rows_off(cap, world, x, r - 1) + IMP_ROW_FLOAT4);
    }
  // the epoch words of the two exchanges: distinct from each other and from the four arrays in front of them
  std::vector<int> seen(FLAG_BYTES / sizeof(uint32_t), 0);
  for (int k = 0; k < 4 * MAX_WORLD; k++) seen[(size_t)k] = 1;
  for (int x = 0; x < ROW_EXCHANGES; x++)
    for (int r = 0; r < MAX_WORLD; r++) {
      const uint32_t w = rows_flag_word(x, r);
      CHECK(w < seen.size() && !seen[w]);
      seen[w] = 1;
    }
  return 0;
}

// Arena(halo_cap, inbox) is the function of its two capacities it was (tests/cpp/tiled_plan_host.cpp: tp_arena, restated), and a job
// without bodies asks for the capacity it asked for before
static int arena_unchanged() {
  const Arena A(1000, 65536);
  CHECK(A.flags == 0 && A.red[0] == 4096 && A.red[1] == 12288);
  CHECK(A.table[0] == 20480 && A.table[1] == 38912 && A.table_bytes == 18432);
  CHECK(A.recv[0] == 57344 && A.recv[1] == 73472 && A.recv_bytes == 16128);
  CHECK(A.inbox == 89600 && A.inbox_bytes == 11534336 && A.total == 11623936);
  const Arena B(1000 + rows_extra_cap(8), 65536);  // the same job with bodies: 288 float4 = 4608 bytes more per receive buffer
  CHECK(B.recv[0] == A.recv[0] && B.recv_bytes == 20736 && B.recv[1] == A.recv[1] + 4608 && B.inbox == A.inbox + 9216 && B.total == A.total + 9216);
  for (int world : {1, 2, 8, 64}) CHECK(rows_node_cap(25350, world, false) == 25350);
  return 0;
}

int main() {
  int (*const all[])() = {by_hand, no_overlap, arena_unchanged};
  const char *const names[] = {"by_hand", "no_overlap", "arena_unchanged"};
  int failed = 0;
  for (size_t i = 0; i < sizeof all / sizeof all[0]; i++)
    if (const int line = all[i]()) {
      std::printf("%s: check at line %d failed\n", names[i], line);
      failed = 1;
    }
  if (!failed) std::printf("cpic_job: %zu scenarios ok\n", sizeof all / sizeof all[0]);
  return failed;
}
