// tests/cpp/tiled_recut_host.cpp — the host-only rules of re-cutting a running job (taichi_mpm_amd/csrc/tiled_plan.h: balanced_cuts,
// round_quotas, rounds_needed, capacity_check, split_recut_table) compiled by g++ with no HIP header.  As a shared library the entry
// points below are held against the Python model by tests/test_tiled_recut_cpu.py; as a program (main) the scenarios run under
// AddressSanitizer and UBSan on seeded random inputs and check the rules' own invariants.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../taichi_mpm_amd/csrc/tiled_plan.h"

extern "C" {

void tr_balanced_cuts(int res, int parts, const int64_t *hist, int *cuts) { tplan::balanced_cuts(res, parts, hist, cuts); }
int64_t tr_round_quotas(int world, const int64_t *left, const uint32_t *room, int64_t *q) { return tplan::round_quotas(world, left, room, q); }
int64_t tr_rounds_needed(int world, const int64_t *counts, const uint32_t *room) { return tplan::rounds_needed(world, counts, room); }
// out = {rank (-1: all fit), its count after the move, the excess}
void tr_capacity(int world, const int64_t *counts, const int64_t *live, const int64_t *cap, int64_t out[3]) {
  const tplan::Growth g = tplan::capacity_check(world, counts, live, cap);
  out[0] = g.rank; out[1] = g.need; out[2] = g.excess;
}
int64_t tr_live_after(int world, const int64_t *counts, const int64_t *live, int r) { return tplan::live_after(world, counts, live, r); }
int tr_row_words() { return (int)tplan::ROW; }
void tr_split(uint32_t *h, int world, int64_t *live, int64_t *cap) { tplan::split_recut_table(h, world, live, cap); }

}  // extern "C"

namespace {

struct Rng {
  uint64_t s;
  uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
  int range(int lo, int hi) { return lo + (int)(next() % (uint32_t)(hi - lo + 1)); }  // inclusive
};
#define CHECK(x) do { if (!(x)) return __LINE__; } while (0)

// cuts of random histograms: start at 0, end at res, strictly increase; a balanced histogram is balanced; the empty one splits evenly
int sc_cuts() {
  Rng R{1};
  for (int it = 0; it < 3000; it++) {
    const int parts = R.range(1, 16), res = R.range(parts, 512), kind = R.range(0, 4);
    std::vector<int64_t> h((size_t)res, 0);
    if (kind == 1) h[(size_t)R.range(0, res - 1)] = R.range(1, 100000);
    if (kind == 2) h[(size_t)res - 1] = R.range(1, 100000);
    if (kind == 3) for (int c = 0; c < R.range(1, 5); c++) { const int a = R.range(0, res - 1), w = R.range(1, 20); for (int i = a; i < std::min(res, a + w); i++) h[(size_t)i] += R.range(1, 1000); }
    if (kind == 4) for (auto &v : h) v = R.range(0, 50);
    std::vector<int> cuts((size_t)parts + 1, -7);
    tplan::balanced_cuts(res, parts, h.data(), cuts.data());
    CHECK(cuts[0] == 0 && cuts[(size_t)parts] == res);
    for (int k = 0; k < parts; k++) CHECK(cuts[(size_t)k] < cuts[(size_t)k + 1]);
    if (kind == 0) for (int k = 1; k < parts; k++) CHECK(cuts[(size_t)k] == (int)((int64_t)res * k / parts));
  }
  const int64_t flat[8] = {5, 5, 5, 5, 5, 5, 5, 5};
  int cuts[5];
  tplan::balanced_cuts(8, 4, flat, cuts);
  CHECK(cuts[1] == 2 && cuts[2] == 4 && cuts[3] == 6);
  const int64_t gap[10] = {9, 0, 0, 0, 0, 0, 0, 9, 0, 0};  // two clusters: the cut in the middle of the empty stretch
  tplan::balanced_cuts(10, 2, gap, cuts);
  CHECK(cuts[0] == 0 && cuts[1] == 4 && cuts[2] == 10);
  return 0;
}

// the round rule on random tables: quotas within room and within what is left, sources in ascending order, the rounds end within
// max over dst of ceil(arrivals / room), every "rank" gets the same quotas from the same table
int sc_rounds() {
  Rng R{2};
  for (int it = 0; it < 400; it++) {
    const int world = R.range(2, 16);
    const size_t n = (size_t)world * world;
    std::vector<int64_t> left(n), q(n), q2(n);
    std::vector<uint32_t> room((size_t)world);
    for (auto &v : room) v = (uint32_t)R.range(1, 10000);
    for (int r = 0; r < world; r++)
      for (int s = 0; s < world; s++) left[(size_t)r * world + s] = r == s || R.range(0, 2) == 0 ? 0 : R.range(0, 100000);
    int64_t bound = 0;
    for (int s = 0; s < world; s++) {
      int64_t arr = 0;
      for (int r = 0; r < world; r++) arr += left[(size_t)r * world + s];
      bound = std::max(bound, (arr + room[(size_t)s] - 1) / room[(size_t)s]);
    }
    if (bound > 5000) continue;  // (a tiny inbox against 10^5 records: the same rule, only more rounds than a test should walk)
    CHECK(tplan::rounds_needed(world, left.data(), room.data()) <= bound);
    int64_t rounds = 0;
    for (;;) {
      int64_t todo = 0;
      for (int64_t v : left) todo += v;
      if (!todo) break;
      const int64_t moved = tplan::round_quotas(world, left.data(), room.data(), q.data());
      CHECK(moved > 0 && moved == tplan::round_quotas(world, left.data(), room.data(), q2.data()) && q == q2);
      for (int s = 0; s < world; s++) {
        int64_t sum = 0;
        bool full = false;
        for (int r = 0; r < world; r++) {
          const int64_t v = q[(size_t)r * world + s], l = left[(size_t)r * world + s];
          CHECK(v >= 0 && v <= l);
          CHECK(!full || v == 0);             // behind a source that was cut short nobody is served
          if (v < l) full = true;
          sum += v;
        }
        CHECK(sum <= (int64_t)room[(size_t)s]);
        CHECK(!full || sum == (int64_t)room[(size_t)s]);  // a source is cut short only by a full inbox
      }
      for (size_t i = 0; i < n; i++) left[i] -= q[i];
      rounds++;
      CHECK(rounds <= bound);
    }
  }
  const int64_t stuck[4] = {0, 3, 0, 0};
  const uint32_t none[2] = {5, 0};
  CHECK(tplan::rounds_needed(2, stuck, none) == -1);
  return 0;
}

// the capacity rule on tables written out by hand, and the two words a redistribution's table carries beside a migration's
int sc_capacity() {
  // 3 ranks: 0 sends 40 to 1 and 10 to 2; 1 sends 5 to 0; 2 sends nothing
  const int64_t counts[9] = {0, 40, 10, 5, 0, 0, 0, 0, 0};
  const int64_t live[3] = {100, 50, 20};
  CHECK(tplan::live_after(3, counts, live, 0) == 55 && tplan::live_after(3, counts, live, 1) == 85 && tplan::live_after(3, counts, live, 2) == 30);
  const int64_t fits[3] = {55, 85, 30}, one[3] = {100, 84, 64}, two[3] = {100, 60, 25};
  CHECK(tplan::capacity_check(3, counts, live, fits).rank == -1);
  tplan::Growth g = tplan::capacity_check(3, counts, live, one);
  CHECK(g.rank == 1 && g.need == 85 && g.excess == 1);
  g = tplan::capacity_check(3, counts, live, two);  // two ranks too small: the first is reported
  CHECK(g.rank == 1 && g.need == 85 && g.excess == 25);
  const int world = 3;
  std::vector<uint32_t> h((size_t)tplan::ROW * world, 0);
  for (int r = 0; r < world; r++) {
    uint32_t *row = &h[(size_t)r * tplan::ROW];
    for (int s = 0; s < world; s++) row[s] = s == r ? (uint32_t)live[r] : (uint32_t)counts[r * 3 + s];
    row[world + 6] = 1000u + (uint32_t)r; row[world + 7] = 77u;
  }
  int64_t l[3], c[3];
  tplan::split_recut_table(h.data(), world, l, c);
  tplan::Mig M;
  M.decode(h.data(), world, 1);
  for (int r = 0; r < world; r++) {
    CHECK(l[r] == live[r] && c[r] == 1000 + r && M.room[(size_t)r] == 77u);
    for (int s = 0; s < world; s++) CHECK(M.count(r, s) == counts[r * 3 + s]);
  }
  CHECK(M.total == 55 && M.n_out == 5 && M.n_in == 40 && M.speed == 0.0f);
  return 0;
}

}  // namespace

int main() {
  int (*const scenarios[])() = {sc_cuts, sc_rounds, sc_capacity};
  const char *const names[] = {"sc_cuts", "sc_rounds", "sc_capacity"};
  for (int i = 0; i < 3; i++) {
    const int line = scenarios[i]();
    if (line) { printf("%s failed at line %d\n", names[i], line); return 1; }
  }
  printf("scenarios ok\n");
  return 0;
}
