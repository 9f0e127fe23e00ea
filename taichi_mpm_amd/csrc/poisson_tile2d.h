// taichi_mpm_amd/csrc/poisson_tile2d.h — the periodic blue-noise tile behind mpmhip2d_seed_particles (host only, no HIP, no other
// header of this library: tests/test_seed2d_cpu.py compiles it alone).
// Restates PoissonDiskSampler<2>::write_periodic_data (src/poisson_disk_sampler.h:255-324) with the design of poisson_tile.h, one axis
// fewer: Bridson's algorithm in the periodic box [-20, 20)^2, minimum distance 1, 30 attempts per active point, the first point at the
// centre, a candidate drawn from the square [-2, 2]^2 around the active point and kept when its distance lies in [1, 2].  The
// reference reads the result from a file it does not ship ($mpm/periodic_pd_2d.dat); this library generates its own, once per process.
//
// Every machine must get the same bytes: coordinates are integers in units of 2^-16 (the period is 40 * 2^16 units), distances are
// compared as exact 64-bit squares, the generator is splitmix64 with a fixed seed of its own.  A coordinate converts to fp32 exactly.
// 80 x 80 background cells of side exactly 1/2 (<= 1 / sqrt(2): a cell holds at most one point, its diagonal is 0.707) make the period,
// the cell of a coordinate is a shift, and a 5 x 5 neighbourhood holds every point nearer than 1.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <utility>
#include <vector>

namespace poisson_tile2d {

constexpr int FRAC_BITS = 16;
constexpr int64_t ONE = int64_t(1) << FRAC_BITS;   // the minimum distance
constexpr int64_t PERIOD = 40 * ONE;               // periodic_bound (src/poisson_disk_sampler.h:27)
constexpr int CELL_SHIFT = FRAC_BITS - 1;          // cells of side 1/2
constexpr int CELLS = int(PERIOD >> CELL_SHIFT);   // 80 per axis: a whole number of cells makes the period
constexpr int MAX_ATTEMPTS = 30;
constexpr uint64_t SEED = 0x7a696c655f706432ull;

struct Rng {  // splitmix64
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
  }
};

struct Point { int32_t x[2]; };  // in [0, PERIOD)

inline int cell_of(const Point &p) { return (p.x[0] >> CELL_SHIFT) * CELLS + (p.x[1] >> CELL_SHIFT); }

// no sample nearer than 1 to p, across the seams of the period
inline bool far_enough(const Point &p, const std::vector<int32_t> &grid, const std::vector<Point> &samples) {
  int c[2];
  for (int d = 0; d < 2; d++) c[d] = p.x[d] >> CELL_SHIFT;
  for (int i = -2; i <= 2; i++)
    for (int j = -2; j <= 2; j++) {
      const int a = (c[0] + i + CELLS) % CELLS, b = (c[1] + j + CELLS) % CELLS;
      const int32_t s = grid[(size_t)a * CELLS + b];
      if (s < 0) continue;
      int64_t r2 = 0;
      for (int d = 0; d < 2; d++) {
        int64_t u = (int64_t)p.x[d] - samples[s].x[d];
        if (u < 0) u = -u;
        if (u > PERIOD / 2) u = PERIOD - u;  // the nearest periodic image
        r2 += u * u;
      }
      if (r2 < ONE * ONE) return false;
    }
  return true;
}

// the tile's points in the order Bridson's algorithm created them, in fixed point
inline std::vector<Point> generate_fixed() {
  Rng rng{SEED};
  std::vector<int32_t> grid((size_t)CELLS * CELLS, -1);
  std::vector<Point> samples;
  std::vector<int32_t> active;
  const Point centre = {{int32_t(PERIOD / 2), int32_t(PERIOD / 2)}};
  samples.push_back(centre);
  active.push_back(0);
  grid[cell_of(centre)] = 0;
  while (!active.empty()) {
    const size_t pick = (size_t)(rng.next() % active.size());
    const Point cur = samples[active[pick]];
    std::swap(active[pick], active.back());
    bool found = false;
    for (int attempt = 0; attempt < MAX_ATTEMPTS; attempt++) {
      // get_random_point_nearby (:78-89): uniform in the square of half side 2, kept in the ring 1 <= r <= 2
      int64_t off[2], r2;
      do {
        const uint64_t w = rng.next();
        r2 = 0;
        for (int d = 0; d < 2; d++) {
          off[d] = (int64_t)((w >> (21 * d)) & 0x3ffffu) - 2 * ONE;  // 18 bits: [-2, 2) in steps of 2^-16
          r2 += off[d] * off[d];
        }
      } while (r2 < ONE * ONE || r2 > 4 * ONE * ONE);
      Point q;
      for (int d = 0; d < 2; d++) q.x[d] = (int32_t)(((int64_t)cur.x[d] + off[d] + PERIOD) % PERIOD);
      if (grid[cell_of(q)] >= 0 || !far_enough(q, grid, samples)) continue;
      found = true;
      const int32_t index = (int32_t)samples.size();
      samples.push_back(q);
      active.push_back(index);
      grid[cell_of(q)] = index;
    }
    if (!found) active.pop_back();
  }
  return samples;
}

// the tile as the seeding call reads it: 2 floats per point in [-20, 20), the centre point (0, 0) first
inline std::vector<float> generate() {
  const std::vector<Point> s = generate_fixed();
  std::vector<float> out(s.size() * 2);
  for (size_t i = 0; i < s.size(); i++)
    for (int d = 0; d < 2; d++) out[2 * i + d] = (float)(s[i].x[d] - PERIOD / 2) * (1.0f / (float)ONE);
  return out;
}

// generated once per process
inline const std::vector<float> &tile() {
  static const std::vector<float> t = generate();
  return t;
}

}  // namespace poisson_tile2d
