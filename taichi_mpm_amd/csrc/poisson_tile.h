// taichi_mpm_amd/csrc/poisson_tile.h — the periodic blue-noise tiles behind mpmhip_seed_particles (D = 3) and mpmhip2d_seed_particles
// (D = 2): one generator for both (host only, no HIP, no other header of this library: tests/test_seed_cpu.py and
// tests/test_seed2d_cpu.py compile it alone).
// Restates PoissonDiskSampler<D>::write_periodic_data (src/poisson_disk_sampler.h:255-324): Bridson's algorithm in the periodic box
// [-20, 20)^D, minimum distance 1, 30 attempts per active point, the first point at the centre, a candidate drawn from the cube
// [-2, 2]^D around the active point and kept when its distance lies in [1, 2].  The reference reads the result from a file it does not
// ship ($mpm/periodic_pd_{2,3}d.dat); this library generates its own tiles, each once per process.
//
// Every machine must get the same bytes, so nothing here is floating point until the very last step: coordinates are integers in
// units of 2^-16 (the period is 40 * 2^16 = 2 621 440 units), distances are compared as exact 64-bit squares, and the generator is an
// integer one (splitmix64, a fixed seed per dimension).  A coordinate converts to fp32 exactly (22 bits, a power-of-two scale).
// tests/test_seed_cpu.py and tests/test_seed2d_cpu.py pin the count and the SHA-256 of either tile.
//
// One defect of the reference is not copied.  Its background cells have side 1 / sqrt(D) and in 3D ceil(40 sqrt(3)) = 70 of them
// cover 40.41, not 40, so wrapping the cell index skips a cell at the seam and points on both sides of the seam come closer than 1.
// Here 80 cells of side exactly 1/2 (<= 1 / sqrt(3): a cell holds at most one point, its diagonal is 0.866, 0.707 in 2D) make the
// period, the cell of a coordinate is a shift, and a 5^D neighbourhood holds every point nearer than 1 (two cells further away start
// more than 1 away).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <utility>
#include <vector>

namespace poisson_tile {

constexpr int FRAC_BITS = 16;
constexpr int64_t ONE = int64_t(1) << FRAC_BITS;   // the minimum distance
constexpr int64_t PERIOD = 40 * ONE;               // periodic_bound (src/poisson_disk_sampler.h:27)
constexpr int CELL_SHIFT = FRAC_BITS - 1;          // cells of side 1/2
constexpr int CELLS = int(PERIOD >> CELL_SHIFT);   // 80 per axis: a whole number of cells makes the period
constexpr int MAX_ATTEMPTS = 30;
constexpr uint64_t SEED[2] = {0x7a696c655f706432ull /* D = 2 */, 0x7a696c655f706433ull /* D = 3 */};

struct Rng {  // splitmix64
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
  }
};

template <int D>
struct Point { int32_t x[D]; };  // in [0, PERIOD)

template <int D>
constexpr size_t ipow(size_t b) { size_t r = 1; for (int d = 0; d < D; d++) r *= b; return r; }

template <int D>
inline size_t cell_of(const Point<D> &p) {
  size_t c = 0;
  for (int d = 0; d < D; d++) c = c * CELLS + (size_t)(p.x[d] >> CELL_SHIFT);
  return c;
}

// no sample nearer than 1 to p, across the seams of the period
template <int D>
inline bool far_enough(const Point<D> &p, const std::vector<int32_t> &grid, const std::vector<Point<D>> &samples) {
  for (size_t n = 0; n < ipow<D>(5); n++) {  // the 5^D cells around p's: digit d of n is the offset along axis d, plus 2
    size_t cell = 0, m = n;
    for (int d = 0; d < D; d++, m /= 5) cell = cell * CELLS + (size_t)(((p.x[d] >> CELL_SHIFT) + (int)(m % 5) - 2 + CELLS) % CELLS);
    const int32_t s = grid[cell];
    if (s < 0) continue;
    int64_t r2 = 0;
    for (int d = 0; d < D; d++) {
      int64_t u = (int64_t)p.x[d] - samples[s].x[d];
      if (u < 0) u = -u;
      if (u > PERIOD / 2) u = PERIOD - u;  // the nearest periodic image
      r2 += u * u;
    }
    if (r2 < ONE * ONE) return false;
  }
  return true;
}

// the tile's points in the order Bridson's algorithm created them, in fixed point (here and below: no dimension given means 3)
template <int D = 3>
inline std::vector<Point<D>> generate_fixed() {
  static_assert(D == 2 || D == 3, "a tile in the plane or in space");
  Rng rng{SEED[D - 2]};
  std::vector<int32_t> grid(ipow<D>(CELLS), -1);
  std::vector<Point<D>> samples;
  std::vector<int32_t> active;
  Point<D> centre;
  for (int d = 0; d < D; d++) centre.x[d] = int32_t(PERIOD / 2);
  samples.push_back(centre);
  active.push_back(0);
  grid[cell_of(centre)] = 0;
  while (!active.empty()) {
    const size_t pick = (size_t)(rng.next() % active.size());
    const Point<D> cur = samples[active[pick]];
    std::swap(active[pick], active.back());
    bool found = false;
    for (int attempt = 0; attempt < MAX_ATTEMPTS; attempt++) {
      // get_random_point_nearby (:78-89): uniform in the cube of half side 2, kept in the shell 1 <= r <= 2; one draw
      // per candidate, 18 bits of it per axis
      int64_t off[D], r2;
      do {
        const uint64_t w = rng.next();
        r2 = 0;
        for (int d = 0; d < D; d++) {
          off[d] = (int64_t)((w >> (21 * d)) & 0x3ffffu) - 2 * ONE;  // 18 bits: [-2, 2) in steps of 2^-16
          r2 += off[d] * off[d];
        }
      } while (r2 < ONE * ONE || r2 > 4 * ONE * ONE);
      Point<D> q;
      for (int d = 0; d < D; d++) q.x[d] = (int32_t)(((int64_t)cur.x[d] + off[d] + PERIOD) % PERIOD);
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

// the tile as the seeding call reads it: D floats per point in [-20, 20), the centre point (all zero) first
template <int D = 3>
inline std::vector<float> generate() {
  const std::vector<Point<D>> s = generate_fixed<D>();
  std::vector<float> out(s.size() * D);
  for (size_t i = 0; i < s.size(); i++)
    for (int d = 0; d < D; d++) out[D * i + d] = (float)(s[i].x[d] - PERIOD / 2) * (1.0f / (float)ONE);
  return out;
}

// generated once per process
template <int D = 3>
inline const std::vector<float> &tile() {
  static const std::vector<float> t = generate<D>();
  return t;
}

}  // namespace poisson_tile
