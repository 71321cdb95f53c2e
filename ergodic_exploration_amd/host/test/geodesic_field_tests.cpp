// GeodesicField of the host mirror (geodesic_field.hpp) on two small maps, fixed sources and fixed poses: prints the answers,
// tests/test_gpu_geodesic.py compares them with the restatement.  Needs a GPU.
//   map n W H resolution origin_x origin_y clear_sq flags sources      the map (cells: see below), what the update was given
//   source n x y                                                       one line per source pose
//   geo n i c...                                                       the field, one line per row
//   pose n q x y th reachable cost len                                 one line per looked-up pose
//   way n q t x y th                                                   its n_steps way-points
#include <cstdio>
#include <exception>
#include <vector>

#include <ergodic_exploration/geodesic_field.hpp>

using namespace ergodic_exploration;

namespace
{
constexpr unsigned kSteps = 12;

void report(unsigned n, GeodesicField& field, const GridMap& g, unsigned W, unsigned H, double res, double ox, double oy,
            const mat& sources, const DistanceField* distance, int clear_sq, unsigned flags)
{
  field.update(g, sources, distance, clear_sq, flags);
  std::printf("map %u %u %u %.17g %.17g %.17g %d %u %u\n", n, W, H, res, ox, oy, distance ? clear_sq : -1, flags, field.sources());
  for (unsigned q = 0; q < sources.n_cols(); ++q) std::printf("source %u %.17g %.17g\n", n, sources(0, q), sources(1, q));
  std::vector<int> geo(W * H);
  hip_check(hipMemcpy(geo.data(), field.costs(), sizeof(int) * W * H, hipMemcpyDeviceToHost));
  for (unsigned i = 0; i < H; ++i) {
    std::printf("geo %u %u", n, i);
    for (unsigned j = 0; j < W; ++j) std::printf(" %d", geo[i * W + j]);
    std::printf("\n");
  }
  const unsigned NX = 9, NY = 7, P = NX * NY;
  mat poses(3, P);
  for (unsigned a = 0; a < NY; ++a) {
    for (unsigned b = 0; b < NX; ++b) {  // from outside the map to outside it
      poses(0, a * NX + b) = ox - 0.13 + (W * res + 0.3) * b / (NX - 1);
      poses(1, a * NX + b) = oy - 0.11 + (H * res + 0.3) * a / (NY - 1);
      poses(2, a * NX + b) = 0.1 * a - 0.2 * b;
    }
  }
  const std::vector<bool> reach = field.reachable(poses);
  const std::vector<int> cost = field.cost(poses);
  const GeodesicField::Walk w = field.path(poses, kSteps);
  for (unsigned q = 0; q < P; ++q) {
    std::printf("pose %u %u %.17g %.17g %.17g %d %d %d\n", n, q, poses(0, q), poses(1, q), poses(2, q), reach[q] ? 1 : 0, cost[q],
                w.len[q]);
    for (unsigned t = 0; t < kSteps; ++t) {
      std::printf("way %u %u %u %.17g %.17g %.17g\n", n, q, t, w.path(0, q * kSteps + t), w.path(1, q * kSteps + t),
                  w.path(2, q * kSteps + t));
    }
  }
}
}  // namespace

int main()
{
  try {
    const double res = 0.1, ox = -1.0, oy = -2.0;
    GeodesicField field(0.3, 1.2, 0.1, 0.8);
    // map 0: 50 x 40 (more than one tile), a wall with a door, a sealed room, unknown cells that block, the 79 / 80 pair
    {
      const unsigned W = 50, H = 40;
      GridData d(W * H, 0);
      for (unsigned i = 0; i < 30; ++i) d[i * W + 20] = 100;
      d[12 * W + 20] = 0;
      for (unsigned j = 34; j < 44; ++j) d[25 * W + j] = d[34 * W + j] = 100;
      for (unsigned i = 25; i < 35; ++i) d[i * W + 34] = d[i * W + 43] = 100;
      for (unsigned i = 3; i < 9; ++i)
        for (unsigned j = 30; j < 36; ++j) d[i * W + j] = -1;
      d[36 * W + 5] = 80;
      d[37 * W + 5] = 79;
      const GridMap g = GridMap::fromOccupancyGrid(W, H, res, ox, oy, d);
      mat src(3, 3);
      const double sx[3] = { -0.75, 3.2, -5.0 }, sy[3] = { -1.85, 1.6, 0.0 };  // two on the map, one off it
      for (unsigned q = 0; q < 3; ++q) {
        src(0, q) = sx[q];
        src(1, q) = sy[q];
        src(2, q) = 0.0;
      }
      report(0, field, g, W, H, res, ox, oy, src, nullptr, 0, EEA_GEODESIC_UNKNOWN_BLOCKS);
    }
    // map 1: 21 x 17 (smaller: the buffers are reused), inflated by the distance field: a corridor of two cells closes
    {
      const unsigned W = 21, H = 17;
      GridData d(W * H, 0);
      for (unsigned j = 0; j < W; ++j) d[8 * W + j] = 100;
      d[8 * W + 4] = d[8 * W + 5] = 0;                       // two cells wide
      for (unsigned j = 12; j < 17; ++j) d[8 * W + j] = 0;   // five cells wide
      const GridMap g = GridMap::fromOccupancyGrid(W, H, res, ox, oy, d);
      DistanceField distance(0.3, 1.2, 0.1, 0.8);
      distance.update(g);
      mat src(3, 1);
      src(0, 0) = ox + 2.5 * res;
      src(1, 0) = oy + 2.5 * res;
      src(2, 0) = 0.0;
      report(1, field, g, W, H, res, ox, oy, src, &distance, 1, 0);
    }
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "geodesic_field_tests: %s\n", e.what());
    return 1;
  }
}
