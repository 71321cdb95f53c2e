// FrontierRegions::auction of the host mirror (frontier_regions.hpp) on a small map with fixed robots: prints the answers,
// tests/test_gpu_auction.py compares them with the restatement.  Needs a GPU.
//   map W H resolution origin_x origin_y flags max_regions n_auction min_size cells_per_robot n_steps
//   robot q x y th                                                     one line per robot
//   state final assigned rounds
//   goal q region cell cost len                                        one line per robot
//   path q t x y th                                                    one line per row
#include <cstdio>
#include <exception>

#include <ergodic_exploration/frontier_regions.hpp>

using namespace ergodic_exploration;

int main()
{
  try {
    const double res = 0.1, ox = -1.0, oy = -2.0;
    const unsigned W = 50, H = 40, P = 8, max_regions = 6, n_auction = 3, min_size = 3, cells_per_robot = 20, n_steps = 12;
    // the map of frontier_regions_tests.cpp: a wall with a door, a sealed room, an unknown patch, an unknown strip down the
    // right side that the wall's row cuts, and a one-cell hole in explored space
    GridData d(W * H, 0);
    for (unsigned i = 0; i < 30; ++i) d[i * W + 20] = 100;
    d[12 * W + 20] = 0;
    for (unsigned j = 34; j < 44; ++j) d[25 * W + j] = d[34 * W + j] = 100;
    for (unsigned i = 25; i < 35; ++i) d[i * W + 34] = d[i * W + 43] = 100;
    for (unsigned i = 3; i < 9; ++i)
      for (unsigned j = 30; j < 36; ++j) d[i * W + j] = -1;
    for (unsigned i = 0; i < H; ++i)
      for (unsigned j = 46; j < W; ++j) d[i * W + j] = -1;
    for (unsigned j = 40; j < 46; ++j) d[20 * W + j] = 100;
    d[22 * W + 5] = -1;
    const GridMap g = GridMap::fromOccupancyGrid(W, H, res, ox, oy, d);
    // three robots left of the wall, two right of it, one off the map, one inside the sealed room, one on the wall
    const double rx[P] = { -0.75, 0.45, 3.2, -5.0, 2.95, -0.35, 2.05, 1.05 }, ry[P] = { -1.85, 1.33, 1.63, 0.0, 1.05, 0.25, -1.55, -1.55 };
    mat robots(3, P);
    for (unsigned q = 0; q < P; ++q) {
      robots(0, q) = rx[q];
      robots(1, q) = ry[q];
      robots(2, q) = 0.25 * q - 0.5;
    }
    FrontierRegions frontier(0.3, 1.2, 0.1, 0.8, max_regions);
    frontier.update(g);
    const FrontierRegions::Assignment a = frontier.auction(g, robots, n_auction, min_size, cells_per_robot, n_steps, EEA_GEODESIC_UNKNOWN_BLOCKS);
    std::printf("map %u %u %.17g %.17g %.17g %u %u %u %u %u %u\n", W, H, res, ox, oy, EEA_GEODESIC_UNKNOWN_BLOCKS, max_regions, n_auction,
                min_size, cells_per_robot, n_steps);
    for (unsigned q = 0; q < P; ++q) std::printf("robot %u %.17g %.17g %.17g\n", q, robots(0, q), robots(1, q), robots(2, q));
    std::printf("state %d %u %u\n", a.final ? 1 : 0, a.assigned, a.rounds);
    for (unsigned q = 0; q < P; ++q) std::printf("goal %u %d %d %d %d\n", q, a.region[q], a.cell[q], a.cost[q], a.len[q]);
    for (unsigned q = 0; q < P; ++q) {
      for (unsigned t = 0; t < n_steps; ++t) {
        const size_t col = static_cast<size_t>(q) * n_steps + t;
        std::printf("path %u %u %.17g %.17g %.17g\n", q, t, a.path(0, col), a.path(1, col), a.path(2, col));
      }
    }
    // the same object again: nothing of the first call is left in its buffers
    const FrontierRegions::Assignment b = frontier.auction(g, robots, n_auction, min_size, cells_per_robot, n_steps, EEA_GEODESIC_UNKNOWN_BLOCKS);
    if (b.region != a.region || b.cell != a.cell || b.cost != a.cost || b.len != a.len || b.assigned != a.assigned) {
      std::fprintf(stderr, "frontier_auction_tests: a second call gave another answer\n");
      return 1;
    }
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "frontier_auction_tests: %s\n", e.what());
    return 1;
  }
}
