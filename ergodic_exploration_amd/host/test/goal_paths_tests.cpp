// GoalPaths::go of the host mirror (goal_paths.hpp) on a fixed map with fixed robots and goals: prints the answers,
// tests/test_gpu_goto.py compares them with the restatement.  Needs a GPU.
//   map W H resolution origin_x origin_y flags margin n_steps
//   row v ...                                                          one line per row of the map, W cell values
//   robot q x y th goal                                                one line per robot
//   state ok window cut_off refused
//   answer q cost status len                                           one line per robot
//   path q t x y th                                                    one line per row
#include <cstdio>
#include <exception>

#include <ergodic_exploration/goal_paths.hpp>

using namespace ergodic_exploration;

int main()
{
  try {
    const double res = 0.1, ox = -1.0, oy = -2.0;
    const unsigned W = 200, H = 100, P = 10, margin = 3, n_steps = 12;  // (20000 cells: the whole map is past the cap)
    // a wall with a door, an unknown patch that blocks, and open space
    GridData d(W * H, 0);
    for (unsigned i = 0; i < 30; ++i) d[i * W + 20] = 100;
    d[12 * W + 20] = 0;
    for (unsigned i = 3; i < 9; ++i)
      for (unsigned j = 30; j < 36; ++j) d[i * W + j] = -1;
    const GridMap g = GridMap::fromOccupancyGrid(W, H, res, ox, oy, d);
    // (row, column) of the robots and of their goals; robot 3 is off the map, robot 7 stands on the wall
    const int rc[P][2] = { { 5, 5 }, { 10, 10 }, { 25, 10 }, { 0, 0 }, { 40, 50 }, { 2, 2 }, { 50, 100 }, { 3, 20 }, { 5, 5 }, { 5, 28 } };
    const int gc[P][2] = { { 5, 15 }, { 14, 30 }, { 25, 30 }, { 5, 5 }, { 0, 0 }, { 99, 199 }, { 50, 100 }, { 5, 5 }, { 3, 20 }, { 5, 38 } };
    mat robots(3, P);
    std::vector<int> goals(P);
    for (unsigned q = 0; q < P; ++q) {
      robots(0, q) = ox + (rc[q][1] + 0.5) * res;
      robots(1, q) = oy + (rc[q][0] + 0.5) * res;
      robots(2, q) = 0.25 * q - 0.5;
      goals[q] = gc[q][0] * static_cast<int>(W) + gc[q][1];
    }
    robots(0, 3) = -5.0;
    goals[4] = -1;
    GoalPaths paths(0.3, 1.2, 0.1, 0.8);
    const GoalPaths::Paths a = paths.go(g, robots, goals, margin, n_steps, nullptr, 0, EEA_GEODESIC_UNKNOWN_BLOCKS);
    std::printf("map %u %u %.17g %.17g %.17g %u %u %u\n", W, H, res, ox, oy, EEA_GEODESIC_UNKNOWN_BLOCKS, margin, n_steps);
    for (unsigned i = 0; i < H; ++i) {
      std::printf("row");
      for (unsigned j = 0; j < W; ++j) std::printf(" %d", static_cast<int>(d[i * W + j]));
      std::printf("\n");
    }
    for (unsigned q = 0; q < P; ++q) std::printf("robot %u %.17g %.17g %.17g %d\n", q, robots(0, q), robots(1, q), robots(2, q), goals[q]);
    std::printf("state %u %u %u %u\n", a.ok, a.window, a.cut_off, a.refused);
    for (unsigned q = 0; q < P; ++q) std::printf("answer %u %d %d %d\n", q, a.cost[q], a.status[q], a.len[q]);
    for (unsigned q = 0; q < P; ++q) {
      for (unsigned t = 0; t < n_steps; ++t) {
        const size_t col = static_cast<size_t>(q) * n_steps + t;
        std::printf("path %u %u %.17g %.17g %.17g\n", q, t, a.path(0, col), a.path(1, col), a.path(2, col));
      }
    }
    // the same object again, with fewer robots and steps and then the first call's: nothing is left in its buffers
    mat two(3, 2);
    for (unsigned r = 0; r < 3; ++r) {
      two(r, 0) = robots(r, 1);
      two(r, 1) = robots(r, 2);
    }
    const GoalPaths::Paths s = paths.go(g, two, { goals[1], goals[2] }, margin, 2, nullptr, 0, EEA_GEODESIC_UNKNOWN_BLOCKS);
    const GoalPaths::Paths b = paths.go(g, robots, goals, margin, n_steps, nullptr, 0, EEA_GEODESIC_UNKNOWN_BLOCKS);
    if (s.cost[0] != a.cost[1] || s.status[1] != a.status[2] || s.len[0] != 2 || b.cost != a.cost || b.status != a.status ||
        b.len != a.len || b.ok != a.ok) {
      std::fprintf(stderr, "goal_paths_tests: a second call gave another answer\n");
      return 1;
    }
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "goal_paths_tests: %s\n", e.what());
    return 1;
  }
}
