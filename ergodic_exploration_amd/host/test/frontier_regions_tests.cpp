// FrontierRegions of the host mirror (frontier_regions.hpp) on a small map with fixed robots: prints the answers,
// tests/test_gpu_frontier.py compares them with the restatement.  Needs a GPU.
//   map W H resolution origin_x origin_y flags max_regions min_size    the map (cells: see below), what the calls were given
//   weights w_size w_cost
//   robot q x y th                                                     one line per robot
//   state n kept members
//   record r sum_i sum_j entry_cell entry_cost root size i_min i_max j_min j_max entry_owner reserved
//   root i c... / region i c...                                        the two planes, one line per row
//   at i j root region                                                 rootAt / regionAt of a few cells
//   goal q cell region score                                           one line per robot
//   len q n                                                            the path to the goal: moves written
#include <cstdio>
#include <exception>
#include <vector>

#include <ergodic_exploration/frontier_regions.hpp>

using namespace ergodic_exploration;

int main()
{
  try {
    const double res = 0.1, ox = -1.0, oy = -2.0, w_size = 1.0, w_cost = 0.125;
    const unsigned W = 50, H = 40, P = 5, max_regions = 3, min_size = 2, n_steps = 64;
    // 50 x 40 (more than one tile): a wall with a door, a sealed room, an unknown patch, an unknown strip down the right side
    // that the wall's row cuts, and a one-cell hole in explored space
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
    // two robots left of the wall, one right of it, one off the map, one inside the sealed room
    const double rx[P] = { -0.75, 0.45, 3.2, -5.0, 2.95 }, ry[P] = { -1.85, 1.33, 1.63, 0.0, 1.05 };
    mat robots(3, P);
    for (unsigned q = 0; q < P; ++q) {
      robots(0, q) = rx[q];
      robots(1, q) = ry[q];
      robots(2, q) = 0.25 * q - 0.5;
    }
    GeodesicPartition part(0.3, 1.2, 0.1, 0.8);
    part.update(g, robots, nullptr, 0, EEA_GEODESIC_UNKNOWN_BLOCKS);
    FrontierRegions frontier(0.3, 1.2, 0.1, 0.8, max_regions);
    frontier.update(g, &part);
    std::printf("map %u %u %.17g %.17g %.17g %u %u %u\n", W, H, res, ox, oy, EEA_GEODESIC_UNKNOWN_BLOCKS, max_regions, min_size);
    std::printf("weights %.17g %.17g\n", w_size, w_cost);
    for (unsigned q = 0; q < P; ++q) std::printf("robot %u %.17g %.17g %.17g\n", q, robots(0, q), robots(1, q), robots(2, q));
    std::printf("state %u %zu %u\n", frontier.count(), frontier.regions().size(), frontier.members());
    for (size_t r = 0; r < frontier.regions().size(); ++r) {
      const eea_frontier_region& e = frontier.regions()[r];
      std::printf("record %zu %llu %llu %d %d %d %u %d %d %d %d %d %d\n", r, static_cast<unsigned long long>(e.sum_i),
                  static_cast<unsigned long long>(e.sum_j), e.entry_cell, e.entry_cost, e.root, e.size, e.i_min, e.i_max, e.j_min,
                  e.j_max, e.entry_owner, e.reserved);
    }
    std::vector<int> plane(W * H);
    const char* const names[2] = { "root", "region" };
    for (int k = 0; k < 2; ++k) {
      hip_check(hipMemcpy(plane.data(), k == 0 ? frontier.roots() : frontier.ranks(), sizeof(int) * W * H, hipMemcpyDeviceToHost));
      for (unsigned i = 0; i < H; ++i) {
        std::printf("%s %u", names[k], i);
        for (unsigned j = 0; j < W; ++j) std::printf(" %d", plane[i * W + j]);
        std::printf("\n");
      }
    }
    const unsigned probe[4][2] = { { 0, 0 }, { 2, 30 }, { 22, 4 }, { 39, 45 } };
    for (const auto& c : probe) std::printf("at %u %u %d %d\n", c[0], c[1], frontier.rootAt(c[0], c[1]), frontier.regionAt(c[0], c[1]));
    const FrontierRegions::Goals goals = frontier.goals(min_size, w_size, w_cost);
    for (unsigned q = 0; q < P; ++q) std::printf("goal %u %d %d %.17g\n", q, goals.cell[q], goals.region[q], goals.score[q]);
    // the goal cells go into the partition's own path call as they are
    std::vector<double> pose(3 * P);
    for (unsigned q = 0; q < P; ++q)
      for (unsigned k = 0; k < 3; ++k) pose[3 * q + k] = robots(k, q);
    double *d_pose = nullptr, *d_path = nullptr;
    int* d_len = nullptr;
    hip_check(hipMalloc(reinterpret_cast<void**>(&d_pose), sizeof(double) * 3 * P));
    hip_check(hipMalloc(reinterpret_cast<void**>(&d_path), sizeof(double) * 3 * P * n_steps));
    hip_check(hipMalloc(reinterpret_cast<void**>(&d_len), sizeof(int) * P));
    hip_check(hipMemcpy(d_pose, pose.data(), sizeof(double) * 3 * P, hipMemcpyHostToDevice));
    const Collision collision(0.3, 1.2, 0.1, 0.8);
    const eea_collision_cfg cfg = collision.deviceConfig(g);
    throw_on_error(eea_partition_path_batch(device_ordinal(), &cfg, part.costs(), part.owners(), d_pose, P, frontier.goalCells(), n_steps,
                                            d_path, d_len, nullptr));
    int len[P];
    hip_check(hipMemcpy(len, d_len, sizeof(len), hipMemcpyDeviceToHost));
    for (unsigned q = 0; q < P; ++q) std::printf("len %u %d\n", q, len[q]);
    (void)hipFree(d_pose);
    (void)hipFree(d_path);
    (void)hipFree(d_len);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "frontier_regions_tests: %s\n", e.what());
    return 1;
  }
}
