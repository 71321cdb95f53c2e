// GeodesicPartition of the host mirror (geodesic_partition.hpp) on a small map with fixed robots and a fixed gain field: prints
// the answers, tests/test_gpu_partition.py compares them with the restatement.  Needs a GPU.
//   map W H resolution origin_x origin_y flags sources stride n_steps   the map (cells: see below), what the calls were given
//   weights w_field w_cost
//   robot q x y th                                                     one line per robot
//   geo i c... / owner i c...                                          the two planes, one line per row
//   goal q area cell score                                             one line per robot
//   len q n / way q t x y th                                           its path: moves written, n_steps way-points
#include <cstdio>
#include <exception>
#include <vector>

#include <ergodic_exploration/geodesic_partition.hpp>

using namespace ergodic_exploration;

int main()
{
  try {
    const double res = 0.1, ox = -1.0, oy = -2.0, w_field = 1.0, w_cost = 0.125;
    const unsigned W = 50, H = 40, stride = 2, n_steps = 12, P = 5;
    // 50 x 40 (more than one tile): a wall with a door, a sealed room, unknown cells that block
    GridData d(W * H, 0);
    for (unsigned i = 0; i < 30; ++i) d[i * W + 20] = 100;
    d[12 * W + 20] = 0;
    for (unsigned j = 34; j < 44; ++j) d[25 * W + j] = d[34 * W + j] = 100;
    for (unsigned i = 25; i < 35; ++i) d[i * W + 34] = d[i * W + 43] = 100;
    for (unsigned i = 3; i < 9; ++i)
      for (unsigned j = 30; j < 36; ++j) d[i * W + j] = -1;
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
    std::printf("map %u %u %.17g %.17g %.17g %u %u %u %u\n", W, H, res, ox, oy, EEA_GEODESIC_UNKNOWN_BLOCKS, part.sources(), stride, n_steps);
    std::printf("weights %.17g %.17g\n", w_field, w_cost);
    for (unsigned q = 0; q < P; ++q) std::printf("robot %u %.17g %.17g %.17g\n", q, robots(0, q), robots(1, q), robots(2, q));
    std::vector<int> plane(W * H);
    const char* const names[2] = { "geo", "owner" };
    for (int k = 0; k < 2; ++k) {
      hip_check(hipMemcpy(plane.data(), k == 0 ? part.costs() : part.owners(), sizeof(int) * W * H, hipMemcpyDeviceToHost));
      for (unsigned i = 0; i < H; ++i) {
        std::printf("%s %u", names[k], i);
        for (unsigned j = 0; j < W; ++j) std::printf(" %d", plane[i * W + j]);
        std::printf("\n");
      }
    }
    // a gain field full of repeated values
    std::vector<unsigned> field(W * H);
    for (unsigned c = 0; c < W * H; ++c) field[c] = (c * 7u + 3u) % 5u;
    unsigned* d_field = nullptr;
    hip_check(hipMalloc(reinterpret_cast<void**>(&d_field), sizeof(unsigned) * W * H));
    hip_check(hipMemcpy(d_field, field.data(), sizeof(unsigned) * W * H, hipMemcpyHostToDevice));
    const std::vector<unsigned> area = part.area();
    const GeodesicPartition::Goals goals = part.goals(0, d_field, stride, w_field, w_cost);
    for (unsigned q = 0; q < P; ++q) {
      if (area[q] != goals.area[q]) throw std::runtime_error("area() and goals() disagree");
      std::printf("goal %u %u %d %.17g\n", q, goals.area[q], goals.cell[q], goals.score[q]);
    }
    const GeodesicPartition::Walk w = part.paths(n_steps);
    for (unsigned q = 0; q < P; ++q) {
      std::printf("len %u %d\n", q, w.len[q]);
      for (unsigned t = 0; t < n_steps; ++t) {
        std::printf("way %u %u %.17g %.17g %.17g\n", q, t, w.path(0, q * n_steps + t), w.path(1, q * n_steps + t), w.path(2, q * n_steps + t));
      }
    }
    (void)hipFree(d_field);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "geodesic_partition_tests: %s\n", e.what());
    return 1;
  }
}
