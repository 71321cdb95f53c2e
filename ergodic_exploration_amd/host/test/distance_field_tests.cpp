// DistanceField of the host mirror (distance_field.hpp) on a fixed grid, fixed poses and fixed trajectories: prints the
// answers, tests/test_gpu_distance_field.py compares them with the numpy restatement.  Needs a GPU.
//   grid W H resolution origin_x origin_y         the map (cells: see fill below)
//   field i sq... / near i n...                   the two planes, one line per row
//   batch q x y msg sqrd_obs dx dy dmin disp_x disp_y      one line per pose
//   worst b T msg sqrd_obs dx dy step dmin        one line per trajectory; its steps are the poses b, b + 1, ..., b + T - 1
#include <cstdio>
#include <exception>
#include <vector>

#include <ergodic_exploration/distance_field.hpp>

using namespace ergodic_exploration;

int main()
{
  try {
    const unsigned W = 50, H = 40;
    const double res = 0.1, ox = -1.0, oy = -2.0;
    GridData d(W * H, 0);
    for (unsigned i = 10; i < 14; ++i)
      for (unsigned j = 20; j < 26; ++j) d[i * W + j] = 100;  // a block
    d[30 * W + 5] = 80;                                        // exactly at the threshold: occupied
    d[31 * W + 7] = 79;                                        // just below: free
    d[25 * W + 40] = 100;
    d[3 * W + 44] = 100;
    d[38 * W + 30] = 100;
    for (unsigned i = 5; i < 8; ++i) d[i * W + 2] = -1;        // unknown: free
    const GridMap g = GridMap::fromOccupancyGrid(W, H, res, ox, oy, d);
    DistanceField field(0.3, 1.2, 0.1, 0.8);
    // a larger and a smaller map first: the planes are reallocated, then reused
    const GridMap big = GridMap::fromOccupancyGrid(70, 60, res, ox, oy, GridData(70 * 60, 100));
    const GridMap small = GridMap::fromOccupancyGrid(9, 7, res, ox, oy, GridData(9 * 7, 0));
    field.update(big);
    field.update(small);
    field.update(g);
    std::printf("grid %u %u %.17g %.17g %.17g\n", W, H, res, ox, oy);

    std::vector<int> sq(W * H), near(W * H);
    hip_check(hipMemcpy(sq.data(), field.squaredDistances(), sizeof(int) * W * H, hipMemcpyDeviceToHost));
    hip_check(hipMemcpy(near.data(), field.nearestCells(), sizeof(int) * W * H, hipMemcpyDeviceToHost));
    for (unsigned i = 0; i < H; ++i) {
      std::printf("field %u", i);
      for (unsigned j = 0; j < W; ++j) std::printf(" %d", sq[i * W + j]);
      std::printf("\nnear %u", i);
      for (unsigned j = 0; j < W; ++j) std::printf(" %d", near[i * W + j]);
      std::printf("\n");
    }

    const unsigned NX = 14, NY = 11, P = NX * NY;
    mat poses(3, P);
    for (unsigned a = 0; a < NY; ++a) {
      for (unsigned b = 0; b < NX; ++b) {
        poses(0, a * NX + b) = -1.55 + 0.45 * b;  // from outside the map to outside it
        poses(1, a * NX + b) = -2.55 + 0.45 * a;
        poses(2, a * NX + b) = 0.1 * a;
      }
    }
    const DistanceField::Answer c = field.query(poses);
    for (unsigned q = 0; q < P; ++q) {
      std::printf("batch %u %.17g %.17g %d %d %d %d %.17g %.17g %.17g\n", q, poses(0, q), poses(1, q), static_cast<int>(c.msg[q]),
                  c.cells[q].sqrd_obs, c.cells[q].dx, c.cells[q].dy, c.dmin[q], c.disp(0, q), c.disp(1, q));
    }
    // trajectories: runs of consecutive poses (a run inside one row of the pose lattice stays on the map, one across rows leaves it)
    const unsigned starts[] = { 30, 30, 58, 44, 100, 89 }, lengths[] = { 1, 11, 11, 70, 5, 6 };
    for (unsigned n = 0; n < 6; ++n) {
      mat traj(3, lengths[n]);
      for (unsigned t = 0; t < lengths[n]; ++t) traj.set_col(t, poses.col(starts[n] + t));
      const DistanceField::WorstStep w = field.worstStep(traj);
      std::printf("worst %u %u %d %d %d %d %d %.17g\n", starts[n], lengths[n], static_cast<int>(w.msg), w.cell.sqrd_obs, w.cell.dx,
                  w.cell.dy, w.step, w.dmin);
    }
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "distance_field_tests: %s\n", e.what());
    return 1;
  }
}
