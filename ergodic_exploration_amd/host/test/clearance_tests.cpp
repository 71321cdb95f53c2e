// Collision::minDistance / minDirection of the host mirror (collision.hpp) on a fixed grid and fixed poses: prints the answers,
// tests/test_gpu_clearance.py compares them with the oracle's search.  Needs a GPU.
//   grid W H resolution origin_x origin_y         the map (cells: see fill below)
//   batch q x y msg sqrd_obs dx dy dmin disp_x disp_y      one line per pose, from the batched form
//   single q msg dmin msg disp_x disp_y           minDistance and minDirection of the first poses, one call each
#include <cstdio>
#include <exception>

#include <ergodic_exploration/collision.hpp>

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
    const Collision col(0.3, 1.2, 0.1, 0.8);
    std::printf("grid %u %u %.17g %.17g %.17g\n", W, H, res, ox, oy);

    const unsigned NX = 14, NY = 11, P = NX * NY;
    mat poses(3, P);
    for (unsigned a = 0; a < NY; ++a) {
      for (unsigned b = 0; b < NX; ++b) {
        poses(0, a * NX + b) = -1.55 + 0.45 * b;  // from outside the map to outside it
        poses(1, a * NX + b) = -2.55 + 0.45 * a;
        poses(2, a * NX + b) = 0.1 * a;
      }
    }
    const Collision::Clearance c = col.clearance(g, poses);
    for (unsigned q = 0; q < P; ++q) {
      std::printf("batch %u %.17g %.17g %d %d %d %d %.17g %.17g %.17g\n", q, poses(0, q), poses(1, q), static_cast<int>(c.msg[q]),
                  c.cells[q].sqrd_obs, c.cells[q].dx, c.cells[q].dy, c.dmin[q], c.disp(0, q), c.disp(1, q));
    }
    for (unsigned q = 0; q < P; q += 9) {
      const auto [m1, dmin] = col.minDistance(g, poses.col(q));
      const auto [m2, disp] = col.minDirection(g, poses.col(q));
      std::printf("single %u %d %.17g %d %.17g %.17g\n", q, static_cast<int>(m1), dmin, static_cast<int>(m2), disp(0), disp(1));
    }
    eea_release_collision_caches();
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "clearance_tests: %s\n", e.what());
    return 1;
  }
}
