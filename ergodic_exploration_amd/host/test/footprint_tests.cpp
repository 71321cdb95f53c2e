// Footprint of the host mirror (footprint.hpp) on a fixed grid, fixed poses and fixed trajectories, each with and without a
// DistanceField: prints the answers, tests/test_gpu_footprint.py compares them with the numpy restatement.  Needs a GPU.
//   grid W H resolution origin_x origin_y         the map (cells: see fill below)
//   radii f r_in r_out                            footprint f (0: the 0.9 m x 0.5 m rectangle, 1: the origin 0.1 m from the rear)
//   check f q x y th hit hit_through_the_field    one line per footprint and pose
//   first f b T step step_through_the_field       one line per footprint and trajectory; its steps are the poses b .. b + T - 1
//   refused n                                     the number of malformed footprints the constructor threw on
#include <cmath>
#include <cstdio>
#include <exception>
#include <stdexcept>
#include <utility>
#include <vector>

#include <ergodic_exploration/footprint.hpp>

using namespace ergodic_exploration;
using Vertices = std::vector<std::pair<double, double>>;

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
    field.update(g);
    std::printf("grid %u %u %.17g %.17g %.17g\n", W, H, res, ox, oy);

    const Vertices shapes[2] = { { { 0.45, -0.25 }, { 0.45, 0.25 }, { -0.45, 0.25 }, { -0.45, -0.25 } },
                                 { { 0.9, -0.2 }, { 0.9, 0.2 }, { -0.1, 0.2 }, { -0.1, -0.2 } } };
    const unsigned NX = 14, NY = 11, P = NX * NY;
    mat poses(3, P);
    for (unsigned a = 0; a < NY; ++a) {
      for (unsigned b = 0; b < NX; ++b) {
        poses(0, a * NX + b) = -1.55 + 0.45 * b;  // from outside the map to outside it
        poses(1, a * NX + b) = -2.55 + 0.45 * a;
        poses(2, a * NX + b) = 0.37 * (a * NX + b) - 3.0;
      }
    }
    const unsigned starts[] = { 30, 30, 58, 44, 100, 89, 0 }, lengths[] = { 1, 11, 11, 70, 5, 6, 154 };
    for (unsigned f = 0; f < 2; ++f) {
      const Footprint base(shapes[f], 0.8);
      std::printf("radii %u %.17g %.17g\n", f, base.inscribedRadius(), base.circumscribedRadius());
      const std::vector<bool> plain = base.check(g, poses), through = base.check(g, poses, &field);
      for (unsigned q = 0; q < P; ++q) {
        std::printf("check %u %u %.17g %.17g %.17g %d %d\n", f, q, poses(0, q), poses(1, q), poses(2, q), static_cast<int>(plain[q]),
                    static_cast<int>(through[q]));
      }
      // the single-pose form is the batch's
      const bool one = base.check(g, poses.col(47)), one_through = base.check(g, poses.col(47), &field);
      if (one != plain[47] || one_through != through[47]) throw std::logic_error("the single-pose form differs from the batch");
      for (unsigned n = 0; n < 7; ++n) {
        mat traj(3, lengths[n]);
        for (unsigned t = 0; t < lengths[n]; ++t) traj.set_col(t, poses.col(starts[n] + t));
        std::printf("first %u %u %u %d %d\n", f, starts[n], lengths[n], base.firstStep(g, traj), base.firstStep(g, traj, &field));
      }
    }

    // malformed footprints: clockwise, a collinear vertex, the origin on an edge, two vertices, seventeen
    Vertices many;
    for (int k = 0; k < 17; ++k) many.push_back({ 0.5 * std::cos(k * 6.283185307179586 / 17), 0.5 * std::sin(k * 6.283185307179586 / 17) });
    const Vertices bad[] = { { { -0.45, -0.25 }, { -0.45, 0.25 }, { 0.45, 0.25 }, { 0.45, -0.25 } },
                             { { 0.45, -0.25 }, { 0.45, 0.0 }, { 0.45, 0.25 }, { -0.45, 0.25 }, { -0.45, -0.25 } },
                             { { 0.9, -0.2 }, { 0.9, 0.2 }, { 0.0, 0.2 }, { 0.0, -0.2 } },
                             { { 0.5, 0.0 }, { -0.5, 0.0 } },
                             many };
    unsigned refused = 0;
    for (const Vertices& v : bad) {
      try {
        const Footprint base(v);
        (void)base;
      } catch (const std::invalid_argument&) {
        ++refused;
      }
    }
    std::printf("refused %u\n", refused);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "footprint_tests: %s\n", e.what());
    return 1;
  }
}
