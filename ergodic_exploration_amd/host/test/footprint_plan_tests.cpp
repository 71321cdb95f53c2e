// Footprint::validateControl and DynamicWindow::control for a polygon base (footprint.hpp, dynamic_window.hpp) on the grid of
// footprint_tests, fixed robots, each with and without a DistanceField: prints the answers, tests/test_gpu_footprint_plan.py
// compares them with tests/footprint_plan_restatement.py.  Needs a GPU.
//   grid W H resolution origin_x origin_y       the map (cells: see fill below)
//   robot q x y th vb0 vb1 vb2 r0 r1 r2          robot q: pose, odometry, and r -- the twist validateControl rolls out, the
//                                                reference twist of the twist-error mode, and the step of the reference
//                                                trajectory: column t is x0 + (t + 1) * (0.1 * r), 25 columns every 0.1 s
//   validate f q valid valid_through_the_field   footprint f (0: the 0.9 m x 0.5 m rectangle, 1: the origin 0.1 m from the rear)
//   vref f q found u0 u1 u2 found u0 u1 u2       the twist-error mode, plain and through the field
//   traj f q found u0 u1 u2 found u0 u1 u2       the trajectory mode
#include <cstdio>
#include <exception>
#include <tuple>
#include <utility>
#include <vector>

#include <ergodic_exploration/dynamic_window.hpp>
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
    // the omni window of the tests: 3 x 8 x 5 samples, 10 steps of 0.1 s
    const DynamicWindow dwa(Collision(0.7, 1.0, 0.2, 0.8), 0.1, 1.0, 0.2, 1.0, 1.0, 1.0, 1.0, -1.0, 1.0, -1.0, 2.0, -2.0, 3, 8, 5);
    const unsigned NX = 8, NY = 6, P = NX * NY, n_ref = 25;
    const double dt_ref = 0.1;
    std::vector<vec> x0(P, vec(3)), vb(P, vec(3)), r(P, vec(3));
    for (unsigned q = 0; q < P; ++q) {
      x0[q](0) = -0.8 + 0.62 * (q % NX);  // over the map, the block and the single cells
      x0[q](1) = -1.7 + 0.7 * (q / NX);
      x0[q](2) = 0.37 * q - 3.0;
      vb[q](0) = -0.9 + 0.04 * q;
      vb[q](1) = 0.8 - 0.035 * q;
      vb[q](2) = -1.5 + 0.07 * q;
      r[q](0) = 0.9 - 0.045 * q;
      r[q](1) = -0.7 + 0.03 * q;
      r[q](2) = 1.2 - 0.05 * q;
      std::printf("robot %u %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", q, x0[q](0), x0[q](1), x0[q](2), vb[q](0),
                  vb[q](1), vb[q](2), r[q](0), r[q](1), r[q](2));
    }
    for (unsigned f = 0; f < 2; ++f) {
      const Footprint base(shapes[f], 0.8);
      for (unsigned q = 0; q < P; ++q) {
        std::printf("validate %u %u %d %d\n", f, q, static_cast<int>(base.validateControl(g, x0[q], r[q], 0.1, 1.0)),
                    static_cast<int>(base.validateControl(g, x0[q], r[q], 0.1, 1.0, &field)));
        mat xt(3, n_ref);
        for (unsigned t = 0; t < n_ref; ++t) {
          for (unsigned c = 0; c < 3; ++c) xt(c, t) = x0[q](c) + static_cast<double>(t + 1) * (0.1 * r[q](c));
        }
        for (int mode = 0; mode < 2; ++mode) {
          bool ok[2];
          vec u[2];
          for (int through = 0; through < 2; ++through) {
            const DistanceField* const fld = through ? &field : nullptr;
            std::tie(ok[through], u[through]) =
                mode == 0 ? dwa.control(g, x0[q], vb[q], r[q], base, fld) : dwa.control(g, x0[q], vb[q], xt, dt_ref, base, fld);
          }
          std::printf("%s %u %u %d %.17g %.17g %.17g %d %.17g %.17g %.17g\n", mode == 0 ? "vref" : "traj", f, q, static_cast<int>(ok[0]),
                      u[0](0), u[0](1), u[0](2), static_cast<int>(ok[1]), u[1](0), u[1](1), u[1](2));
        }
      }
    }
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "footprint_plan_tests: %s\n", e.what());
    return 1;
  }
}
