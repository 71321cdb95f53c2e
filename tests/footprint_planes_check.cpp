// csrc/footprint_planes.hpp alone, without a GPU: the validation of a footprint, its half-planes and radii, and the integer
// thresholds of the filter.  tests/test_footprint.py builds this with the address and undefined-behaviour sanitizers and
// runs it as a process of its own; it stops at the first wrong answer and names the line.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>

#include "../ergodic_exploration_amd/csrc/footprint_planes.hpp"

using namespace eea;

#define EXPECT(cond)                                                         \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::printf("footprint planes: line %d: %s\n", __LINE__, #cond);       \
      std::exit(1);                                                          \
    }                                                                        \
  } while (0)

static FootprintFault fault_of(unsigned n, const double* x, const double* y)
{
  FootprintPlanes p;
  return footprint_planes(n, x, y, p);
}

int main()
{
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  FootprintPlanes p;
  {  // the 0.9 m x 0.5 m rectangle: normals +x +y -x -y, offsets the half sides
    const double x[] = { 0.45, 0.45, -0.45, -0.45 }, y[] = { -0.25, 0.25, 0.25, -0.25 };
    EXPECT(footprint_planes(4, x, y, p) == FootprintFault::none);
    EXPECT(p.n == 4);
    EXPECT(p.nx[0] == 1.0 && p.ny[0] == 0.0 && p.h[0] == 0.45);
    EXPECT(p.nx[1] == 0.0 && p.ny[1] == 1.0 && p.h[1] == 0.25);
    EXPECT(p.nx[2] == -1.0 && p.ny[2] == 0.0 && p.h[2] == 0.45);
    EXPECT(p.nx[3] == 0.0 && p.ny[3] == -1.0 && p.h[3] == 0.25);
    EXPECT(p.r_in == 0.25);
    EXPECT(p.r_out == std::sqrt(0.45 * 0.45 + 0.25 * 0.25));
    EXPECT(footprint_supported(p, 0.1) && footprint_supported(p, p.r_out / 1024.0) && !footprint_supported(p, 0.0005));
    // the same polygon clockwise
    const double cx[] = { -0.45, -0.45, 0.45, 0.45 }, cy[] = { -0.25, 0.25, 0.25, -0.25 };
    EXPECT(fault_of(4, cx, cy) == FootprintFault::not_convex);
    // the body origin on an edge, and outside
    const double ex[] = { 0.9, 0.9, 0.0, 0.0 };
    EXPECT(fault_of(4, ex, y) == FootprintFault::origin_outside);
    const double ox[] = { 0.9, 0.9, 0.1, 0.1 };
    EXPECT(fault_of(4, ox, y) == FootprintFault::origin_outside);
  }
  {  // the body origin 0.1 m from the rear edge
    const double x[] = { 0.9, 0.9, -0.1, -0.1 }, y[] = { -0.2, 0.2, 0.2, -0.2 };
    EXPECT(footprint_planes(4, x, y, p) == FootprintFault::none);
    EXPECT(p.r_in == 0.1 && p.r_out == std::sqrt(0.9 * 0.9 + 0.2 * 0.2));
  }
  {  // the number of vertices: the arrays are not read when it is out of range
    const double x[] = { 1.0, -1.0 }, y[] = { 0.0, 0.0 };
    EXPECT(fault_of(2, x, y) == FootprintFault::vertex_count);
    EXPECT(fault_of(0, nullptr, nullptr) == FootprintFault::vertex_count);
    EXPECT(fault_of(17, x, y) == FootprintFault::vertex_count);
    EXPECT(fault_of(0xffffffffu, x, y) == FootprintFault::vertex_count);
  }
  {  // 16 vertices on a circle pass, every h the same apothem within rounding
    double x[16], y[16];
    for (int k = 0; k < 16; ++k) {
      x[k] = 0.5 * std::cos(k * 0.39269908169872414);
      y[k] = 0.5 * std::sin(k * 0.39269908169872414);
    }
    EXPECT(footprint_planes(16, x, y, p) == FootprintFault::none);
    for (int k = 0; k < 16; ++k) EXPECT(std::fabs(p.h[k] - 0.5 * std::cos(0.19634954084936207)) < 1e-15);
    EXPECT(std::fabs(p.r_out - 0.5) < 1e-15 && p.r_in <= p.r_out);
  }
  {  // not finite, collinear, repeated, a reflex turn
    const double y[] = { 0.0, 0.35, -0.35 };
    const double a[] = { 0.6, nan, -0.3 }, b[] = { 0.6, -0.3, inf };
    EXPECT(fault_of(3, a, y) == FootprintFault::not_finite && fault_of(3, b, y) == FootprintFault::not_finite);
    const double lx[] = { 0.45, 0.45, 0.45, -0.45, -0.45 }, ly[] = { -0.25, 0.0, 0.25, 0.25, -0.25 };
    EXPECT(fault_of(5, lx, ly) == FootprintFault::not_convex);
    const double rx[] = { 0.45, 0.45, 0.45, -0.45, -0.45 }, ry[] = { -0.25, 0.25, 0.25, 0.25, -0.25 };
    EXPECT(fault_of(5, rx, ry) == FootprintFault::not_convex);
    const double fx[] = { 0.45, 0.1, 0.45, -0.45, -0.45 }, fy[] = { -0.25, 0.0, 0.25, 0.25, -0.25 };
    EXPECT(fault_of(5, fx, fy) == FootprintFault::not_convex);
    const double hx[] = { 1e200, -1e200, -1e200 }, hy[] = { 0.0, 1e200, -1e200 };  // the cross product overflows
    EXPECT(fault_of(3, hx, hy) != FootprintFault::none);
  }
  {  // thresholds: a = r_in / res - 0.7072 - 1e-6; floor(a)^2 or -1; ceil(r_out / res + 0.7072 + 1e-6)^2; ceil(r_out / res) + 1
    FootprintThresholds t = footprint_thresholds(0.25, 0.51478150704935, 0.05);
    EXPECT(t.sq_hit == 16 && t.sq_free == 144 && t.box == 12);
    t = footprint_thresholds(0.25, 0.51478150704935, 0.25);
    EXPECT(t.sq_hit == 0 && t.sq_free == 9 && t.box == 4);
    t = footprint_thresholds(0.1, 0.9219544457292888, 0.1);
    EXPECT(t.sq_hit == 0 && t.sq_free == 100 && t.box == 11);
    t = footprint_thresholds(0.0707, 0.2, 0.1);  // a just below 0: no pose is a sure hit
    EXPECT(t.sq_hit == -1);
    t = footprint_thresholds(0.07073, 0.2, 0.1);  // a just above 0: only an occupied own cell is
    EXPECT(t.sq_hit == 0);
    t = footprint_thresholds(1024.0, 1024.0, 1.0);  // the largest supported footprint
    EXPECT(t.sq_hit == 1023 * 1023 && t.sq_free == 1025 * 1025 && t.box == 1025);
    EXPECT(2 * t.box + 1 == 2051 && 2051ll * 2051ll < (1ll << 31));  // the largest box's cells fit an int
  }
  std::printf("footprint planes: ok\n");
  return 0;
}
