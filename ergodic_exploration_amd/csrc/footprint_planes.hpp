// A polygon base as half-planes, and the thresholds of its filter through the distance field (footprint_kernel.hip,
// include/ergodic_amd.h "footprint collision").  Plain C++: no HIP call, no global state, like hit_map_table.hpp;
// tests/footprint_planes_check.cpp drives this file alone, without a GPU.
//
// The vertices are in the body frame, counter-clockwise, strictly convex, the body origin strictly inside.  Every value is
// formed by single IEEE operations in the order written here -- no hypot, no fused multiply-add -- so that
// tests/footprint_restatement.py reproduces the bits.
#pragma once

#include <cmath>

namespace eea
{
constexpr unsigned kFootprintMaxVertices = 16;
// the largest circumscribed radius in cells: box <= 1025, boxes of at most 2051^2 cells, thresholds far inside int
constexpr double kFootprintMaxCells = 1024.0;

// edge k runs from vertex k to vertex k + 1 (mod n); a body point b is inside iff nx[k] * b.x + ny[k] * b.y <= h[k] for every k
struct FootprintPlanes
{
  unsigned n;
  double nx[kFootprintMaxVertices], ny[kFootprintMaxVertices], h[kFootprintMaxVertices];
  double r_in, r_out;  // inscribed / circumscribed circle about the body origin
};

enum class FootprintFault
{
  none,
  vertex_count,    // n < 3 or n > 16
  not_finite,      // a vertex is NaN or infinite
  not_convex,      // a turn is not strictly left: the cross product of consecutive edges is <= 0 (clockwise, collinear, repeated)
  origin_outside   // some h_k <= 0: the body origin is on an edge or outside
};

inline const char* footprint_fault_text(FootprintFault f)
{
  switch (f) {
    case FootprintFault::vertex_count: return "a footprint has 3 to 16 vertices";
    case FootprintFault::not_finite: return "a footprint vertex is not finite";
    case FootprintFault::not_convex: return "the footprint must be strictly convex and counter-clockwise";
    case FootprintFault::origin_outside: return "the body origin must lie strictly inside the footprint";
    default: return "";
  }
}

// `p` is complete only when the answer is none
inline FootprintFault footprint_planes(unsigned n, const double* x, const double* y, FootprintPlanes& p)
{
  p = FootprintPlanes{};
  if (n < 3 || n > kFootprintMaxVertices) return FootprintFault::vertex_count;
  for (unsigned k = 0; k < n; ++k) {
    if (!std::isfinite(x[k]) || !std::isfinite(y[k])) return FootprintFault::not_finite;
  }
  for (unsigned k = 0; k < n; ++k) {  // before any division: an edge of length 0 turns nowhere
    const unsigned k1 = (k + 1) % n, k2 = (k + 2) % n;
    const double ax = x[k1] - x[k], ay = y[k1] - y[k], bx = x[k2] - x[k1], by = y[k2] - y[k1];
    if (!(ax * by - ay * bx > 0.0)) return FootprintFault::not_convex;
  }
  p.n = n;
  for (unsigned k = 0; k < n; ++k) {
    const unsigned k1 = (k + 1) % n;
    const double ex = x[k1] - x[k], ey = y[k1] - y[k];
    const double len = std::sqrt(ex * ex + ey * ey);
    p.nx[k] = ey / len;
    p.ny[k] = -ex / len;
    p.h[k] = p.nx[k] * x[k] + p.ny[k] * y[k];
    if (!(p.h[k] > 0.0)) return FootprintFault::origin_outside;
    const double r = std::sqrt(x[k] * x[k] + y[k] * y[k]);
    if (k == 0 || p.h[k] < p.r_in) p.r_in = p.h[k];
    if (k == 0 || r > p.r_out) p.r_out = r;
  }
  return FootprintFault::none;
}

// r_out / resolution <= kFootprintMaxCells (the caller has checked resolution > 0)
inline bool footprint_supported(const FootprintPlanes& p, double resolution) { return p.r_out / resolution <= kFootprintMaxCells; }

// The filter.  sq = the field's squared cell distance at the pose's cell; every occupied centre o then has
// | |p - o| - resolution * sqrt(sq) | <= resolution * sqrt(2) / 2 (the pose is anywhere in its cell, the centre in the middle
// of its own).  0.7072 > sqrt(2) / 2, and 1e-6 of a cell is many orders above any rounding:
//   0 <= sq <= sq_hit          an occupied centre lies inside the inscribed circle: a hit
//   sq == -1 or sq > sq_free   every occupied centre lies outside the circumscribed circle: free
// and the cells within `box` of the pose's own are all the exact test of the others has to look at.
struct FootprintThresholds
{
  int sq_hit;   // -1: the inscribed circle is too small to decide any pose
  int sq_free;
  int box;
};

inline FootprintThresholds footprint_thresholds(double r_in, double r_out, double resolution)
{
  FootprintThresholds t{ -1, 0, 0 };
  const double a = r_in / resolution - 0.7072 - 1e-6;
  if (a >= 0.0) {
    const int f = static_cast<int>(std::floor(a));
    t.sq_hit = f * f;
  }
  const int c = static_cast<int>(std::ceil(r_out / resolution + 0.7072 + 1e-6));
  t.sq_free = c * c;
  t.box = static_cast<int>(std::ceil(r_out / resolution)) + 1;
  return t;
}
}  // namespace eea
