// One cell test for every footprint kernel (footprint_kernel.hip, footprint_plan_kernel.hip): classify -- what one int of the
// distance field decides about a pose -- and resolve, the exact test of one pose's box by a whole wavefront.  The files that
// include this are compiled without FMA contraction; footprint_kernel.hip's header describes both.
//
// Every function that judges a pose takes a last argument: NoBodies (nothing changes, the code is the code it was) or Bodies,
// the body layer (body_layer_kernel.hip) as one lane sees it -- reached through `if constexpr` only, the way FleetView joined the
// disc's kernels.  With Bodies a cell is occupied when the grid says so OR a stamped robot other than the lane's own covers it.
#pragma once

#include <cmath>
#include <cstdint>
#include <type_traits>

#include "common.hpp"
#include "footprint_planes.hpp"
#include "grid_cell.hpp"

namespace eea
{
namespace
{
constexpr int kCellsPerLane = 4;  // of a chunk of the box: 256 cells

enum : int { kFree = 0, kHit = 1, kAmbiguous = 2 };

struct Box
{
  int x0, x1, y0, y1;  // inclusive, inside the grid
};

// the empty view: no layer
struct NoBodies
{
};
// the layer and the snapshot of the robot whose pose the lane judges (stamped false: nobody's body is taken out)
struct Bodies
{
  BodyView v;
  double px, py, sn, cs;
  bool stamped;
};
template <class BV>
constexpr bool kWithBodies = std::is_same_v<BV, Bodies>;
// what resolve keeps beside a cell with the layer (nothing without): the robot of the pose, and the count of a cell
template <class BV>
struct SelfOf
{
};
template <>
struct SelfOf<Bodies>
{
  double px, py, sn, cs;
  bool stamped;
};
template <class BV>
struct CountOf
{
};
template <>
struct CountOf<Bodies>
{
  int n;
};

__device__ __forceinline__ int classify(const CollisionParams& c, const FootprintArgs& f, const int* __restrict__ d_sq, double px,
                                        double py, double th, Box& b)
{
  b = Box{ 0, -1, 0, -1 };
  if (!(isfinite(px) && isfinite(py) && isfinite(th))) return kFree;
  const double fx = floor((px - c.xmin) / c.resolution), fy = floor((py - c.ymin) / c.resolution);
  const double xlast = static_cast<double>(c.xsize - 1u), ylast = static_cast<double>(c.ysize - 1u), rb = static_cast<double>(f.box);
  // (a NaN from a non-finite xmin / ymin fails the comparison: free)
  if (!(fx + rb >= 0.0 && fx - rb <= xlast && fy + rb >= 0.0 && fy - rb <= ylast)) return kFree;
  b.x0 = static_cast<int>(fmax(fx - rb, 0.0));
  b.x1 = static_cast<int>(fmin(fx + rb, xlast));
  b.y0 = static_cast<int>(fmax(fy - rb, 0.0));
  b.y1 = static_cast<int>(fmin(fy + rb, ylast));
  if (d_sq != nullptr && fx >= 0.0 && fx <= xlast && fy >= 0.0 && fy <= ylast) {
    const int sq = d_sq[static_cast<size_t>(fy) * c.xsize + static_cast<size_t>(fx)];
    if (sq < 0 || sq > f.sq_free) return kFree;
    if (sq <= f.sq_hit) return kHit;
  }
  return kAmbiguous;
}

// lane k < n of every wavefront holds half-plane k in registers: the test reads them with v_readlane (no memory, no wait)
struct PlaneRegs
{
  double nx, ny, h;
};
__device__ __forceinline__ PlaneRegs load_planes(const FootprintArgs& f, int lane)
{
  const int k = lane % static_cast<int>(kFootprintMaxVertices);
  return PlaneRegs{ f.nx[k], f.ny[k], f.h[k] };
}

// lane src's value in every lane, src wavefront-uniform
__device__ __forceinline__ int lane_value(int v, int src) { return __builtin_amdgcn_readlane(v, src); }
__device__ __forceinline__ double lane_value(double v, int src)
{
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), src), __builtin_amdgcn_readlane(__double2loint(v), src));
}

// T(cell, pose): the closed test of the centre of cell (row i, column j) against the polygon placed at (px, py) with the sine
// and cosine given -- resolve's products and sums in resolve's order.  The stamp of the body layer and every lookup that takes
// a robot's own body out of the count call this one function with the same values: the same bits
__device__ __forceinline__ bool cell_inside(const CollisionParams& c, const FootprintArgs& f, const PlaneRegs& pl, int i, int j,
                                            double px, double py, double sn, double cs)
{
  const double cxw = static_cast<double>(j) * c.resolution + c.resolution / 2.0 + c.xmin;
  const double cyw = static_cast<double>(i) * c.resolution + c.resolution / 2.0 + c.ymin;
  const double dx = cxw - px, dy = cyw - py;
  const double bx = cs * dx + sn * dy, by = (-sn) * dx + cs * dy;
  bool in = true;
  for (int kk = 0; kk < static_cast<int>(f.n); ++kk) {
    const int ku = __builtin_amdgcn_readfirstlane(kk);
    in = in & (lane_value(pl.nx, ku) * bx + lane_value(pl.ny, ku) * by <= lane_value(pl.h, ku));
  }
  return in;
}

// the robot whose pose query q is: self[q], or q itself (the tick), or nobody (-1); an index outside [-1, B) is the caller's error
__device__ __forceinline__ Bodies load_bodies(const BodyArgs& a, size_t q)
{
  Bodies bv{ a.v, 0.0, 0.0, 0.0, 0.0, false };
  const int i = a.self != nullptr ? a.self[q] : (a.self_is_index != 0 ? static_cast<int>(q) : -1);
  if (i >= 0) {
    const double* const s = a.v.snap + static_cast<size_t>(kBodySnap) * static_cast<size_t>(i);
    bv.px = s[0];
    bv.py = s[1];
    bv.sn = s[2];
    bv.cs = s[3];
    bv.stamped = s[4] != 0.0;
  }
  return bv;
}

// does a stamped robot other than the lane's own cover the in-grid cell (row i, column j)?  n = cover there
__device__ __forceinline__ bool other_body(const CollisionParams& c, const FootprintArgs& f, const PlaneRegs& pl, int n, int i, int j,
                                           bool stamped, double spx, double spy, double ssn, double scs)
{
  if (n > 0 && stamped && cell_inside(c, f, pl, i, j, spx, spy, ssn, scs)) n -= 1;
  return n > 0;
}

// The filter of the layer: true when `near` proves that no other robot's body shares a cell with a polygon placed at (px, py).
// Only for a pose whose box touches the grid (classify's first test): its cell then lies inside the near map
__device__ __forceinline__ bool nobody_near(const CollisionParams& c, const Bodies& bv, double px, double py)
{
  if ((bv.v.flags & kBodyLayerNoFilter) != 0u) return false;
  const double fx = floor((px - c.xmin) / c.resolution), fy = floor((py - c.ymin) / c.resolution);
  const double rb = static_cast<double>(bv.v.box), rn = static_cast<double>(bv.v.Rn);
  int n = bv.v.near[static_cast<size_t>(static_cast<int>(fy + rb)) * static_cast<size_t>(bv.v.near_w) +
                    static_cast<size_t>(static_cast<int>(fx + rb))];
  if (bv.stamped) {
    const double sx = floor((bv.px - c.xmin) / c.resolution), sy = floor((bv.py - c.ymin) / c.resolution);
    if (fabs(fx - sx) <= rn && fabs(fy - sy) <= rn) n -= 1;
  }
  return n == 0;
}

// classify with the layer: a sure hit stands; free by the field only where the layer's filter agrees
template <class BV>
__device__ __forceinline__ int classify_with(const CollisionParams& c, const FootprintArgs& f, const int* __restrict__ d_sq, double px,
                                             double py, double th, Box& b, BV bv)
{
  int cls = classify(c, f, d_sq, px, py, th, b);
  if constexpr (kWithBodies<BV>) {
    if (cls == kFree && b.x1 >= b.x0 && !nobody_near(c, bv, px, py)) cls = kAmbiguous;
  }
  return cls;
}

// The exact test of lane `src`'s pose over its box, by the whole wavefront; the result is wavefront-uniform.  (sn, cs) =
// sincos of the lane's own heading, formed by every ambiguous lane before the first of them is resolved.  The centre of cell
// (i, j) in the body frame: dx = cxw - px, dy = cyw - py, bx = cs * dx + sn * dy, by = (-sn) * dx + cs * dy.
template <class BV = NoBodies>
__device__ __forceinline__ bool resolve(const CollisionParams& c, const FootprintArgs& f, const PlaneRegs& pl,
                                        const int8_t* __restrict__ grid, int src, double px, double py, double sn, double cs,
                                        const Box& b, int lane, BV bv = BV{})
{
  const double qx = lane_value(px, src), qy = lane_value(py, src), qs = lane_value(sn, src), qc = lane_value(cs, src);
  const int x0 = lane_value(b.x0, src), x1 = lane_value(b.x1, src), y0 = lane_value(b.y0, src), y1 = lane_value(b.y1, src);
  const int w = x1 - x0 + 1, n = w * (y1 - y0 + 1);  // <= 2051^2
  // lane's cell idx = row * w + col of the box, advanced by 64 cells at a time without a division per step
  const int row_step = kWave / w, col_step = kWave - row_step * w;
  int row = lane / w, col = lane - row * w;
  const unsigned first_cell = static_cast<unsigned>(y0) * c.xsize + static_cast<unsigned>(x0);
  // (with the layer: the robot of lane src's pose, and grid may be null -- robots only)
  [[maybe_unused]] SelfOf<BV> self;
  if constexpr (kWithBodies<BV>) {
    self.px = lane_value(bv.px, src);
    self.py = lane_value(bv.py, src);
    self.sn = lane_value(bv.sn, src);
    self.cs = lane_value(bv.cs, src);
    self.stamped = lane_value(static_cast<int>(bv.stamped), src) != 0;
  }
  for (int base = 0; base < n; base += kWave * kCellsPerLane) {
    int8_t v[kCellsPerLane];
    int ci[kCellsPerLane], cj[kCellsPerLane];
    bool in[kCellsPerLane];
    [[maybe_unused]] CountOf<BV> nb[kCellsPerLane];
#pragma unroll
    for (int u = 0; u < kCellsPerLane; ++u) {
      ci[u] = y0 + row;
      cj[u] = x0 + col;
      // (a lane past the box reads the box's first cell and drops it: a select, not a branch around the load; the index fits
      // 32 bits, xsize * ysize <= 2^31)
      in[u] = base + u * kWave + lane < n;
      const unsigned at = in[u] ? static_cast<unsigned>(ci[u]) * c.xsize + static_cast<unsigned>(cj[u]) : first_cell;
      if constexpr (kWithBodies<BV>) {
        v[u] = grid != nullptr ? grid[at] : static_cast<int8_t>(0);
        nb[u].n = bv.v.cover[at];
      } else {
        v[u] = grid[at];
      }
      row += row_step;
      col += col_step;
      if (col >= w) {
        col -= w;
        ++row;
      }
    }
    bool any = false;
#pragma unroll
    for (int u = 0; u < kCellsPerLane; ++u) {
      if constexpr (kWithBodies<BV>) {
        in[u] = in[u] && ((grid != nullptr && v[u] >= f.v_min) || other_body(c, f, pl, nb[u].n, ci[u], cj[u], self.stamped, self.px, self.py, self.sn, self.cs));
      } else {
        in[u] = in[u] && v[u] >= f.v_min;  // occupied() as blocking_cutoff(occupied_threshold) states it (common.hpp)
      }
      any = any || in[u];
    }
    if (!__any(any)) continue;  // no occupied cell among these 256
    double bx[kCellsPerLane], by[kCellsPerLane];
#pragma unroll
    for (int u = 0; u < kCellsPerLane; ++u) {
      const double cxw = static_cast<double>(cj[u]) * c.resolution + c.resolution / 2.0 + c.xmin;
      const double cyw = static_cast<double>(ci[u]) * c.resolution + c.resolution / 2.0 + c.ymin;
      const double dx = cxw - qx, dy = cyw - qy;
      bx[u] = qc * dx + qs * dy;
      by[u] = (-qs) * dx + qc * dy;
    }
    for (int k = 0; k < static_cast<int>(f.n); ++k) {
      const double nx = lane_value(pl.nx, k), ny = lane_value(pl.ny, k), h = lane_value(pl.h, k);
#pragma unroll
      for (int u = 0; u < kCellsPerLane; ++u) in[u] = in[u] & (nx * bx[u] + ny * by[u] <= h);
    }
    any = false;
#pragma unroll
    for (int u = 0; u < kCellsPerLane; ++u) any = any || in[u];
    if (__any(any)) return true;
  }
  return false;
}
}  // namespace
}  // namespace eea
