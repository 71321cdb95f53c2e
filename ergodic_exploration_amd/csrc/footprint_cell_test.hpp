// One cell test for every footprint kernel (footprint_kernel.hip, footprint_plan_kernel.hip): classify -- what one int of the
// distance field decides about a pose -- and resolve, the exact test of one pose's box by a whole wavefront.  The files that
// include this are compiled without FMA contraction; footprint_kernel.hip's header describes both.
#pragma once

#include <cmath>
#include <cstdint>

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

// The exact test of lane `src`'s pose over its box, by the whole wavefront; the result is wavefront-uniform.  (sn, cs) =
// sincos of the lane's own heading, formed by every ambiguous lane before the first of them is resolved.  The centre of cell
// (i, j) in the body frame: dx = cxw - px, dy = cyw - py, bx = cs * dx + sn * dy, by = (-sn) * dx + cs * dy.
__device__ __forceinline__ bool resolve(const CollisionParams& c, const FootprintArgs& f, const PlaneRegs& pl,
                                        const int8_t* __restrict__ grid, int src, double px, double py, double sn, double cs,
                                        const Box& b, int lane)
{
  const double qx = lane_value(px, src), qy = lane_value(py, src), qs = lane_value(sn, src), qc = lane_value(cs, src);
  const int x0 = lane_value(b.x0, src), x1 = lane_value(b.x1, src), y0 = lane_value(b.y0, src), y1 = lane_value(b.y1, src);
  const int w = x1 - x0 + 1, n = w * (y1 - y0 + 1);  // <= 2051^2
  // lane's cell idx = row * w + col of the box, advanced by 64 cells at a time without a division per step
  const int row_step = kWave / w, col_step = kWave - row_step * w;
  int row = lane / w, col = lane - row * w;
  const unsigned first_cell = static_cast<unsigned>(y0) * c.xsize + static_cast<unsigned>(x0);
  for (int base = 0; base < n; base += kWave * kCellsPerLane) {
    int8_t v[kCellsPerLane];
    int ci[kCellsPerLane], cj[kCellsPerLane];
    bool in[kCellsPerLane];
#pragma unroll
    for (int u = 0; u < kCellsPerLane; ++u) {
      ci[u] = y0 + row;
      cj[u] = x0 + col;
      // (a lane past the box reads the box's first cell and drops it: a select, not a branch around the load; the index fits
      // 32 bits, xsize * ysize <= 2^31)
      in[u] = base + u * kWave + lane < n;
      const unsigned at = in[u] ? static_cast<unsigned>(ci[u]) * c.xsize + static_cast<unsigned>(cj[u]) : first_cell;
      v[u] = grid[at];
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
      in[u] = in[u] && v[u] >= f.v_min;  // occupied() as blocking_cutoff(occupied_threshold) states it (common.hpp)
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
