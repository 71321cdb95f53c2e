// Body layer for gfx950: the robots of a fleet as obstacles to one another, each a convex polygon (the footprint of
// footprint_kernel.hip), built from their poses every tick.  The disc's counterpart is fleet_layer_kernel.hip; no reference
// counterpart.  Compiled without FMA contraction: the test of a cell is footprint_cell_test.hpp's.
//
// The rule (include/ergodic_amd.h states it for callers): robot j is stamped when it is active, its pose is finite and its box
// touches the grid (classify's first test, as doubles); its body is the set of IN-GRID cells c with T(c, pose_j), T = the
// closed test of the cell's centre against the polygon placed at the pose (cell_inside), sine and cosine from tick_sincos.
// The verdict of a pose of robot i is the footprint's verdict on a grid in which every cell of every OTHER stamped robot's
// body is occupied.
//
// cover [ysize][xsize]   the number of stamped robots whose body holds the cell.  A reader takes robot i's own body out with
//            the very values the stamp used (the snapshot table: px, py, sine, cosine, stamped): n = cover[c]; if (n > 0 && i
//            stamped && T(c, snapshot_i)) n -= 1 -- the same function on the same doubles, so the subtraction matches the stamp
//            bit for bit.
// near       over the cells [-box, xsize + box) x [-box, ysize + box): the stamped robots whose cell (floor as doubles, no wrap)
//            lies within Chebyshev distance Rn = 2 ceil(r_out / res) + 2 = 2 box of this one.  Two polygons that share a cell
//            have their origins within 2 r_out, so their cells differ by at most ceil(2 r_out / res) <= Rn - 2 on either axis:
//            near - [own cell within Rn] == 0 proves that nobody else's body meets a polygon placed in this cell.  A filter,
//            never a verdict.
//
// An update is stream operations only: one clear over both maps (one allocation), one stamp kernel -- a wavefront per robot;
// per row of its box the lanes take the columns, 64 at a time, a ballot of T gives the covered runs, +1 at a run's start and -1
// behind its end into the difference map (a run cut by a chunk's end is closed and opened again at the same cell: the sums
// cancel); per row of its near square one span -- and fleet_layer_kernel.hip's row prefix sum over either map.  Integer sums:
// exact whatever the order of the atomics.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "common.hpp"
#include "footprint_cell_test.hpp"
#include "footprint_planes.hpp"
#include "twist_step.hpp"

namespace eea
{
namespace
{
// Every write lands inside its map: the box is clamped to the grid, the near square to the near map; the -1 behind a run that
// ends in a map's last column is dropped (nothing follows it in the row).
__global__ __launch_bounds__(kWave) void body_stamp_kernel(const CollisionParams c, const FootprintArgs f, const BodyView v,
                                                           const double* __restrict__ pose, const int* __restrict__ mask,
                                                           int* __restrict__ cover, int* __restrict__ near, double* __restrict__ snap)
{
  const unsigned r = blockIdx.x;
  if (r >= v.B) return;
  const int lane = threadIdx.x;
  const PlaneRegs pl = load_planes(f, lane);
  const double px = pose[3 * static_cast<size_t>(r)], py = pose[3 * static_cast<size_t>(r) + 1], th = pose[3 * static_cast<size_t>(r) + 2];
  bool stamped = (mask == nullptr || mask[r] != 0) && isfinite(px) && isfinite(py) && isfinite(th);
  Box b{ 0, -1, 0, -1 };
  double fx = 0.0, fy = 0.0;
  const double rb = static_cast<double>(f.box);
  if (stamped) {  // classify's first test
    fx = floor((px - c.xmin) / c.resolution);
    fy = floor((py - c.ymin) / c.resolution);
    const double xlast = static_cast<double>(c.xsize - 1u), ylast = static_cast<double>(c.ysize - 1u);
    stamped = fx + rb >= 0.0 && fx - rb <= xlast && fy + rb >= 0.0 && fy - rb <= ylast;
    if (stamped) {
      b.x0 = static_cast<int>(fmax(fx - rb, 0.0));
      b.x1 = static_cast<int>(fmin(fx + rb, xlast));
      b.y0 = static_cast<int>(fmax(fy - rb, 0.0));
      b.y1 = static_cast<int>(fmin(fy + rb, ylast));
    }
  }
  double sn = 0.0, cs = 0.0;
  if (stamped) tick_sincos(th, &sn, &cs);
  if (lane == 0) {
    double* const s = snap + static_cast<size_t>(kBodySnap) * r;
    s[0] = stamped ? px : 0.0;
    s[1] = stamped ? py : 0.0;
    s[2] = sn;
    s[3] = cs;
    s[4] = stamped ? 1.0 : 0.0;
  }
  if (!stamped) return;  // (wavefront-uniform)
  const int xsize = static_cast<int>(c.xsize);
  for (int i = b.y0; i <= b.y1; ++i) {
    int* const row = cover + static_cast<size_t>(i) * c.xsize;
    for (int j0 = b.x0; j0 <= b.x1; j0 += kWave) {
      const int j = j0 + lane;
      const bool in = j <= b.x1 && cell_inside(c, f, pl, i, j, px, py, sn, cs);
      const unsigned long long m = __ballot(in);
      if (in) {
        const bool left = lane > 0 && ((m >> (lane - 1)) & 1ull) != 0ull;
        const bool right = lane < kWave - 1 && ((m >> (lane + 1)) & 1ull) != 0ull;
        if (!left) atomicAdd(row + j, 1);
        if (!right && j + 1 < xsize) atomicAdd(row + j + 1, -1);
      }
    }
  }
  // the near square, clipped to the map (the robot's own cell lies inside the map: its box touches the grid)
  const double rn = static_cast<double>(v.Rn);
  const int nx0 = static_cast<int>(fmax(fx + rb - rn, 0.0)), nx1 = static_cast<int>(fmin(fx + rb + rn, static_cast<double>(v.near_w - 1)));
  const int ny0 = static_cast<int>(fmax(fy + rb - rn, 0.0)), ny1 = static_cast<int>(fmin(fy + rb + rn, static_cast<double>(v.near_h - 1)));
  for (int y = ny0 + lane; y <= ny1; y += kWave) {
    int* const row = near + static_cast<size_t>(y) * v.near_w;
    atomicAdd(row + nx0, 1);
    if (nx1 + 1 < v.near_w) atomicAdd(row + nx1 + 1, -1);
  }
}

constexpr int kShare = kBlock / kWave;

// footprint_check_kernel (footprint_kernel.hip) with the layer: one lane per pose, 64 poses per workgroup, the ambiguous ones
// shared among the four wavefronts.  Sine and cosine are the stamp's and the rollouts' (tick_sincos)
__global__ __launch_bounds__(kBlock) void body_check_kernel(const CollisionParams c, const FootprintArgs f, const BodyArgs a,
                                                            const int8_t* __restrict__ grid, const int* __restrict__ d_sq,
                                                            const double* __restrict__ pose, unsigned P, int* __restrict__ hit)
{
  const int lane = threadIdx.x % kWave;
  const int part = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const size_t q = static_cast<size_t>(blockIdx.x) * kWave + lane;
  const PlaneRegs pl = load_planes(f, lane);
  const bool live = q < P;
  double px = 0.0, py = 0.0, th = 0.0, sn = 0.0, cs = 0.0;
  Box b{ 0, -1, 0, -1 };
  int cls = kFree;
  Bodies bv{ a.v, 0.0, 0.0, 0.0, 0.0, false };
  if (live) {
    px = pose[3 * q];
    py = pose[3 * q + 1];
    th = pose[3 * q + 2];
    bv = load_bodies(a, q);
    // (without a grid the field has nothing to say: robots only)
    cls = classify_with(c, f, grid != nullptr ? d_sq : nullptr, px, py, th, b, bv);
  }
  unsigned long long todo = __ballot(cls == kAmbiguous);
  unsigned long long mine = 0ull;
  for (int i = 0; todo != 0ull; ++i) {
    const unsigned long long lowest = todo & (0ull - todo);
    if (i % kShare == part) mine |= lowest;
    todo ^= lowest;
  }
  const bool own = ((mine >> lane) & 1ull) != 0ull;
  if (own) tick_sincos(th, &sn, &cs);
  int verdict = cls == kHit;
  while (mine != 0ull) {
    const int src = __ffsll(static_cast<long long>(mine)) - 1;
    mine &= mine - 1ull;
    const bool h = resolve(c, f, pl, grid, src, px, py, sn, cs, b, lane, bv);
    if (lane == src) verdict = h;
  }
  if (live && (own || (part == 0 && cls != kAmbiguous))) hit[q] = verdict;
}
}  // namespace

hipError_t launch_body_layer_update(const CollisionParams& c, const FootprintArgs& f, const BodyView& v, int* d_maps, double* d_snap,
                                    const double* d_pose, const int* d_mask, hipStream_t s)
{
  const size_t n_cover = static_cast<size_t>(c.xsize) * c.ysize, n_near = static_cast<size_t>(v.near_w) * v.near_h;
  int* const d_cover = d_maps;
  int* const d_near = d_maps + n_cover;
  hipError_t e = hipMemsetAsync(d_maps, 0, sizeof(int) * (n_cover + n_near), s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(body_stamp_kernel, dim3(v.B), dim3(kWave), 0, s, c, f, v, d_pose, d_mask, d_cover, d_near, d_snap);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  e = launch_fleet_row_scan(d_cover, static_cast<int>(c.xsize), static_cast<int>(c.ysize), s);
  if (e != hipSuccess) return e;
  return launch_fleet_row_scan(d_near, v.near_w, v.near_h, s);
}

hipError_t launch_body_check(const CollisionParams& c, const FootprintArgs& f, const BodyArgs& a, const int8_t* d_grid,
                             const int* d_sq, const double* d_pose, unsigned P, int* d_hit, hipStream_t s)
{
  if (P == 0) return hipSuccess;
  const dim3 blocks(static_cast<unsigned>((static_cast<size_t>(P) + kWave - 1) / kWave));
  hipLaunchKernelGGL(body_check_kernel, blocks, dim3(kBlock), 0, s, c, f, a, d_grid, d_sq, d_pose, P, d_hit);
  return hipGetLastError();
}
}  // namespace eea
