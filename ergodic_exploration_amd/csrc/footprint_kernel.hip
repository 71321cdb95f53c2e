// Footprint collision for gfx950: a convex polygon base placed at a pose, against the occupied cells of a GridMap, with the
// distance field (distance_kernel.hip) as a filter.  No reference counterpart (the reference README lists "model the robot's
// base as a polygon" and "use a distance field for detecting obstacle cells" under "Future Improvements").  Compiled without
// FMA contraction: the test of one cell is the products and sums include/ergodic_amd.h writes down, each rounded on its own.
//
// The verdict of a pose (px, py, th), all three finite: some in-grid cell (i, j) is occupied (checkCell's test as blocking_cutoff states it) and its
// centre (j * res + res / 2 + xmin, i * res + res / 2 + ymin) (grid.cpp:126-131), taken into the body frame, satisfies every
// half-plane nx_k * bx + ny_k * by <= h_k.  A pose with a non-finite component collides with nothing.
//
// classify   One lane per pose (or per step of a trajectory).  fx = floor((px - xmin) / res) and fy stay doubles until they are
//            known to be inside the grid -- NOT world_to_grid: its x86 wrap folds poses a multiple of 2^32 cells away on to the
//            grid and its == size step takes the column fx == xsize and the row fy == ysize, outside the grid, into the last
//            cells, and either would make a false sure hit.  The box of
//            cells within `box` of (fx, fy) is clamped to the grid as doubles, then converted; a box that misses the grid is
//            free.  A pose with a cell and a field reads ONE int: 0 <= sq <= sq_hit is a hit, sq < 0 or sq > sq_free is free
//            (footprint_planes.hpp has the bounds).  Everything else is ambiguous.
// resolve    The wavefront takes the ambiguous lanes one after the other (a ballot, its bits in order): the pose and its box are
//            broadcast, the 64 lanes stride the box row-major -- neighbouring lanes read neighbouring bytes of a grid row -- four
//            cells per lane and chunk, the half-planes are tested only in a chunk with an occupied cell, and the box is left at
//            the first chunk with a hit.  Sine and cosine are formed by all ambiguous lanes at once, before the first is
//            resolved.  A wavefront resolves its poses one after the other, and that chain of instructions is what a call costs
//            (a call took the same time for 4096 and for 65 536 poses; more cells per lane and chunk, i.e. fewer rounds of loads
//            and more arithmetic per round, did not help).  So the pose kernel gives 64 poses to a workgroup: each of its four wavefronts classifies all 64 (one load each) and takes
//            every fourth ambiguous pose; every pose is written by exactly one of them, and they share nothing.
// The half-planes travel in the kernel arguments; lane k of a wavefront keeps plane k in registers and the test reads it with
// v_readlane.  (Read from the kernel arguments inside the test -- scalar loads at a wavefront-uniform index -- every cell would
// wait for three loads per plane in a chain that has nothing to hide them behind.)  No LDS, no atomics, no wait between
// wavefronts; every loop is bounded by the box: box <= 1025, at most 2051^2 cells.
#include <cmath>
#include <cstdint>

#include "../../include/ergodic_amd.h"
#include "common.hpp"
#include "footprint_planes.hpp"
#include "footprint_cell_test.hpp"
#include "grid_cell.hpp"

namespace eea
{
static_assert(kFootprintMaxVertices == EEA_FOOTPRINT_MAX_VERTICES, "the header states the limit");

namespace
{
constexpr int kShare = kBlock / kWave;  // wavefronts that share the ambiguous poses of 64

// one lane per pose, 64 poses per workgroup: wavefront `part` of the four resolves the ambiguous poses part, part + 4, ... (in
// the ballot's order) and writes those; wavefront 0 also writes the poses the field decided
__global__ __launch_bounds__(kBlock) void footprint_check_kernel(const CollisionParams c, const FootprintArgs f,
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
  if (live) {
    px = pose[3 * q];
    py = pose[3 * q + 1];
    th = pose[3 * q + 2];
    cls = classify(c, f, d_sq, px, py, th, b);
  }
  unsigned long long todo = __ballot(cls == kAmbiguous);
  // this wavefront's share of them
  unsigned long long mine = 0ull;
  for (int i = 0; todo != 0ull; ++i) {
    const unsigned long long lowest = todo & (0ull - todo);
    if (i % kShare == part) mine |= lowest;
    todo ^= lowest;
  }
  const bool own = ((mine >> lane) & 1ull) != 0ull;
  if (own) sincos(th, &sn, &cs);
  int verdict = cls == kHit;
  while (mine != 0ull) {
    const int src = __ffsll(static_cast<long long>(mine)) - 1;
    mine &= mine - 1ull;
    const bool h = resolve(c, f, pl, grid, src, px, py, sn, cs, b, lane);
    if (lane == src) verdict = h;
  }
  if (live && (own || (part == 0 && cls != kAmbiguous))) hit[q] = verdict;
}

// one wavefront per trajectory: the steps in chunks of 64, a lane per step; the first chunk with a hit answers
__global__ __launch_bounds__(kBlock) void footprint_traj_first_kernel(const CollisionParams c, const FootprintArgs f,
                                                                      const int8_t* __restrict__ grid, const int* __restrict__ d_sq,
                                                                      const double* __restrict__ traj, unsigned B, unsigned T,
                                                                      int* __restrict__ step)
{
  const size_t t_id = static_cast<size_t>(blockIdx.x) * (kBlock / kWave) + threadIdx.x / kWave;  // wavefront-uniform
  if (t_id >= B) return;
  const int lane = threadIdx.x % kWave;
  const PlaneRegs pl = load_planes(f, lane);
  const double* const x = traj + t_id * T * 3;
  int first = -1;
  for (unsigned t0 = 0; t0 < T && first < 0; t0 += kWave) {
    const unsigned t = t0 + static_cast<unsigned>(lane);
    double px = 0.0, py = 0.0, th = 0.0, sn = 0.0, cs = 0.0;
    Box b{ 0, -1, 0, -1 };
    int cls = kFree;
    if (t < T) {
      px = x[3 * static_cast<size_t>(t)];
      py = x[3 * static_cast<size_t>(t) + 1];
      th = x[3 * static_cast<size_t>(t) + 2];
      cls = classify(c, f, d_sq, px, py, th, b);
    }
    // only the steps before the chunk's first sure hit can still be the answer
    const unsigned long long sure = __ballot(cls == kHit);
    unsigned long long todo = __ballot(cls == kAmbiguous);
    if (sure != 0ull) {
      first = __ffsll(static_cast<long long>(sure)) - 1;
      todo &= (1ull << first) - 1ull;
      first += static_cast<int>(t0);
    }
    if (cls == kAmbiguous && ((todo >> lane) & 1ull) != 0ull) sincos(th, &sn, &cs);
    while (todo != 0ull) {
      const int src = __ffsll(static_cast<long long>(todo)) - 1;
      todo &= todo - 1ull;
      if (resolve(c, f, pl, grid, src, px, py, sn, cs, b, lane)) {
        first = static_cast<int>(t0) + src;
        break;
      }
    }
  }
  if (lane == 0) step[t_id] = first;
}
}  // namespace

hipError_t launch_footprint_check(const CollisionParams& c, const FootprintArgs& f, const int8_t* d_grid, const int* d_sq,
                                  const double* d_pose, unsigned P, int* d_hit, hipStream_t s)
{
  if (P == 0) return hipSuccess;
  const dim3 blocks(static_cast<unsigned>((static_cast<size_t>(P) + kWave - 1) / kWave));  // 64 poses per workgroup
  hipLaunchKernelGGL(footprint_check_kernel, blocks, dim3(kBlock), 0, s, c, f, d_grid, d_sq, d_pose, P, d_hit);
  return hipGetLastError();
}

hipError_t launch_footprint_traj_first(const CollisionParams& c, const FootprintArgs& f, const int8_t* d_grid, const int* d_sq,
                                       const double* d_traj, unsigned B, unsigned T, int* d_step, hipStream_t s)
{
  if (B == 0) return hipSuccess;
  constexpr unsigned per_block = kBlock / kWave;
  const dim3 blocks(static_cast<unsigned>((static_cast<size_t>(B) + per_block - 1) / per_block));
  hipLaunchKernelGGL(footprint_traj_first_kernel, blocks, dim3(kBlock), 0, s, c, f, d_grid, d_sq, d_traj, B, T, d_step);
  return hipGetLastError();
}
}  // namespace eea
