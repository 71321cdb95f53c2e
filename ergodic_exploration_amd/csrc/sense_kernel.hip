// Range sensing of a simulated fleet (include/ergodic_amd.h, eea_sense_reveal_batch / eea_grid_census): every robot casts 8R
// rays through a ground-truth occupancy grid and the cells the rays cross become known -- the counterpart of
// integrate_twist_kernel (the simulated fleet's motion).  The reference has the consumer of such a map (entropy(),
// numerics.hpp:164-179: an unknown cell is worth 0.7, a known one 1e-3) and describes the sensor in words (README.md:74-76,
// "simulating a 360 degree range finder"); its OccupancyMapper (mapping.cpp) fuses real scans and is NOT what this is.
//
//  - integers only: the robot's cell is world2Grid of grid_cell.hpp (the collision kernels' definition), a ray's step s sits
//    at sgn(m) ((2 s |m| + R) div 2R) per axis -- formed here by adding 2|m| per step to a remainder that starts at R and
//    wraps at 2R, which is that quotient exactly (2|m| <= 2R: at most one wrap per step) --, and "blocks a ray" is
//    cell >= cutoff, cutoff = the smallest int8 value v with !(v / 100.0 < occupied_threshold) found on the host (common.hpp; the
//    quotient is monotone in v: checkCell's test, collision.cpp:216-243 with grid.cpp:177-184, is a threshold on the cell);
//  - every write to a cell of `known` stores that cell of `truth`, whoever makes it: robots, rays and calls may overlap in
//    any order, no atomics, byte (vector) stores only;
//  - one workgroup of 256 threads per robot, a thread per ray (8R rays: ceil(8R / 256) rounds, the last one ragged).
//    R <= 127: the robot's (2R + 1)^2 window is staged in LDS as one byte per cell (bit 0: blocks; rows read coalesced, one
//    wavefront per row), the rays march in LDS and set bit 1 of the cells they cross (every writer of a byte writes the
//    same value, bit 0 is never changed), then the marked cells are copied truth -> known row by row.  The overlap of the
//    rays near the robot costs LDS cycles only; global memory sees each window byte at most twice, in rows.  The window's
//    rows are 2R + 1 bytes, an odd count: the cells of a column sit in different banks.
//    R > 127 (the window passes 64 KB): the rays march in global memory, a dependent byte load and a byte store per step.
//    Both compute the contract bit for bit (tests/test_gpu_sense.py holds each to tests/sense_restatement.py).
//  What a scan is around its staging and write-out -- the launch block, the robot of a workgroup's turn, the march on the staged
//  window -- lives in sense_rays.hpp, for this file and evidence_kernel.hip; the census' classes, reduction and 16-byte split
//  live in grid_census.hpp, for grid_census_kernel and the evidence grid's publish kernel.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.hpp"
#include "grid_census.hpp"  // Census, count_value, census_commit, stream_split: shared with evidence_kernel.hip
#include "sense_rays.hpp"   // the rays (shared with the candidate fields) and the scan's prologue and march (with evidence_kernel.hip)

namespace eea
{
namespace
{
constexpr unsigned kSenseLdsMaxR = 127;  // (2R + 1)^2 bytes <= 64 KB

struct SenseParams : ScanParams<int8_t>  // out: `known`
{
};

__global__ __launch_bounds__(kBlock) void sense_reveal_lds_kernel(const SenseParams p)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char s_cell[];  // [2R + 1][2R + 1]: bit 0 blocks, bit 1 revealed
  const int R = p.R, W = 2 * R + 1, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (unsigned b = blockIdx.x; b < p.P; b += gridDim.x) {
    __syncthreads();  // the robot before has read the window
    unsigned i0, j0;
    if (!robot_cell(p, b, i0, j0)) continue;  // (uniform over the workgroup)
    const Clip w = clip_of(p.c, i0, j0, R);
    for (int dy = w.ylo + wave; dy <= w.yhi; dy += kBlock / 64) {
      const int8_t* const trow = p.truth + cell_index(p.c, i0, j0, 0, dy);
      unsigned char* const srow = s_cell + (dy + R) * W + R;
      for (int dx = w.xlo + lane; dx <= w.xhi; dx += 64) srow[dx] = trow[dx] >= p.cutoff ? 1 : 0;
    }
    __syncthreads();
    if (tid == 0) s_cell[R * W + R] |= 2;  // the robot's own cell (no ray visits offset (0, 0))
    march_window(p, b, w, s_cell);
    __syncthreads();
    for (int dy = w.ylo + wave; dy <= w.yhi; dy += kBlock / 64) {
      const size_t g0 = cell_index(p.c, i0, j0, 0, dy);
      const unsigned char* const srow = s_cell + (dy + R) * W + R;
      for (int dx = w.xlo + lane; dx <= w.xhi; dx += 64) {
        if (srow[dx] & 2) p.out[g0 + dx] = p.truth[g0 + dx];
      }
    }
  }
}

__global__ __launch_bounds__(kBlock) void sense_reveal_global_kernel(const SenseParams p)
{
  const int R = p.R, tid = threadIdx.x;
  for (unsigned b = blockIdx.x; b < p.P; b += gridDim.x) {
    unsigned i0, j0;
    if (!robot_cell(p, b, i0, j0)) continue;
    const Clip w = clip_of(p.c, i0, j0, R);
    if (tid == 0) {
      const size_t g = cell_index(p.c, i0, j0, 0, 0);
      p.out[g] = p.truth[g];
    }
    for (int q = tid; q < 8 * R; q += kBlock) {
      const int range = march(q, R, w, [&](int dx, int dy) {
        const size_t g = cell_index(p.c, i0, j0, dx, dy);
        const int8_t t = p.truth[g];
        p.out[g] = t;
        return t >= p.cutoff;
      });
      if (p.ranges != nullptr) p.ranges[static_cast<size_t>(b) * 8u * R + q] = range;
    }
  }
}

// ---- census (grid_census.hpp) ------------------------------------------------------------------
// 16 bytes per load from the grid's first 16-byte boundary on; the bytes in front of it and behind the last whole load one
// by one (at most 15 each: the first threads of the launch take them).  d_counts was zeroed on the stream.
__global__ __launch_bounds__(kBlock) void grid_census_kernel(const int8_t* __restrict__ grid, size_t n, int cutoff,
                                                             unsigned long long* __restrict__ counts)
{
  const StreamSplit sp = stream_split<1>(reinterpret_cast<uintptr_t>(grid), n);
  const size_t t = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x, stride = static_cast<size_t>(gridDim.x) * kBlock;
  Census cnt{ 0u, 0u, 0u };
  const uint4* const body = reinterpret_cast<const uint4*>(grid + sp.head);
  for (size_t ch = t; ch < sp.chunks; ch += stride) {
    const uint4 v = body[ch];
    const unsigned word[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int k = 0; k < 4; ++k) count_value(cnt, static_cast<int8_t>((word[a] >> (8 * k)) & 0xffu), cutoff);
  }
  if (t < sp.head) count_value(cnt, grid[t], cutoff);
  if (t < n - sp.tail0) count_value(cnt, grid[sp.tail0 + t], cutoff);
  census_commit(cnt, counts);
}
}  // namespace

hipError_t launch_sense_reveal(const CollisionParams& c, unsigned range_cells, const int8_t* d_truth, int8_t* d_known,
                               const double* d_pose, const int* d_mask, unsigned P, int* d_ranges, hipStream_t s)
{
  if (P == 0) return hipSuccess;
  SenseParams p;
  size_t window = 0;
  const unsigned blocks = scan_launch(c, range_cells, d_truth, d_known, d_pose, d_mask, d_ranges, P, p, &window);
  if (range_cells <= kSenseLdsMaxR) {
    hipLaunchKernelGGL(sense_reveal_lds_kernel, dim3(blocks), dim3(kBlock), window, s, p);
  } else {
    hipLaunchKernelGGL(sense_reveal_global_kernel, dim3(blocks), dim3(kBlock), 0, s, p);
  }
  return hipGetLastError();
}

hipError_t launch_grid_census(const CollisionParams& c, const int8_t* d_grid, unsigned long long* d_counts, hipStream_t s)
{
  const size_t n = static_cast<size_t>(c.xsize) * c.ysize;
  hipError_t e = hipMemsetAsync(d_counts, 0, 3 * sizeof(unsigned long long), s);
  if (e != hipSuccess) return e;
  const size_t want = (n / 16u + kBlock - 1) / kBlock + 1;  // (+ 1: the head and tail bytes when there is no whole load)
  const unsigned blocks = want < 2048u ? static_cast<unsigned>(want) : 2048u;
  hipLaunchKernelGGL(grid_census_kernel, dim3(blocks), dim3(kBlock), 0, s, d_grid, n, blocking_cutoff(c.occupied_threshold),
                     d_counts);
  return hipGetLastError();
}
}  // namespace eea
