// Distance field for gfx950: the exact Euclidean distance transform of a GridMap's occupied cells, and queries through it.
// No reference counterpart (the reference README lists a distance field under "Future Improvements"): this is the gap-free
// notion of distance beside the reference-exact ring search of collision_kernel.hip / clearance_kernel.hip.  Integer work up
// to the last lines of a query; those are compiled without FMA contraction.
//
// sq (i, j) = min over occupied (i', j') of (i - i')^2 + (j - j')^2, nearest (i, j) = the row-major index of the cell that
// attains it, the smallest index among equals.  Two separable passes over one int plane, in place in d_sq:
//   columns   dy (i, j) = signed row offset from i to the nearest occupied cell of column j, the smaller row on a tie.  A
//             workgroup owns 16 columns and cuts them into 64 strips of rows, a thread per column and strip.  A thread notes
//             the first and last occupied row of its strip in LDS, takes the nearest occupied rows outside its strip from
//             the other strips' notes (the prefix max / suffix min of an associative scan), then walks its strip down
//             (nearest at or above, written to the plane) and up (nearest at or below; the two are combined in place).
//             Measured on 1024 x 1024 (profiles/distance_field.txt): 64 columns x 16 strips leave the pass on 16 workgroups,
//             and every build takes 30 us longer (53 against 22 us on an empty grid).
//   rows      sq (i, j) = min over j' of (j - j')^2 + dy (i, j')^2.  A workgroup holds row i of dy in LDS; a lane owns a j
//             and walks outwards over j -+ k while k^2 <= best -- <=, not <: a candidate at k^2 == best can still win the tie
//             by index.  Neighbouring lanes read neighbouring LDS words.  The minimum is over one 64-bit key (sq, index).
// The tie rule survives the separation: every cell of column j' that attains the minimal sq from (i, j) lies at that column's
// minimal |dy|, so it is enough that the column pass keeps the smaller row among the (at most two) cells at that |dy|; the
// row pass then minimises (sq, index) over the columns.  All minima are integer: order-free, bit-reproducible.
// Cost: columns O(cells); rows O(cells * walk), the walk being the distance to the nearest cell in cells -- a grid whose
// only occupied cell sits in a corner walks whole rows (measured: profiles/distance_field.txt).
#include <cfloat>
#include <cmath>
#include <cstdint>

#include "../../include/ergodic_amd.h"
#include "common.hpp"
#include "grid_cell.hpp"  // world_to_grid (grid.cpp:143-159), ClearanceAnswer, write_answer

namespace eea
{
namespace
{
constexpr int kNoCell = INT32_MIN;  // dy of a column without an occupied cell
constexpr int kColumns = 16;        // columns per workgroup of the column pass
constexpr int kStrips = 64;         // ... and the strips of rows it cuts them into: a thread per column and strip
constexpr int kFar = 1 << 20;       // a row distance no grid has (sides <= kDistanceMaxSide)

static_assert(kDistanceMaxSide == EEA_DISTANCE_MAX_SIDE, "the header states the limit");
static_assert(2ll * (kDistanceMaxSide - 1) * (kDistanceMaxSide - 1) < INT32_MAX, "sq fits an int");
static_assert(static_cast<long long>(kDistanceMaxSide) * kDistanceMaxSide < INT32_MAX, "a cell's index fits an int");
static_assert(kDistanceMaxSide * sizeof(int) <= 64 * 1024, "a row of dy fits a workgroup's LDS");

// column pass: plane [ysize][xsize] <- dy.  occupied: cell >= v_min (blocking_cutoff, common.hpp: checkCell's test as an integer)
__global__ __launch_bounds__(kColumns* kStrips) void distance_columns_kernel(const int8_t* __restrict__ grid, int xsize, int ysize,
                                                                            int v_min, int* __restrict__ plane)
{
  __shared__ int s_first[kStrips][kColumns], s_last[kStrips][kColumns];  // occupied rows of a strip, -1: none
  const int col = threadIdx.x % kColumns, strip = threadIdx.x / kColumns;
  const int j = blockIdx.x * kColumns + col;
  const bool live = j < xsize;
  const int rows = (ysize + kStrips - 1) / kStrips;
  const int i0 = min(strip * rows, ysize), i1 = min(i0 + rows, ysize);
  int first = -1, last = -1;
  if (live) {
    for (int i = i0; i < i1; ++i) {
      if (grid[static_cast<size_t>(i) * xsize + j] >= v_min) {
        if (first < 0) first = i;
        last = i;
      }
    }
  }
  s_first[strip][col] = first;
  s_last[strip][col] = last;
  __syncthreads();
  if (!live) return;
  int up = -1, down = -1;  // nearest occupied row above / below the strip
  for (int s = 0; s < strip; ++s) {
    const int l = s_last[s][col];
    if (l >= 0) up = l;
  }
  for (int s = kStrips - 1; s > strip; --s) {
    const int f = s_first[s][col];
    if (f >= 0) down = f;
  }
  for (int i = i0; i < i1; ++i) {
    const size_t at = static_cast<size_t>(i) * xsize + j;
    if (grid[at] >= v_min) up = i;
    plane[at] = up;
  }
  for (int i = i1 - 1; i >= i0; --i) {
    int* const at = &plane[static_cast<size_t>(i) * xsize + j];
    const int u = *at;  // (this thread's own store)
    if (u == i) down = i;
    const int du = u < 0 ? kFar : i - u, dd = down < 0 ? kFar : down - i;
    *at = du <= dd ? (du == kFar ? kNoCell : -du) : dd;  // the smaller row on a tie
  }
}

__device__ __forceinline__ unsigned long long distance_key(int k, int d, int i, int j, int xsize)
{
  return (static_cast<unsigned long long>(static_cast<unsigned>(k * k + d * d)) << 32) | static_cast<unsigned>((i + d) * xsize + j);
}

// row pass: workgroup i turns row i of the plane from dy into sq, in place (the row is in LDS before anything is written)
__global__ __launch_bounds__(kBlock) void distance_rows_kernel(int xsize, int* __restrict__ plane, int* __restrict__ nearest)
{
  extern __shared__ int s_dy[];  // [xsize]
  const int i = blockIdx.x;
  int* const row = plane + static_cast<size_t>(i) * xsize;
  int* const near_row = nearest == nullptr ? nullptr : nearest + static_cast<size_t>(i) * xsize;
  int any = 0;
  for (int j = threadIdx.x; j < xsize; j += kBlock) {
    const int d = row[j];
    s_dy[j] = d;
    any |= d != kNoCell;
  }
  // (a column with an occupied cell has a dy in every row: a row without any dy means a grid without an occupied cell)
  if (!__syncthreads_or(any)) {
    for (int j = threadIdx.x; j < xsize; j += kBlock) {
      row[j] = -1;
      if (near_row != nullptr) near_row[j] = -1;
    }
    return;
  }
  for (int j = threadIdx.x; j < xsize; j += kBlock) {
    unsigned long long best = ~0ull;
    const int d0 = s_dy[j];
    if (d0 != kNoCell) best = distance_key(0, d0, i, j, xsize);
    const int k_end = max(j, xsize - 1 - j);
    for (int k = 1; k <= k_end && static_cast<unsigned>(k * k) <= static_cast<unsigned>(best >> 32); ++k) {
      if (j - k >= 0) {
        const int d = s_dy[j - k];
        if (d != kNoCell) best = min(best, distance_key(k, d, i, j - k, xsize));
      }
      if (j + k < xsize) {
        const int d = s_dy[j + k];
        if (d != kNoCell) best = min(best, distance_key(k, d, i, j + k, xsize));
      }
    }
    row[j] = static_cast<int>(best >> 32);
    if (near_row != nullptr) near_row[j] = static_cast<int>(best & 0xffffffffull);
  }
}

// ---- queries ------------------------------------------------------------------------------------------------------
struct DistanceField
{
  const int* sq;
  const int* nearest;  // may be null when no output needs the cell
};

// sqrt of a positive integer below 2^31, correctly rounded: the device's sqrt followed by one Markstein step (the residual
// x - r * r is exact in an fma; r + residual / (2 r) then rounds to the correctly rounded root whenever r was within an
// ulp of it, and leaves a correctly rounded r as it is)
__device__ __forceinline__ double sqrt_rn(double x)
{
  const double r = sqrt(x);
  return fma(fma(-r, r, x), 0.5 / r, r);
}

// the answer of one pose's cell: what eea_distance_query_batch documents
__device__ __forceinline__ ClearanceAnswer distance_answer(const CollisionParams& c, double boundary_radius, const DistanceField& f,
                                                           unsigned j, unsigned i, bool want_cell)
{
  ClearanceAnswer a{ EEA_COLLISION_OFF_GRID, -1, 0, 0, 0.0, 0.0, 0.0 };
  if (!((i <= c.ysize - 1u) && (j <= c.xsize - 1u))) return a;  // gridBounds (grid.cpp:96-100)
  const size_t at = static_cast<size_t>(i) * c.xsize + j;
  const int sq = f.sq[at];
  if (sq < 0) {
    a.msg = EEA_COLLISION_NONE;
    a.dmin = a.d0 = a.d1 = DBL_MAX;
    return a;
  }
  a.msg = sq <= c.r_col * c.r_col ? EEA_COLLISION_CRASH : EEA_COLLISION_OBSTACLE;
  a.sq = sq;
  a.dmin = (sq == 0 ? 0.0 : sqrt_rn(static_cast<double>(sq))) * c.resolution - boundary_radius;
  if (want_cell) {
    const int n = f.nearest[at];
    const int ni = n / static_cast<int>(c.xsize), nj = n - ni * static_cast<int>(c.xsize);
    a.dx = nj - static_cast<int>(j);
    a.dy = ni - static_cast<int>(i);
    a.d0 = c.resolution * static_cast<double>(a.dx);
    a.d1 = c.resolution * static_cast<double>(a.dy);
  }
  return a;
}

// one lane per pose
__global__ __launch_bounds__(kBlock) void distance_query_kernel(const CollisionParams c, double boundary_radius, const DistanceField f,
                                                                const double* __restrict__ pose, unsigned P, int* __restrict__ out,
                                                                double* __restrict__ dmin, double* __restrict__ disp)
{
  const size_t q = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (q >= P) return;
  unsigned j, i;
  world_to_grid(c, pose[3 * q], pose[3 * q + 1], j, i);
  write_answer(out, dmin, disp, q, distance_answer(c, boundary_radius, f, j, i, out != nullptr || disp != nullptr));
}

// one wavefront per trajectory: lanes take the steps lane, lane + 64, ...; the worst step is the smallest key
// (class / sq, step) -- 0: off the grid, 1 + sq: on it, all ones: on it with an empty field -- so the earliest among equals
__global__ __launch_bounds__(kBlock) void distance_traj_min_kernel(const CollisionParams c, double boundary_radius, const DistanceField f,
                                                                   const double* __restrict__ traj, unsigned B, unsigned T,
                                                                   int* __restrict__ out, int* __restrict__ step,
                                                                   double* __restrict__ dmin)
{
  const size_t b = static_cast<size_t>(blockIdx.x) * (kBlock / kWave) + threadIdx.x / kWave;  // wavefront-uniform
  if (b >= B) return;
  const unsigned lane = threadIdx.x % kWave;
  const double* const x = traj + b * T * 3;
  unsigned long long best = ~0ull;
  for (unsigned t = lane; t < T; t += kWave) {
    unsigned j, i;
    world_to_grid(c, x[3 * static_cast<size_t>(t)], x[3 * static_cast<size_t>(t) + 1], j, i);
    unsigned cls = 0u;
    if ((i <= c.ysize - 1u) && (j <= c.xsize - 1u)) {
      const int sq = f.sq[static_cast<size_t>(i) * c.xsize + j];
      cls = sq < 0 ? 0xffffffffu : 1u + static_cast<unsigned>(sq);
    }
    const unsigned long long key = (static_cast<unsigned long long>(cls) << 32) | t;
    best = key < best ? key : best;
  }
#pragma unroll
  for (int m = kWave / 2; m >= 1; m >>= 1) {
    const unsigned long long other = __shfl_xor(best, m, kWave);
    best = other < best ? other : best;
  }
  if (lane != 0) return;
  const unsigned t = static_cast<unsigned>(best & 0xffffffffull);
  unsigned j, i;
  world_to_grid(c, x[3 * static_cast<size_t>(t)], x[3 * static_cast<size_t>(t) + 1], j, i);
  write_answer(out, dmin, nullptr, b, distance_answer(c, boundary_radius, f, j, i, out != nullptr));
  if (step != nullptr) step[b] = static_cast<int>(t);
}
}  // namespace

hipError_t launch_distance_field(const CollisionParams& c, const int8_t* d_grid, int* d_sq, int* d_nearest, hipStream_t s)
{
  const int xsize = static_cast<int>(c.xsize), ysize = static_cast<int>(c.ysize);
  hipLaunchKernelGGL(distance_columns_kernel, dim3((c.xsize + kColumns - 1) / kColumns), dim3(kColumns * kStrips), 0, s, d_grid, xsize,
                     ysize, blocking_cutoff(c.occupied_threshold), d_sq);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(distance_rows_kernel, dim3(c.ysize), dim3(kBlock), c.xsize * sizeof(int), s, xsize, d_sq, d_nearest);
  return hipGetLastError();
}

hipError_t launch_distance_query(const CollisionParams& c, double boundary_radius, const int* d_sq, const int* d_nearest,
                                 const double* d_pose, unsigned P, int* d_out, double* d_dmin, double* d_disp, hipStream_t s)
{
  if (P == 0) return hipSuccess;
  const dim3 blocks(static_cast<unsigned>((static_cast<size_t>(P) + kBlock - 1) / kBlock));
  hipLaunchKernelGGL(distance_query_kernel, blocks, dim3(kBlock), 0, s, c, boundary_radius, DistanceField{ d_sq, d_nearest }, d_pose, P,
                     d_out, d_dmin, d_disp);
  return hipGetLastError();
}

hipError_t launch_distance_traj_min(const CollisionParams& c, double boundary_radius, const int* d_sq, const int* d_nearest,
                                    const double* d_traj, unsigned B, unsigned T, int* d_out, int* d_step, double* d_dmin,
                                    hipStream_t s)
{
  if (B == 0) return hipSuccess;
  constexpr unsigned per_block = kBlock / kWave;
  const dim3 blocks(static_cast<unsigned>((static_cast<size_t>(B) + per_block - 1) / per_block));
  hipLaunchKernelGGL(distance_traj_min_kernel, blocks, dim3(kBlock), 0, s, c, boundary_radius, DistanceField{ d_sq, d_nearest }, d_traj, B,
                     T, d_out, d_step, d_dmin);
  return hipGetLastError();
}
}  // namespace eea
