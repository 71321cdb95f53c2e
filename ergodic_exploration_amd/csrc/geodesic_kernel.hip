// Geodesic field of a grid (include/ergodic_amd.h, eea_geodesic_field / eea_geodesic_path_batch / eea_set_target_reachable):
// the cost of the cheapest 5-7 chamfer move sequence through traversable cells from a set of source cells to every cell, -1
// where there is none; the descent of that field from a pose; and the value grid of a target restricted to reachable cells.
// The build is geodesic_tile.hpp's rounds on 32-bit costs (CostCell), straight on d_geo; a source stores 0 into its cell.
//  - the path: one lane per pose walks down the field, serially.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/ergodic_amd.h"
#include "common.hpp"
#include "gain_tile.hpp"  // candidate_values, values_grid: the value grid's body and launch shape, shared with the candidate fields
#include "geodesic_tile.hpp"

namespace eea
{
static_assert(kGeodesicTileX == EEA_GEODESIC_TILE_X && kGeodesicTileY == EEA_GEODESIC_TILE_Y, "the header publishes the tile");

namespace
{
__global__ __launch_bounds__(kBlock) void geodesic_init_kernel(const CollisionParams c, const GeodesicWs w, const GeodesicArgs a,
                                                              const int8_t* __restrict__ grid, const int* __restrict__ sq,
                                                              int* __restrict__ geo, unsigned* __restrict__ state)
{
  const size_t cells = static_cast<size_t>(c.xsize) * c.ysize;
  const size_t n = static_cast<size_t>(gridDim.x) * kBlock, t0 = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  for (size_t g = t0; g < cells; g += n) {
    w.trav[g] = traversable(c, a, grid[g], sq, g) ? 1 : 0;
    if (!a.keep_field) geo[g] = -1;
  }
  reset_rounds(w, state, t0, n);
}

// one lane per source
__global__ __launch_bounds__(kBlock) void geodesic_seed_kernel(const CollisionParams c, const GeodesicArgs a,
                                                              const int8_t* __restrict__ grid, const double* __restrict__ pose,
                                                              const int* __restrict__ src, int* __restrict__ geo,
                                                              unsigned* __restrict__ state)
{
  const size_t q = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  size_t at;
  if (q >= static_cast<size_t>(a.P) + a.n_cells || !source_cell(c, a, grid, pose, src, q, at)) return;
  geo[at] = 0;  // (every writer of this launch stores 0)
  atomicAdd(&state[2], 1u);
}

__global__ __launch_bounds__(kBlock) void geodesic_round_kernel(const GeodesicWs w, unsigned xsize, unsigned ysize, unsigned r,
                                                               unsigned* geo, unsigned* state)
{
  tile_round<CostCell>(w, geo, xsize, ysize, r, state);
}

__global__ void geodesic_close_kernel(const GeodesicWs w, unsigned last, unsigned* state) { close_rounds(w, last, state); }

__global__ __launch_bounds__(kBlock) void geodesic_path_kernel(const CollisionParams c, const int* __restrict__ geo,
                                                              const double* __restrict__ pose, unsigned P, unsigned n_steps,
                                                              double* __restrict__ path, int* __restrict__ len)
{
  const size_t q = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (q >= P) return;
  double wx = pose[3 * q], wy = pose[3 * q + 1], wth = pose[3 * q + 2];
  double* const out = path + q * n_steps * 3;
  unsigned j, i;
  world_to_grid(c, wx, wy, j, i);
  const bool in_grid = (i <= c.ysize - 1u) && (j <= c.xsize - 1u);  // gridBounds (grid.cpp:96-100)
  int here = in_grid ? geo[static_cast<size_t>(i) * c.xsize + j] : -1;
  int moves = here < 0 ? -1 : 0;
  unsigned written = 0;
  if (here >= 0) {
    // until a step is written the rows hold the centre of the pose's own cell with the pose's heading
    wx = centre_x(c, j);
    wy = centre_y(c, i);
    int ci = static_cast<int>(i), cj = static_cast<int>(j);
    while (here > 0 && written < n_steps) {
      const int k = descend<false>(c, geo, nullptr, 0, ci, cj, here);
      if (k == 8) break;  // (the walk ends)
      wx = centre_x(c, static_cast<unsigned>(cj));
      wy = centre_y(c, static_cast<unsigned>(ci));
      wth = move_heading(k);
      out[3 * static_cast<size_t>(written)] = wx;
      out[3 * static_cast<size_t>(written) + 1] = wy;
      out[3 * static_cast<size_t>(written) + 2] = wth;
      ++written;
      ++moves;
    }
  }
  for (; written < n_steps; ++written) {
    out[3 * static_cast<size_t>(written)] = wx;
    out[3 * static_cast<size_t>(written) + 1] = wy;
    out[3 * static_cast<size_t>(written) + 2] = wth;
  }
  if (len != nullptr) len[q] = moves;
}

// the value grid of eea_set_target_reachable: candidate_values (gain_tile.hpp) with "and geo >= 0"
template <typename R, typename Cell>
__global__ __launch_bounds__(kBlock) void reachable_values_kernel(const int8_t* __restrict__ known, const Cell* __restrict__ field,
                                                                 const int* __restrict__ geo, unsigned xsize, unsigned ysize,
                                                                 unsigned stride, int cutoff, double floor, R* __restrict__ out)
{
  candidate_values<R, Cell, true>(known, field, geo, xsize, ysize, stride, cutoff, floor, out);
}
}  // namespace

size_t geodesic_ws_bytes(unsigned xsize, unsigned ysize) { return tile_workspace_bytes(xsize, ysize); }

hipError_t launch_geodesic_begin(const CollisionParams& c, const GeodesicArgs& a, const int8_t* d_grid, const int* d_sq,
                                 const double* d_pose, const int* d_cells, int* d_geo, void* d_ws, unsigned* d_state, hipStream_t s)
{
  const GeodesicWs w = tile_workspace(c.xsize, c.ysize, d_ws);
  const unsigned blocks = cell_pass_blocks(static_cast<size_t>(c.xsize) * c.ysize);
  hipLaunchKernelGGL(geodesic_init_kernel, dim3(blocks), dim3(kBlock), 0, s, c, w, a, d_grid, d_sq, d_geo, d_state);
  const size_t n_src = static_cast<size_t>(a.P) + a.n_cells;
  if (n_src != 0) {
    hipLaunchKernelGGL(geodesic_seed_kernel, dim3(static_cast<unsigned>((n_src - 1) / kBlock + 1)), dim3(kBlock), 0, s, c, a, d_grid,
                       d_pose, d_cells, d_geo, d_state);
  }
  return hipGetLastError();
}

hipError_t launch_geodesic_rounds(const CollisionParams& c, unsigned first, unsigned count, int* d_geo, void* d_ws, unsigned* d_state,
                                  hipStream_t s)
{
  const GeodesicWs w = tile_workspace(c.xsize, c.ysize, d_ws);
  for (unsigned r = first; r < first + count; ++r) {
    hipLaunchKernelGGL(geodesic_round_kernel, dim3(w.tiles_x * w.tiles_y), dim3(kBlock), 0, s, w, c.xsize, c.ysize, r,
                       reinterpret_cast<unsigned*>(d_geo), d_state);
  }
  hipLaunchKernelGGL(geodesic_close_kernel, dim3(1), dim3(64), 0, s, w, first + count - 1u, d_state);
  return hipGetLastError();
}

hipError_t launch_geodesic_path(const CollisionParams& c, const int* d_geo, const double* d_pose, unsigned P, unsigned n_steps,
                                double* d_path, int* d_len, hipStream_t s)
{
  hipLaunchKernelGGL(geodesic_path_kernel, dim3((P - 1u) / kBlock + 1u), dim3(kBlock), 0, s, c, d_geo, d_pose, P, n_steps, d_path,
                     d_len);
  return hipGetLastError();
}

template <typename R>
hipError_t launch_reachable_values(const CollisionParams& c, int kind, const void* d_field, unsigned stride, const int8_t* d_known,
                                   const int* d_geo, double floor, R* d_values, hipStream_t s)
{
  const int cutoff = blocking_cutoff(c.occupied_threshold);
  if (kind == 0) {
    hipLaunchKernelGGL((reachable_values_kernel<R, unsigned>), values_grid(c), dim3(kBlock), 0, s, d_known,
                       static_cast<const unsigned*>(d_field), d_geo, c.xsize, c.ysize, stride, cutoff, floor, d_values);
  } else {
    hipLaunchKernelGGL((reachable_values_kernel<R, double>), values_grid(c), dim3(kBlock), 0, s, d_known,
                       static_cast<const double*>(d_field), d_geo, c.xsize, c.ysize, stride, cutoff, floor, d_values);
  }
  return hipGetLastError();
}
template hipError_t launch_reachable_values<double>(const CollisionParams&, int, const void*, unsigned, const int8_t*, const int*, double,
                                                    double*, hipStream_t);
template hipError_t launch_reachable_values<float>(const CollisionParams&, int, const void*, unsigned, const int8_t*, const int*, double,
                                                   float*, hipStream_t);
}  // namespace eea
