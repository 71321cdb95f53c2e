// Geodesic partition of a grid (include/ergodic_amd.h, eea_geodesic_partition / eea_partition_goals / eea_partition_path_batch):
// the geodesic field of geodesic_kernel.hip with, per cell, the label of the source that reaches it most cheaply (the smallest
// label among those that do); per label its area and its best candidate cell under a score; and per robot the path from its own
// cell to its goal inside its own region.  Integers and fixed-order fp64 with a unique answer.
//
//  - a cell carries ONE 64-bit key, cost << 32 | label, all ones for "none", in a key plane in the workspace.  Keys are ordered
//    as unsigned integers, which is the lexicographic order of (cost, label); a move adds cost << 32 and keeps the label, which
//    is monotone, so "no cell can be lowered" has one fixed point: min over sources s of (d_s(cell), s).
//  - the build is geodesic_tile.hpp's rounds on keys (KeyCell); a source takes a 64-bit atomicMin of its label into its cell.
//  - a last launch unpacks the plane into d_geo / d_owner, after a budget has run out as well.
//  - goals: an init launch, a pass that adds the areas and takes the 64-bit atomicMax of an order-preserving key of the score
//    per label (kept in d_goal_score's own 8 bytes), a pass that takes the atomicMin of the cell index over the cells whose key
//    is that maximum, and a launch that turns keys back into doubles.  Max and min are exact and commutative.  A region is
//    contiguous, so the lanes of a wavefront mostly share one label: the lanes that hold the label of the first lane left are
//    combined in registers (areas by ballot and popcount, keys by a cross-lane max), the same label in consecutive chunks of a
//    wavefront's span is carried on, and one lane issues the atomics when the label changes.
//  - the path: one lane per robot walks down from its goal inside its own region, once to count, once to write the rows.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/ergodic_amd.h"
#include "common.hpp"
#include "geodesic_tile.hpp"

namespace eea
{
namespace
{
using u64 = KeyCell::T;
constexpr u64 kNone = KeyCell::kNone;

// the workspace: the key plane (8-byte aligned), then the field's workspace
struct PartitionWs
{
  u64* key;  // [ysize][xsize]
  GeodesicWs tile;
};
inline PartitionWs workspace(const CollisionParams& c, void* d_ws)
{
  u64* const key = static_cast<u64*>(d_ws);
  return PartitionWs{ key, tile_workspace(c.xsize, c.ysize, key + static_cast<size_t>(c.xsize) * c.ysize) };
}

__global__ __launch_bounds__(kBlock) void partition_init_kernel(const CollisionParams c, const PartitionWs w, const GeodesicArgs a,
                                                               const int8_t* __restrict__ grid, const int* __restrict__ sq,
                                                               const int* __restrict__ geo, const int* __restrict__ owner,
                                                               unsigned* __restrict__ state)
{
  const size_t cells = static_cast<size_t>(c.xsize) * c.ysize;
  const size_t n = static_cast<size_t>(gridDim.x) * kBlock, t0 = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  for (size_t g = t0; g < cells; g += n) {
    w.tile.trav[g] = traversable(c, a, grid[g], sq, g) ? 1 : 0;
    u64 k = kNone;
    if (a.keep_field) {  // the planes as they stand
      const int d = geo[g];
      if (d >= 0) k = static_cast<u64>(static_cast<unsigned>(d)) << 32 | static_cast<unsigned>(owner[g]);
    }
    KeyCell::store(&w.key[g], k);
  }
  reset_rounds(w.tile, state, t0, n);
}

// one lane per source; its label is its index
__global__ __launch_bounds__(kBlock) void partition_seed_kernel(const CollisionParams c, const PartitionWs w, const GeodesicArgs a,
                                                               const int8_t* __restrict__ grid, const double* __restrict__ pose,
                                                               const int* __restrict__ src, unsigned* __restrict__ state)
{
  const size_t q = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  size_t at;
  if (q >= static_cast<size_t>(a.P) + a.n_cells || !source_cell(c, a, grid, pose, src, q, at)) return;
  atomicMin(&w.key[at], static_cast<u64>(q));  // cost 0, this label: the smallest label accepted there stays
  atomicAdd(&state[2], 1u);
}

__global__ __launch_bounds__(kBlock) void partition_round_kernel(const PartitionWs w, unsigned xsize, unsigned ysize, unsigned r,
                                                                unsigned* state)
{
  tile_round<KeyCell>(w.tile, w.key, xsize, ysize, r, state);
}

__global__ void partition_close_kernel(const PartitionWs w, unsigned last, unsigned* state) { close_rounds(w.tile, last, state); }

// the key plane into the two output planes: every element of both is written
__global__ __launch_bounds__(kBlock) void partition_unpack_kernel(const u64* __restrict__ key, size_t cells, int* __restrict__ geo,
                                                                 int* __restrict__ owner)
{
  const size_t n = static_cast<size_t>(gridDim.x) * kBlock;
  for (size_t g = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x; g < cells; g += n) {
    const u64 k = key[g];
    geo[g] = k == kNone ? -1 : static_cast<int>(k >> 32);
    owner[g] = k == kNone ? -1 : static_cast<int>(k & 0xffffffffull);
  }
}

// ---- goals ------------------------------------------------------------------------------------------------------------------
// a double as an unsigned integer of the same order (no NaN reaches it); above 0 for every double, so 0 is "no candidate"
__device__ __forceinline__ u64 score_key(double s)
{
  const u64 b = static_cast<u64>(__double_as_longlong(s));
  return (b >> 63) != 0ull ? ~b : b | (1ull << 63);
}
__device__ __forceinline__ double key_score(u64 k)
{
  return __longlong_as_double(static_cast<long long>((k >> 63) != 0ull ? k & ~(1ull << 63) : ~k));
}

constexpr int kGoalNone = 0x7fffffff;  // d_goal_cell during the call: no cell yet (a cell index stays below 2^26)
constexpr unsigned kGoalChunks = 8;    // consecutive chunks of 64 cells a wavefront walks, carrying a label from one to the next

__global__ __launch_bounds__(kBlock) void goals_init_kernel(unsigned n_labels, int* __restrict__ goal_cell, u64* __restrict__ goal_key,
                                                           unsigned* __restrict__ area)
{
  const size_t r = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (r >= n_labels) return;
  goal_cell[r] = kGoalNone;
  goal_key[r] = 0ull;
  area[r] = 0u;
}

struct GoalArgs
{
  unsigned xsize, stride, n_labels;
  int cutoff;
  double w_field, w_cost;
};

// the key of a cell's score if it is a candidate of its label, else 0
template <typename Cell>
__device__ __forceinline__ u64 candidate_key(const GoalArgs& a, size_t g, int known, Cell f, int geo)
{
  const unsigned x = static_cast<unsigned>(g % a.xsize), y = static_cast<unsigned>(g / a.xsize);
  if (x % a.stride != 0u || y % a.stride != 0u || !(known < a.cutoff) || !(f > Cell(0))) return 0ull;
  const double gain = a.w_field * static_cast<double>(f), cost = a.w_cost * static_cast<double>(geo);
  return score_key(gain - cost);
}

// PASS 0: areas and the greatest score key per label; PASS 1: the lowest cell index among the cells that hold it.  Every lane of
// a wavefront stays in the loops (the cross-lane steps need them all); a lane past the grid holds no label.
template <typename Cell, int PASS>
__global__ __launch_bounds__(kBlock) void goals_pass_kernel(const GoalArgs a, size_t cells, const int8_t* __restrict__ known,
                                                           const Cell* __restrict__ field, const int* __restrict__ geo,
                                                           const int* __restrict__ owner, int* goal_cell, u64* goal_key,
                                                           unsigned* area)
{
  const unsigned lane = threadIdx.x % kWave;
  const size_t wave = (static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x) / kWave;
  const size_t first = wave * (kGoalChunks * kWave);
  // what the wavefront carries (uniform): a label, and for it PASS 0 the area and the greatest key / PASS 1 the lowest cell
  int run_label = -1;
  unsigned run_area = 0u;
  u64 run_key = 0ull;
  int run_cell = kGoalNone;
  const auto flush = [&]() {
    if (run_label < 0 || lane != 0u) return;
    if (PASS == 0) {
      atomicAdd(&area[run_label], run_area);
      if (run_key != 0ull) atomicMax(&goal_key[run_label], run_key);
    } else if (run_cell != kGoalNone) {
      atomicMin(&goal_cell[run_label], run_cell);
    }
  };
  // the span's four planes first, every load independent of every other: 4 x kGoalChunks loads in flight per lane (a load that
  // waits for the owner, then for the known cell, then for the field makes the pass wait for memory three times per chunk)
  int own_[kGoalChunks], known_[kGoalChunks], geo_[kGoalChunks];
  Cell field_[kGoalChunks];
#pragma unroll
  for (unsigned ch = 0; ch < kGoalChunks; ++ch) {
    const size_t g = first + static_cast<size_t>(ch) * kWave + lane;
    const bool in = g < cells;
    own_[ch] = in ? owner[g] : -1;
    known_[ch] = in ? static_cast<int>(known[g]) : 127;
    field_[ch] = in ? field[g] : Cell(0);
    geo_[ch] = in ? geo[g] : 0;
  }
#pragma unroll
  for (unsigned ch = 0; ch < kGoalChunks; ++ch) {
    const size_t base = first + static_cast<size_t>(ch) * kWave;
    if (base >= cells) break;  // (uniform)
    const size_t g = base + lane;
    int lab = -1;
    u64 key = 0ull;
    {
      const int o = own_[ch];
      if (o >= 0 && static_cast<unsigned>(o) < a.n_labels) {
        lab = o;
        key = candidate_key<Cell>(a, g, known_[ch], field_[ch], geo_[ch]);
        // PASS 1: only a cell that holds its label's greatest key is left (the pass before has ended: a plain load)
        if (PASS == 1 && key != 0ull && key != goal_key[o]) key = 0ull;
      }
    }
    u64 left = __ballot(lab >= 0);
    while (left != 0ull) {  // (uniform: one turn per distinct label of the chunk)
      const int lead = __ffsll(static_cast<long long>(left)) - 1;
      const int l = __builtin_amdgcn_readlane(lab, lead);
      const bool mine = lab == l;
      const u64 group = __ballot(mine);
      left &= ~group;
      const u64 with_key = __ballot(mine && key != 0ull);
      if (l != run_label) {
        flush();
        run_label = l;
        run_area = 0u;
        run_key = 0ull;
        run_cell = kGoalNone;
      }
      if (PASS == 0) {
        run_area += static_cast<unsigned>(__popcll(group));
        if (with_key != 0ull) {
          u64 k = mine ? key : 0ull;
#pragma unroll
          for (int m = kWave / 2; m >= 1; m >>= 1) {
            const u64 other = __shfl_xor(k, m, kWave);
            k = other > k ? other : k;
          }
          const unsigned lo = __builtin_amdgcn_readfirstlane(static_cast<unsigned>(k));
          const unsigned hi = __builtin_amdgcn_readfirstlane(static_cast<unsigned>(k >> 32));
          const u64 top = static_cast<u64>(hi) << 32 | lo;
          run_key = top > run_key ? top : run_key;
        }
      } else if (with_key != 0ull && run_cell == kGoalNone) {
        // cells rise with the lane and with the chunk: the first one found is the lowest of this wavefront's
        run_cell = static_cast<int>(base) + (__ffsll(static_cast<long long>(with_key)) - 1);
      }
    }
  }
  flush();
}

__global__ __launch_bounds__(kBlock) void goals_finish_kernel(unsigned n_labels, int* __restrict__ goal_cell, u64* __restrict__ goal_key)
{
  const size_t r = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (r >= n_labels) return;
  const u64 k = goal_key[r];
  if (k == 0ull) {
    goal_cell[r] = -1;
    reinterpret_cast<double*>(goal_key)[r] = 0.0;
  } else {
    reinterpret_cast<double*>(goal_key)[r] = key_score(k);
  }
}

// ---- the path ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void partition_path_kernel(const CollisionParams c, const int* __restrict__ geo,
                                                               const int* __restrict__ owner, const double* __restrict__ pose,
                                                               unsigned P, const int* __restrict__ goal_cell, unsigned n_steps,
                                                               double* __restrict__ path, int* __restrict__ len)
{
  const size_t q = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (q >= P) return;
  double wx = pose[3 * q], wy = pose[3 * q + 1], wth = pose[3 * q + 2];
  double* const out = path + q * n_steps * 3;
  const int xs = static_cast<int>(c.xsize);
  const size_t cells = static_cast<size_t>(c.xsize) * c.ysize;
  unsigned j, i;
  world_to_grid(c, wx, wy, j, i);
  const bool in_grid = (i <= c.ysize - 1u) && (j <= c.xsize - 1u);  // gridBounds (grid.cpp:96-100)
  const int goal = goal_cell[q];
  const int label = static_cast<int>(q);
  int moves = -1;  // m: the moves from the robot's cell to the goal
  const bool walk = in_grid && goal >= 0 && static_cast<size_t>(goal) < cells && owner[goal] == label && geo[goal] >= 0;
  if (walk) {
    int ci = goal / xs, cj = goal % xs, here = geo[goal];
    moves = 0;
    while (here > 0) {
      if (descend<true>(c, geo, owner, label, ci, cj, here) == 8) break;  // (a step inside the region)
      ++moves;
    }
    // (in a final field the walk ends on the robot's own cell; one that does not is refused like a goal of another region)
    if (here != 0 || ci != static_cast<int>(i) || cj != static_cast<int>(j)) moves = -1;
  }
  if (moves >= 0) {
    // before any way-point the rows hold the centre of the robot's own cell with the pose's heading
    wx = centre_x(c, j);
    wy = centre_y(c, i);
    int ci = goal / xs, cj = goal % xs, here = geo[goal];
    for (int t = 0; t < moves; ++t) {
      // the descent's move t leaves c_{m - t}: way-point m - t - 1 is that cell's centre with the heading of the move INTO it
      const double px = centre_x(c, static_cast<unsigned>(cj)), py = centre_y(c, static_cast<unsigned>(ci));
      const int k = descend<true>(c, geo, owner, label, ci, cj, here);
      const double pth = move_heading((k & 4) | ((k + 2) & 3));  // the opposite move: 0 <-> 2, 1 <-> 3, 4 <-> 6, 5 <-> 7
      const unsigned row = static_cast<unsigned>(moves - t - 1);
      if (t == 0) {  // the goal: the last way-point, and what the rows past the end repeat
        wx = px;
        wy = py;
        wth = pth;
      }
      if (row < n_steps) {
        out[3 * static_cast<size_t>(row)] = px;
        out[3 * static_cast<size_t>(row) + 1] = py;
        out[3 * static_cast<size_t>(row) + 2] = pth;
      }
    }
  }
  for (unsigned t = moves < 0 ? 0u : static_cast<unsigned>(moves); t < n_steps; ++t) {
    out[3 * static_cast<size_t>(t)] = wx;
    out[3 * static_cast<size_t>(t) + 1] = wy;
    out[3 * static_cast<size_t>(t) + 2] = wth;
  }
  if (len != nullptr) len[q] = moves < 0 ? -1 : (static_cast<unsigned>(moves) < n_steps ? moves : static_cast<int>(n_steps));
}
}  // namespace

size_t partition_ws_bytes(unsigned xsize, unsigned ysize)
{
  return sizeof(u64) * static_cast<size_t>(xsize) * ysize + tile_workspace_bytes(xsize, ysize);
}

hipError_t launch_partition_begin(const CollisionParams& c, const GeodesicArgs& a, const int8_t* d_grid, const int* d_sq,
                                  const double* d_pose, const int* d_cells, const int* d_geo, const int* d_owner, void* d_ws,
                                  unsigned* d_state, hipStream_t s)
{
  const PartitionWs w = workspace(c, d_ws);
  const unsigned blocks = cell_pass_blocks(static_cast<size_t>(c.xsize) * c.ysize);
  hipLaunchKernelGGL(partition_init_kernel, dim3(blocks), dim3(kBlock), 0, s, c, w, a, d_grid, d_sq, d_geo, d_owner, d_state);
  const size_t n_src = static_cast<size_t>(a.P) + a.n_cells;
  if (n_src != 0) {
    hipLaunchKernelGGL(partition_seed_kernel, dim3(static_cast<unsigned>((n_src - 1) / kBlock + 1)), dim3(kBlock), 0, s, c, w, a, d_grid,
                       d_pose, d_cells, d_state);
  }
  return hipGetLastError();
}

hipError_t launch_partition_rounds(const CollisionParams& c, unsigned first, unsigned count, int* d_geo, int* d_owner, void* d_ws,
                                   unsigned* d_state, hipStream_t s)
{
  const PartitionWs w = workspace(c, d_ws);
  for (unsigned r = first; r < first + count; ++r) {
    hipLaunchKernelGGL(partition_round_kernel, dim3(w.tile.tiles_x * w.tile.tiles_y), dim3(kBlock), 0, s, w, c.xsize, c.ysize, r,
                       d_state);
  }
  hipLaunchKernelGGL(partition_close_kernel, dim3(1), dim3(64), 0, s, w, first + count - 1u, d_state);
  const size_t cells = static_cast<size_t>(c.xsize) * c.ysize;
  hipLaunchKernelGGL(partition_unpack_kernel, dim3(cell_pass_blocks(cells)), dim3(kBlock), 0, s, w.key, cells, d_geo, d_owner);
  return hipGetLastError();
}

hipError_t launch_partition_goals(const CollisionParams& c, int kind, const void* d_field, unsigned stride, const int8_t* d_known,
                                  const int* d_geo, const int* d_owner, unsigned n_labels, double w_field, double w_cost,
                                  int* d_goal_cell, double* d_goal_score, unsigned* d_area, hipStream_t s)
{
  const size_t cells = static_cast<size_t>(c.xsize) * c.ysize;
  const GoalArgs a{ c.xsize, stride, n_labels, blocking_cutoff(c.occupied_threshold), w_field, w_cost };
  u64* const d_key = reinterpret_cast<u64*>(d_goal_score);
  const unsigned lb = (n_labels - 1u) / kBlock + 1u;
  constexpr size_t per_block = static_cast<size_t>(kBlock) * kGoalChunks;
  const unsigned cb = static_cast<unsigned>((cells - 1) / per_block + 1);
  hipLaunchKernelGGL(goals_init_kernel, dim3(lb), dim3(kBlock), 0, s, n_labels, d_goal_cell, d_key, d_area);
  if (kind == 0) {
    const unsigned* const f = static_cast<const unsigned*>(d_field);
    hipLaunchKernelGGL((goals_pass_kernel<unsigned, 0>), dim3(cb), dim3(kBlock), 0, s, a, cells, d_known, f, d_geo, d_owner, d_goal_cell, d_key, d_area);
    hipLaunchKernelGGL((goals_pass_kernel<unsigned, 1>), dim3(cb), dim3(kBlock), 0, s, a, cells, d_known, f, d_geo, d_owner, d_goal_cell, d_key, d_area);
  } else {
    const double* const f = static_cast<const double*>(d_field);
    hipLaunchKernelGGL((goals_pass_kernel<double, 0>), dim3(cb), dim3(kBlock), 0, s, a, cells, d_known, f, d_geo, d_owner, d_goal_cell, d_key, d_area);
    hipLaunchKernelGGL((goals_pass_kernel<double, 1>), dim3(cb), dim3(kBlock), 0, s, a, cells, d_known, f, d_geo, d_owner, d_goal_cell, d_key, d_area);
  }
  hipLaunchKernelGGL(goals_finish_kernel, dim3(lb), dim3(kBlock), 0, s, n_labels, d_goal_cell, d_key);
  return hipGetLastError();
}

hipError_t launch_partition_path(const CollisionParams& c, const int* d_geo, const int* d_owner, const double* d_pose, unsigned P,
                                 const int* d_goal_cell, unsigned n_steps, double* d_path, int* d_len, hipStream_t s)
{
  hipLaunchKernelGGL(partition_path_kernel, dim3((P - 1u) / kBlock + 1u), dim3(kBlock), 0, s, c, d_geo, d_owner, d_pose, P, d_goal_cell,
                     n_steps, d_path, d_len);
  return hipGetLastError();
}
}  // namespace eea
