// Geodesic field of a grid (include/ergodic_amd.h, eea_geodesic_field / eea_geodesic_path_batch / eea_set_target_reachable):
// the cost of the cheapest 5-7 chamfer move sequence through traversable cells from a set of source cells to every cell, -1
// where there is none; the descent of that field from a pose; and the value grid of a target restricted to reachable cells.
// Integers only; the field is the unique fixed point of "no cell can be lowered", so it does not depend on the schedule.
//
//  - begin (two launches): one pass writes the traversability byte of every cell into the workspace -- bit 0: a move may enter
//    the cell; the plane is what the rounds read, so grid, d_sq and the flags are looked at once --, fills the field with -1,
//    marks every tile pending in flag plane 0 and clears plane 1 and the round words; a second launch, one lane per source,
//    stores 0 into the accepted sources' cells and counts them.
//  - a round is one launch, one workgroup of 256 threads per tile of 32 x 32 cells.  A workgroup whose flag in the round's
//    plane is 0 exits at once.  A pending one clears its flag, stages its tile of the field and of the plane with a one-cell
//    halo in LDS (an off-grid halo cell: no value, not traversable) and relaxes in place -- every thread lowers its four cells
//    to the least of neighbour + 5 (axis) / neighbour + 7 (diagonal, both passed-between cells traversable) -- until a sweep
//    changes nothing (one workgroup-wide OR per sweep).  In-place means a thread may read a neighbour's value of this sweep or
//    of the last: both are costs of real move sequences, and the loop ends only at the tile's fixed point for its halo.
//    Cells that went down are stored; for each of the eight neighbouring tiles whose halo holds one of them the workgroup
//    stores 1 into that tile's flag of the OTHER plane (idempotent) and ORs 1 into the word "something is pending for round
//    r + 1"; a workgroup that lowered anything ORs 1 into "round r changed something".
//  - the halo is read with plain loads while the neighbour may be storing: a lane sees an older or a newer value of a cell,
//    each the cost of a real move sequence, and the neighbour's mark makes this tile run again behind the next kernel boundary,
//    where it sees the final ones.  Kernel boundaries are the only synchronisation between workgroups; nothing waits.
//  - the round words rotate over three slots so that a word is cleared in a launch that neither reads nor sets it: round r
//    sets pend[(r + 1) % 3] and chg[r % 3]; its first workgroup adds chg[(r - 1) % 3] to d_state[1] and clears it and
//    pend[(r - 1) % 3].  A closing one-lane launch does the same for the last round and writes d_state[0] from pend.
//  - the path: one lane per pose walks down the field, serially; headings come from a table of eight literals.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/ergodic_amd.h"
#include "common.hpp"
#include "grid_cell.hpp"  // world_to_grid (grid.cpp:143-159), occupied

namespace eea
{
static_assert(kGeodesicTileX == EEA_GEODESIC_TILE_X && kGeodesicTileY == EEA_GEODESIC_TILE_Y, "the header publishes the tile");

namespace
{
constexpr unsigned kInf = 0xffffffffu;  // -1 as the field stores it: no move sequence known
constexpr int kTX = static_cast<int>(kGeodesicTileX), kTY = static_cast<int>(kGeodesicTileY);
constexpr int kPitch = kTX + 2;                      // a staged row: the tile and its halo
constexpr int kPerThread = kTX * kTY / kBlock;       // cells of a tile per thread
constexpr int kRowStep = kBlock / kTX;               // rows between a thread's cells
static_assert(kBlock % kTX == 0 && (kTX * kTY) % kBlock == 0, "a thread owns whole cells of one column");

// the workspace: the traversability plane, then (4-byte aligned) two planes of tile flags and the round words
struct GeodesicWs
{
  unsigned char* trav;  // [ysize][xsize]
  unsigned* flags;      // [2][tiles]
  unsigned* pend;       // [3]
  unsigned* chg;        // [3]
  unsigned tiles_x, tiles_y;
};
__host__ __device__ inline size_t trav_bytes(unsigned xsize, unsigned ysize)
{
  return (static_cast<size_t>(xsize) * ysize + 255u) / 256u * 256u;
}
inline GeodesicWs workspace(const CollisionParams& c, void* d_ws)
{
  GeodesicWs w;
  w.tiles_x = (c.xsize - 1u) / kGeodesicTileX + 1u;
  w.tiles_y = (c.ysize - 1u) / kGeodesicTileY + 1u;
  w.trav = static_cast<unsigned char*>(d_ws);
  w.flags = reinterpret_cast<unsigned*>(w.trav + trav_bytes(c.xsize, c.ysize));
  w.pend = w.flags + 2u * static_cast<size_t>(w.tiles_x) * w.tiles_y;
  w.chg = w.pend + 3;
  return w;
}

__global__ __launch_bounds__(kBlock) void geodesic_init_kernel(const CollisionParams c, const GeodesicWs w, const GeodesicArgs a,
                                                              const int8_t* __restrict__ grid, const int* __restrict__ sq,
                                                              int* __restrict__ geo, unsigned* __restrict__ state)
{
  const size_t cells = static_cast<size_t>(c.xsize) * c.ysize, tiles = static_cast<size_t>(w.tiles_x) * w.tiles_y;
  const size_t n = static_cast<size_t>(gridDim.x) * kBlock, t0 = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  for (size_t g = t0; g < cells; g += n) {
    const int8_t v = grid[g];
    bool ok = !occupied(c, v) && !(a.unknown_blocks && v < 0);
    if (ok && sq != nullptr) {
      const int d = sq[g];
      ok = d == -1 || d > a.clear_sq;
    }
    w.trav[g] = ok ? 1 : 0;
    if (!a.keep_field) geo[g] = -1;
  }
  for (size_t t = t0; t < 2 * tiles; t += n) w.flags[t] = t < tiles ? 1u : 0u;
  if (t0 < 3) {
    w.pend[t0] = 0u;
    w.chg[t0] = 0u;
  }
  if (t0 < 4) state[t0] = 0u;
}

// one lane per source: the poses first, then the cells
__global__ __launch_bounds__(kBlock) void geodesic_seed_kernel(const CollisionParams c, const GeodesicArgs a,
                                                              const int8_t* __restrict__ grid, const double* __restrict__ pose,
                                                              const int* __restrict__ src, int* __restrict__ geo,
                                                              unsigned* __restrict__ state)
{
  const size_t q = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (q >= static_cast<size_t>(a.P) + a.n_cells) return;
  size_t at;
  if (q < a.P) {
    unsigned j, i;
    world_to_grid(c, pose[3 * q], pose[3 * q + 1], j, i);
    if (!((i <= c.ysize - 1u) && (j <= c.xsize - 1u))) return;  // gridBounds (grid.cpp:96-100)
    at = static_cast<size_t>(i) * c.xsize + j;
  } else {
    const int k = src[q - a.P];
    if (k < 0 || static_cast<size_t>(k) >= static_cast<size_t>(c.xsize) * c.ysize) return;
    at = static_cast<size_t>(k);
  }
  if (occupied(c, grid[at])) return;
  geo[at] = 0;  // (every writer of this launch stores 0)
  atomicAdd(&state[2], 1u);
}

// what block 0 does at the start of round r (and the closing launch for the round after the last): the words of round r - 1
__device__ __forceinline__ void tally(const GeodesicWs& w, unsigned* state, unsigned r)
{
  if (r == 0u) return;
  const unsigned prev = (r - 1u) % 3u;
  state[1] += w.chg[prev];
  w.chg[prev] = 0u;
  w.pend[prev] = 0u;
}

__global__ __launch_bounds__(kBlock) void geodesic_round_kernel(const GeodesicWs w, unsigned xsize, unsigned ysize, unsigned r,
                                                               unsigned* geo, unsigned* state)
{
  __shared__ unsigned s_geo[(kTY + 2) * kPitch];
  __shared__ unsigned char s_trav[(kTY + 2) * kPitch];
  __shared__ unsigned s_mark;
  const int tid = threadIdx.x;
  const unsigned tile = blockIdx.x, tiles = w.tiles_x * w.tiles_y;
  if (tile == 0u && tid == 0) tally(w, state, r);
  unsigned* const mine = w.flags + static_cast<size_t>(r & 1u) * tiles;
  unsigned* const next = w.flags + static_cast<size_t>((r + 1u) & 1u) * tiles;
  if (mine[tile] == 0u) return;  // (uniform: every thread reads the same word)
  __syncthreads();               // every thread has read the flag
  if (tid == 0) mine[tile] = 0u;
  if (tid == 0) s_mark = 0u;
  const int tx = static_cast<int>(tile % w.tiles_x), ty = static_cast<int>(tile / w.tiles_x);
  const long long x0 = static_cast<long long>(tx) * kTX - 1, y0 = static_cast<long long>(ty) * kTY - 1;
  for (int k = tid; k < (kTY + 2) * kPitch; k += kBlock) {
    const long long gy = y0 + k / kPitch, gx = x0 + k % kPitch;
    unsigned v = kInf;
    unsigned char t = 0;
    if (gy >= 0 && gy < static_cast<long long>(ysize) && gx >= 0 && gx < static_cast<long long>(xsize)) {
      const size_t g = static_cast<size_t>(gy) * xsize + static_cast<size_t>(gx);
      v = geo[g];
      t = w.trav[g];
    }
    s_geo[k] = v;
    s_trav[k] = t;
  }
  __syncthreads();
  // this thread's cells: column tid % kTX, rows tid / kTX + m kRowStep
  const int col = tid % kTX, row0 = tid / kTX;
  unsigned before[kPerThread];
  bool open[kPerThread];  // a move may enter the cell
#pragma unroll
  for (int m = 0; m < kPerThread; ++m) {
    const int at = (row0 + m * kRowStep + 1) * kPitch + col + 1;
    before[m] = s_geo[at];
    open[m] = s_trav[at] != 0;
  }
  bool any = false;
  for (;;) {
    int changed = 0;
#pragma unroll
    for (int m = 0; m < kPerThread; ++m) {
      if (!open[m]) continue;
      const int at = (row0 + m * kRowStep + 1) * kPitch + col + 1;
      const unsigned e = s_geo[at + 1], n = s_geo[at + kPitch], west = s_geo[at - 1], s = s_geo[at - kPitch];
      const bool te = s_trav[at + 1] != 0, tn = s_trav[at + kPitch] != 0, tw = s_trav[at - 1] != 0, ts = s_trav[at - kPitch] != 0;
      unsigned best = s_geo[at];
      // (kInf + 5 wraps to 4: a neighbour without a value is skipped, not added to)
      const auto take = [&](unsigned v, unsigned cost, bool ok) {
        const unsigned cand = v + cost;
        best = (ok && v != kInf && cand < best) ? cand : best;
      };
      take(e, 5u, true);
      take(n, 5u, true);
      take(west, 5u, true);
      take(s, 5u, true);
      take(s_geo[at + kPitch + 1], 7u, te && tn);
      take(s_geo[at + kPitch - 1], 7u, tw && tn);
      take(s_geo[at - kPitch - 1], 7u, tw && ts);
      take(s_geo[at - kPitch + 1], 7u, te && ts);
      if (best < s_geo[at]) {
        s_geo[at] = best;  // (the cell's only writer)
        changed = 1;
      }
    }
    if (__syncthreads_or(changed) == 0) break;
    any = true;
  }
  if (!any) return;  // (uniform)
  unsigned mark = 0u;  // bit k: neighbouring tile k of the list below reads a cell of this thread's that went down
#pragma unroll
  for (int m = 0; m < kPerThread; ++m) {
    const int row = row0 + m * kRowStep;
    const unsigned v = s_geo[(row + 1) * kPitch + col + 1];
    if (v == before[m]) continue;
    const long long gy = y0 + 1 + row, gx = x0 + 1 + col;  // (on the grid: an off-grid cell is not open)
    geo[static_cast<size_t>(gy) * xsize + static_cast<size_t>(gx)] = v;
    const unsigned up = row == 0 ? 1u : 0u, down = row == kTY - 1 ? 1u : 0u, left = col == 0 ? 1u : 0u, right = col == kTX - 1 ? 1u : 0u;
    mark |= up | down << 1 | left << 2 | right << 3 | (up & left) << 4 | (up & right) << 5 | (down & left) << 6 | (down & right) << 7;
  }
  if (mark != 0u) atomicOr(&s_mark, mark);
  __syncthreads();
  if (tid < 8 && ((s_mark >> tid) & 1u) != 0u) {
    const int dy[8] = { -1, 1, 0, 0, -1, -1, 1, 1 }, dx[8] = { 0, 0, -1, 1, -1, 1, -1, 1 };
    const int ny = ty + dy[tid], nx = tx + dx[tid];
    if (ny >= 0 && ny < static_cast<int>(w.tiles_y) && nx >= 0 && nx < static_cast<int>(w.tiles_x)) {
      next[static_cast<size_t>(ny) * w.tiles_x + nx] = 1u;
      atomicOr(&w.pend[(r + 1u) % 3u], 1u);
    }
  }
  if (tid == 8) atomicOr(&w.chg[r % 3u], 1u);
}

// behind round `last`: its words into d_state; final when nothing is pending for the round after it
__global__ void geodesic_close_kernel(const GeodesicWs w, unsigned last, unsigned* state)
{
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  // (the round after `last` would clear pend[last % 3] too: nobody reads it any more)
  tally(w, state, last + 1u);
  state[0] = w.pend[(last + 1u) % 3u] == 0u ? 1u : 0u;
  state[3] = 0u;
}

// headings of the eight moves in the order the walk tries them, (di, dj) = (0,+1) (+1,0) (0,-1) (-1,0) (+1,+1) (+1,-1) (-1,-1)
// (-1,+1): atan2(di, dj) as k pi / 4 wrapped to [-pi, pi)
__device__ __forceinline__ double move_heading(int k)
{
  switch (k) {
    case 0: return 0.0;
    case 1: return 1.5707963267948966;
    case 2: return -3.141592653589793;
    case 3: return -1.5707963267948966;
    case 4: return 0.7853981633974483;
    case 5: return 2.356194490192345;
    case 6: return -2.356194490192345;
    default: return -0.7853981633974483;
  }
}

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
    // grid2World's arithmetic (grid.cpp:161-175): the centre of the cell
    const auto centre_x = [&](unsigned jj) { return static_cast<double>(jj * c.resolution) + c.resolution / 2.0 + c.xmin; };
    const auto centre_y = [&](unsigned ii) { return static_cast<double>(ii * c.resolution) + c.resolution / 2.0 + c.ymin; };
    // until a step is written the rows hold the centre of the pose's own cell with the pose's heading
    wx = centre_x(j);
    wy = centre_y(i);
    const int xs = static_cast<int>(c.xsize), ys = static_cast<int>(c.ysize);
    int ci = static_cast<int>(i), cj = static_cast<int>(j);
    const auto at = [&](int ii, int jj) {
      return (ii >= 0 && ii < ys && jj >= 0 && jj < xs) ? geo[static_cast<size_t>(ii) * c.xsize + static_cast<size_t>(jj)] : -1;
    };
    while (here > 0 && written < n_steps) {
      int k = 0;
      for (; k < 8; ++k) {
        const int di = k < 4 ? (k == 1 ? 1 : k == 3 ? -1 : 0) : (k < 6 ? 1 : -1);
        const int dj = k < 4 ? (k == 0 ? 1 : k == 2 ? -1 : 0) : ((k == 4 || k == 7) ? 1 : -1);
        const int g = at(ci + di, cj + dj);
        if (g < 0 || g + (k < 4 ? 5 : 7) != here) continue;
        if (k >= 4 && (at(ci + di, cj) < 0 || at(ci, cj + dj) < 0)) continue;
        ci += di;
        cj += dj;
        here = g;
        break;
      }
      if (k == 8) break;  // (a field that is not final may have no step here: the walk ends)
      wx = centre_x(static_cast<unsigned>(cj));
      wy = centre_y(static_cast<unsigned>(ci));
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

// the value grid of eea_set_target_reachable: gain_values_kernel's / mi_values_kernel's with "and geo >= 0"
template <typename R, typename Cell>
__global__ __launch_bounds__(kBlock) void reachable_values_kernel(const int8_t* __restrict__ known, const Cell* __restrict__ field,
                                                                 const int* __restrict__ geo, unsigned xsize, unsigned ysize,
                                                                 unsigned stride, int cutoff, double floor, R* __restrict__ out)
{
  const unsigned long long x = static_cast<unsigned long long>(blockIdx.x) * kBlock + threadIdx.x;
  if (x >= xsize) return;
  const bool lattice_col = static_cast<unsigned>(x) % stride == 0u;
  for (unsigned y = blockIdx.y; y < ysize; y += gridDim.y) {
    const size_t g = static_cast<size_t>(y) * xsize + x;
    const bool cand = lattice_col && y % stride == 0u && known[g] < cutoff && geo[g] >= 0;
    out[g] = cand ? static_cast<R>(static_cast<double>(field[g]) + floor) : R(0);
  }
}
}  // namespace

size_t geodesic_ws_bytes(unsigned xsize, unsigned ysize)
{
  const size_t tiles = static_cast<size_t>((xsize - 1u) / kGeodesicTileX + 1u) * ((ysize - 1u) / kGeodesicTileY + 1u);
  return trav_bytes(xsize, ysize) + sizeof(unsigned) * (2 * tiles + 6);
}

hipError_t launch_geodesic_begin(const CollisionParams& c, const GeodesicArgs& a, const int8_t* d_grid, const int* d_sq,
                                 const double* d_pose, const int* d_cells, int* d_geo, void* d_ws, unsigned* d_state, hipStream_t s)
{
  const GeodesicWs w = workspace(c, d_ws);
  const size_t cells = static_cast<size_t>(c.xsize) * c.ysize;
  const unsigned blocks = static_cast<unsigned>(cells / (4 * kBlock) < 1 ? 1 : (cells / (4 * kBlock) > 4096 ? 4096 : cells / (4 * kBlock)));
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
  const GeodesicWs w = workspace(c, d_ws);
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
  const unsigned bx = (c.xsize - 1u) / kBlock + 1u, by = c.ysize < 65535u ? c.ysize : 65535u;
  const int cutoff = blocking_cutoff(c.occupied_threshold);
  if (kind == 0) {
    hipLaunchKernelGGL((reachable_values_kernel<R, unsigned>), dim3(bx, by), dim3(kBlock), 0, s, d_known,
                       static_cast<const unsigned*>(d_field), d_geo, c.xsize, c.ysize, stride, cutoff, floor, d_values);
  } else {
    hipLaunchKernelGGL((reachable_values_kernel<R, double>), dim3(bx, by), dim3(kBlock), 0, s, d_known,
                       static_cast<const double*>(d_field), d_geo, c.xsize, c.ysize, stride, cutoff, floor, d_values);
  }
  return hipGetLastError();
}
template hipError_t launch_reachable_values<double>(const CollisionParams&, int, const void*, unsigned, const int8_t*, const int*, double,
                                                    double*, hipStream_t);
template hipError_t launch_reachable_values<float>(const CollisionParams&, int, const void*, unsigned, const int8_t*, const int*, double,
                                                   float*, hipStream_t);
}  // namespace eea
