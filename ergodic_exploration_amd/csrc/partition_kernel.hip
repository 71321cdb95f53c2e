// Geodesic partition of a grid (include/ergodic_amd.h, eea_geodesic_partition / eea_partition_goals / eea_partition_path_batch):
// the geodesic field of geodesic_kernel.hip with, per cell, the label of the source that reaches it most cheaply (the smallest
// label among those that do); per label its area and its best candidate cell under a score; and per robot the path from its own
// cell to its goal inside its own region.  Integers and fixed-order fp64 with a unique answer.
//
//  - a cell carries ONE 64-bit key, cost << 32 | label, all ones for "none", in a key plane in the workspace.  Keys are ordered
//    as unsigned integers, which is the lexicographic order of (cost, label); a move adds cost << 32 and keeps the label, which
//    is monotone, so "no cell can be lowered" has one fixed point: min over sources s of (d_s(cell), s).
//  - the schedule is geodesic_kernel.hip's, on keys: begin (the traversability plane, the key plane, the tile flags and round
//    words; then one lane per source, a 64-bit atomicMin of its label into its cell), one launch per round with a workgroup per
//    tile of 32 x 32 cells relaxed in LDS to its own fixed point, two flag planes, three rotating round words, a closing launch.
//    Kernel boundaries are the only synchronisation between workgroups; nothing waits.
//  - the halo is read while the neighbour may be storing.  A reader must never pair a new cost with an old label: that key would
//    be lower than any real one and, since keys only go down, would stick.  So a key is one aligned 8-byte word, every load of
//    the plane in a round and every store to it is a relaxed agent-scope 64-bit atomic, and in LDS a key is read and written
//    whole.  A reader then sees an older or a newer key of the cell, each the cost and label of a real move sequence, and the
//    neighbour's mark makes the tile run again behind the next kernel boundary.
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
#include "grid_cell.hpp"  // world_to_grid (grid.cpp:143-159), occupied

namespace eea
{
namespace
{
using u64 = unsigned long long;
constexpr u64 kNone = ~0ull;  // no move sequence known
constexpr int kTX = static_cast<int>(kGeodesicTileX), kTY = static_cast<int>(kGeodesicTileY);
constexpr int kPitch = kTX + 2;                      // a staged row: the tile and its halo
constexpr int kPerThread = kTX * kTY / kBlock;       // cells of a tile per thread
constexpr int kRowStep = kBlock / kTX;               // rows between a thread's cells
static_assert(kBlock % kTX == 0 && (kTX * kTY) % kBlock == 0, "a thread owns whole cells of one column");

// the workspace: the key plane (8-byte aligned), the traversability plane, then two planes of tile flags and the round words
struct PartitionWs
{
  u64* key;             // [ysize][xsize]
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
inline PartitionWs workspace(const CollisionParams& c, void* d_ws)
{
  PartitionWs w;
  w.tiles_x = (c.xsize - 1u) / kGeodesicTileX + 1u;
  w.tiles_y = (c.ysize - 1u) / kGeodesicTileY + 1u;
  w.key = static_cast<u64*>(d_ws);
  w.trav = reinterpret_cast<unsigned char*>(w.key + static_cast<size_t>(c.xsize) * c.ysize);
  w.flags = reinterpret_cast<unsigned*>(w.trav + trav_bytes(c.xsize, c.ysize));
  w.pend = w.flags + 2u * static_cast<size_t>(w.tiles_x) * w.tiles_y;
  w.chg = w.pend + 3;
  return w;
}

__device__ __forceinline__ u64 load_key(const u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void store_key(u64* p, u64 v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ __launch_bounds__(kBlock) void partition_init_kernel(const CollisionParams c, const PartitionWs w, const GeodesicArgs a,
                                                               const int8_t* __restrict__ grid, const int* __restrict__ sq,
                                                               const int* __restrict__ geo, const int* __restrict__ owner,
                                                               unsigned* __restrict__ state)
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
    u64 k = kNone;
    if (a.keep_field) {  // the planes as they stand
      const int d = geo[g];
      if (d >= 0) k = static_cast<u64>(static_cast<unsigned>(d)) << 32 | static_cast<unsigned>(owner[g]);
    }
    store_key(&w.key[g], k);
  }
  for (size_t t = t0; t < 2 * tiles; t += n) w.flags[t] = t < tiles ? 1u : 0u;
  if (t0 < 3) {
    w.pend[t0] = 0u;
    w.chg[t0] = 0u;
  }
  if (t0 < 4) state[t0] = 0u;
}

// one lane per source: the poses first, then the cells; its label is its index
__global__ __launch_bounds__(kBlock) void partition_seed_kernel(const CollisionParams c, const PartitionWs w, const GeodesicArgs a,
                                                               const int8_t* __restrict__ grid, const double* __restrict__ pose,
                                                               const int* __restrict__ src, unsigned* __restrict__ state)
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
  atomicMin(&w.key[at], static_cast<u64>(q));  // cost 0, this label: the smallest label accepted there stays
  atomicAdd(&state[2], 1u);
}

// what block 0 does at the start of round r (and the closing launch for the round after the last): the words of round r - 1
__device__ __forceinline__ void tally(const PartitionWs& w, unsigned* state, unsigned r)
{
  if (r == 0u) return;
  const unsigned prev = (r - 1u) % 3u;
  state[1] += w.chg[prev];
  w.chg[prev] = 0u;
  w.pend[prev] = 0u;
}

__global__ __launch_bounds__(kBlock) void partition_round_kernel(const PartitionWs w, unsigned xsize, unsigned ysize, unsigned r,
                                                                unsigned* state)
{
  __shared__ __attribute__((aligned(8))) u64 s_key[(kTY + 2) * kPitch];
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
    u64 v = kNone;
    unsigned char t = 0;
    if (gy >= 0 && gy < static_cast<long long>(ysize) && gx >= 0 && gx < static_cast<long long>(xsize)) {
      const size_t g = static_cast<size_t>(gy) * xsize + static_cast<size_t>(gx);
      v = load_key(&w.key[g]);  // (the halo's cells may be stored to by their own tile in this launch: one untorn word)
      t = w.trav[g];
    }
    s_key[k] = v;
    s_trav[k] = t;
  }
  __syncthreads();
  // this thread's cells: column tid % kTX, rows tid / kTX + m kRowStep
  const int col = tid % kTX, row0 = tid / kTX;
  u64 before[kPerThread];
  bool open[kPerThread];  // a move may enter the cell
#pragma unroll
  for (int m = 0; m < kPerThread; ++m) {
    const int at = (row0 + m * kRowStep + 1) * kPitch + col + 1;
    before[m] = s_key[at];
    open[m] = s_trav[at] != 0;
  }
  bool any = false;
  for (;;) {
    int changed = 0;
#pragma unroll
    for (int m = 0; m < kPerThread; ++m) {
      if (!open[m]) continue;
      const int at = (row0 + m * kRowStep + 1) * kPitch + col + 1;
      const bool te = s_trav[at + 1] != 0, tn = s_trav[at + kPitch] != 0, tw = s_trav[at - 1] != 0, ts = s_trav[at - kPitch] != 0;
      const u64 was = s_key[at];
      u64 best = was;
      // (a neighbour without a key is skipped, not added to; a cost stays below 2^31, so the sum keeps the label's half)
      const auto take = [&](u64 v, u64 cost, bool ok) {
        const u64 cand = v + (cost << 32);
        best = (ok && v != kNone && cand < best) ? cand : best;
      };
      take(s_key[at + 1], 5u, true);
      take(s_key[at + kPitch], 5u, true);
      take(s_key[at - 1], 5u, true);
      take(s_key[at - kPitch], 5u, true);
      take(s_key[at + kPitch + 1], 7u, te && tn);
      take(s_key[at + kPitch - 1], 7u, tw && tn);
      take(s_key[at - kPitch - 1], 7u, tw && ts);
      take(s_key[at - kPitch + 1], 7u, te && ts);
      if (best < was) {
        s_key[at] = best;  // (the cell's only writer; one 8-byte LDS store)
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
    const u64 v = s_key[(row + 1) * kPitch + col + 1];
    if (v == before[m]) continue;
    const long long gy = y0 + 1 + row, gx = x0 + 1 + col;  // (on the grid: an off-grid cell is not open)
    store_key(&w.key[static_cast<size_t>(gy) * xsize + static_cast<size_t>(gx)], v);
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
__global__ void partition_close_kernel(const PartitionWs w, unsigned last, unsigned* state)
{
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  tally(w, state, last + 1u);
  state[0] = w.pend[(last + 1u) % 3u] == 0u ? 1u : 0u;
  state[3] = 0u;
}

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
// headings of the eight moves in the header's order, (di, dj) = (0,+1) (+1,0) (0,-1) (-1,0) (+1,+1) (+1,-1) (-1,-1) (-1,+1):
// geodesic_kernel.hip's literals
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

__global__ __launch_bounds__(kBlock) void partition_path_kernel(const CollisionParams c, const int* __restrict__ geo,
                                                               const int* __restrict__ owner, const double* __restrict__ pose,
                                                               unsigned P, const int* __restrict__ goal_cell, unsigned n_steps,
                                                               double* __restrict__ path, int* __restrict__ len)
{
  const size_t q = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (q >= P) return;
  double wx = pose[3 * q], wy = pose[3 * q + 1], wth = pose[3 * q + 2];
  double* const out = path + q * n_steps * 3;
  const int xs = static_cast<int>(c.xsize), ys = static_cast<int>(c.ysize);
  const size_t cells = static_cast<size_t>(c.xsize) * c.ysize;
  unsigned j, i;
  world_to_grid(c, wx, wy, j, i);
  const bool in_grid = (i <= c.ysize - 1u) && (j <= c.xsize - 1u);  // gridBounds (grid.cpp:96-100)
  const int goal = goal_cell[q];
  const int label = static_cast<int>(q);
  const auto geo_at = [&](int ii, int jj) {
    return (ii >= 0 && ii < ys && jj >= 0 && jj < xs) ? geo[static_cast<size_t>(ii) * c.xsize + static_cast<size_t>(jj)] : -1;
  };
  // one step of the descent from (ci, cj) inside the region: the move index, or 8 when there is none
  const auto step = [&](int& ci, int& cj, int& here) {
    for (int k = 0; k < 8; ++k) {
      const int di = k < 4 ? (k == 1 ? 1 : k == 3 ? -1 : 0) : (k < 6 ? 1 : -1);
      const int dj = k < 4 ? (k == 0 ? 1 : k == 2 ? -1 : 0) : ((k == 4 || k == 7) ? 1 : -1);
      const int g = geo_at(ci + di, cj + dj);
      if (g < 0 || g + (k < 4 ? 5 : 7) != here) continue;
      if (owner[static_cast<size_t>(ci + di) * c.xsize + static_cast<size_t>(cj + dj)] != label) continue;
      if (k >= 4 && (geo_at(ci + di, cj) < 0 || geo_at(ci, cj + dj) < 0)) continue;
      ci += di;
      cj += dj;
      here = g;
      return k;
    }
    return 8;
  };
  int moves = -1;  // m: the moves from the robot's cell to the goal
  const bool walk = in_grid && goal >= 0 && static_cast<size_t>(goal) < cells && owner[goal] == label && geo[goal] >= 0;
  if (walk) {
    int ci = goal / xs, cj = goal % xs, here = geo[goal];
    moves = 0;
    while (here > 0) {
      if (step(ci, cj, here) == 8) break;
      ++moves;
    }
    // (in a final field the walk ends on the robot's own cell; one that does not is refused like a goal of another region)
    if (here != 0 || ci != static_cast<int>(i) || cj != static_cast<int>(j)) moves = -1;
  }
  if (moves >= 0) {
    // grid2World's arithmetic (grid.cpp:161-175): the centre of the cell
    const auto centre_x = [&](unsigned jj) { return static_cast<double>(jj * c.resolution) + c.resolution / 2.0 + c.xmin; };
    const auto centre_y = [&](unsigned ii) { return static_cast<double>(ii * c.resolution) + c.resolution / 2.0 + c.ymin; };
    // before any way-point the rows hold the centre of the robot's own cell with the pose's heading
    wx = centre_x(j);
    wy = centre_y(i);
    int ci = goal / xs, cj = goal % xs, here = geo[goal];
    for (int t = 0; t < moves; ++t) {
      // the descent's move t leaves c_{m - t}: way-point m - t - 1 is that cell's centre with the heading of the move INTO it
      const double px = centre_x(static_cast<unsigned>(cj)), py = centre_y(static_cast<unsigned>(ci));
      const int k = step(ci, cj, here);
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
  const size_t tiles = static_cast<size_t>((xsize - 1u) / kGeodesicTileX + 1u) * ((ysize - 1u) / kGeodesicTileY + 1u);
  return sizeof(u64) * static_cast<size_t>(xsize) * ysize + trav_bytes(xsize, ysize) + sizeof(unsigned) * (2 * tiles + 6);
}

hipError_t launch_partition_begin(const CollisionParams& c, const GeodesicArgs& a, const int8_t* d_grid, const int* d_sq,
                                  const double* d_pose, const int* d_cells, const int* d_geo, const int* d_owner, void* d_ws,
                                  unsigned* d_state, hipStream_t s)
{
  const PartitionWs w = workspace(c, d_ws);
  const size_t cells = static_cast<size_t>(c.xsize) * c.ysize;
  const unsigned blocks = static_cast<unsigned>(cells / (4 * kBlock) < 1 ? 1 : (cells / (4 * kBlock) > 4096 ? 4096 : cells / (4 * kBlock)));
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
    hipLaunchKernelGGL(partition_round_kernel, dim3(w.tiles_x * w.tiles_y), dim3(kBlock), 0, s, w, c.xsize, c.ysize, r, d_state);
  }
  hipLaunchKernelGGL(partition_close_kernel, dim3(1), dim3(64), 0, s, w, first + count - 1u, d_state);
  const size_t cells = static_cast<size_t>(c.xsize) * c.ysize;
  const unsigned blocks = static_cast<unsigned>(cells / (4 * kBlock) < 1 ? 1 : (cells / (4 * kBlock) > 4096 ? 4096 : cells / (4 * kBlock)));
  hipLaunchKernelGGL(partition_unpack_kernel, dim3(blocks), dim3(kBlock), 0, s, w.key, cells, d_geo, d_owner);
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
