// Frontier regions (include/ergodic_amd.h, eea_frontier_regions / eea_frontier_goals): the member cells of a grid -- frontier
// cells of an occupancy grid, or the non-zero cells of a caller's mask -- grouped into their 8-connected components, each with
// a label (its least row-major index), a rank, a record of integer statistics and an entry cell; and per robot the record it
// should go for.  Integers with a unique answer; the one fp64 expression is a score of two products and a difference.
//
// Label-equivalence union-find on tiles, in a fixed number of launches whatever the map:
//  - local: one workgroup per tile of kGeodesicTileX x kGeodesicTileY cells stages the tile's values with a one-cell halo
//    (the halo only feeds the frontier predicate), decides membership, and unites every member with its member neighbours to
//    the W, NW, N and NE inside the tile by a lock-free union in LDS.  A member then stores the global index of its local root
//    into d_root, which is the parent plane of the next two launches; everything else stores -1.  A local index rises with the
//    global one inside a tile, so parent[x] <= x holds on the plane.
//  - merge: one lane per (member on a tile border, member neighbour to its W, NW, N or NE in ANOTHER tile) runs the same union
//    on the plane:   a = find(a); b = find(b); if equal, done; let a be the larger; old = atomicMin(&parent[a], b); if old == a
//    (a was a root: it hangs under b now) done; else go on with (old, b).  find follows parents until parent[x] == x; parents
//    never rise, so it strictly descends.  old < a in the last case, so the larger of the pair strictly falls per turn: every
//    loop is bounded and none waits for another workgroup.  When the atomicMin lands on a cell that was no root any more, the
//    link it displaced (or the one that stayed) is `old`, and the next turn unites it.  Every access to the plane in this launch
//    is a relaxed agent-scope atomic load or an atomicMin: a parent read late is still a cell of the same final set, which
//    would cost turns, not the answer -- and is not relied upon.  No path compression here.
//  - flatten: behind the kernel boundary every member stores find(cell), the least index of its set.  (A find may pass through
//    a cell another lane has flattened already: it reads the old parent or the root, both in the cell's own tree.)  Members and
//    roots (root == cell) are counted per CHUNK of kChunk consecutive row-major cells: ranks ascend with the root's row-major
//    index, which chunks of the linear order keep and tiles do not.  At most 2^26 / kChunk = 65 536 counts.
//  - rank: one workgroup turns the root counts into exclusive offsets (every thread sums a contiguous share, one scan over the
//    256 sums; no look-back chain, nothing waits) and writes d_state.
//  - scatter: per chunk, a root's rank is the chunk's offset + the roots before it in the chunk (ballots per 64 cells).  The
//    root's lane writes the rank into d_region and, below max_regions, the record in its empty state; non-members get -1.
//  - stats: every other member copies its root's rank (roots are not written in this launch), and members of ranks below
//    max_regions add into their record: size, row and column sums, bounding box, and the 64-bit atomicMin of geo << 32 | cell.
//    All integer and commutative.  A region is contiguous, so the lanes of a wavefront that hold the rank of the first lane left
//    are combined in registers, the same rank in consecutive chunks of 64 cells is carried on, and one lane issues the atomics
//    when the rank changes (goals_pass_kernel's shape in partition_kernel.hip).
//  - finish: entry_owner and reserved per record; entry_cell / entry_cost = -1 without d_geo.
//  - goals: init; per record the 64-bit atomicMax of an order-preserving key of its score into its owner's slot (d_goal_score's
//    own 8 bytes); the atomicMin of the record's index among those at that key; a launch that turns keys into doubles.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/ergodic_amd.h"
#include "common.hpp"
#include "grid_cell.hpp"  // occupied

namespace eea
{
namespace
{
using u64 = unsigned long long;
using Region = eea_frontier_region;
static_assert(sizeof(Region) == 56 && offsetof(Region, entry_cell) == 16 && offsetof(Region, entry_cost) == 20,
              "entry_cost << 32 | entry_cell is one aligned 8-byte word");

constexpr int kFTX = static_cast<int>(kGeodesicTileX), kFTY = static_cast<int>(kGeodesicTileY);
constexpr int kFPitch = kFTX + 2;                    // a staged row: the tile and its halo
constexpr int kTileCells = kFTX * kFTY;
constexpr int kFPerThread = kTileCells / kBlock;     // cells of a tile per thread
constexpr unsigned kChunk = 1024;                    // consecutive row-major cells a workgroup counts / ranks
constexpr unsigned kSegs = kChunk / kWave;           // runs of 64 cells in a chunk
constexpr unsigned kStatChunks = 8;                  // consecutive runs of 64 cells a wavefront walks in the stats pass
constexpr u64 kNoEntry = ~0ull;
static_assert(kTileCells % kBlock == 0 && kChunk % kBlock == 0, "whole cells per thread");

// the workspace: per chunk its root count (an exclusive offset behind the rank launch), then per chunk its member count
struct FrontierWs
{
  unsigned* roots;
  unsigned* members;
  unsigned chunks;
};
inline unsigned chunk_count(size_t cells) { return static_cast<unsigned>((cells - 1) / kChunk + 1); }
inline FrontierWs workspace(size_t cells, void* d_ws)
{
  const unsigned chunks = chunk_count(cells);
  return FrontierWs{ static_cast<unsigned*>(d_ws), static_cast<unsigned*>(d_ws) + chunks, chunks };
}

__device__ __forceinline__ int plane_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ---- local ------------------------------------------------------------------------------------------------------------------
// the lock-free union of the header comment on `parent`: the plane (see merge), or a tile's cells in LDS, where the loads are
// relaxed workgroup-scope atomics beside an LDS atomicMin
template <bool GLOBAL>
__device__ __forceinline__ int find_root(const int* parent, int x)
{
  for (;;) {
    const int p = GLOBAL ? plane_load(&parent[x]) : __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (p == x) return x;
    x = p;
  }
}
template <bool GLOBAL>
__device__ __forceinline__ void unite(int* parent, int a, int b)
{
  for (;;) {
    a = find_root<GLOBAL>(parent, a);
    b = find_root<GLOBAL>(parent, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(&parent[a], b);
    if (old == a) return;
    a = old;  // (old < a: the larger of the pair went down)
  }
}

struct MemberArgs
{
  unsigned xsize, ysize, tiles_x;
  int kind;
  CollisionParams c;
};

__global__ __launch_bounds__(kBlock) void frontier_local_kernel(const MemberArgs a, const int8_t* __restrict__ grid,
                                                               const int* __restrict__ geo, int* __restrict__ root)
{
  __shared__ signed char s_val[(kFTY + 2) * kFPitch];
  __shared__ int s_parent[kTileCells];
  const int tid = threadIdx.x;
  const int tx = static_cast<int>(blockIdx.x % a.tiles_x), ty = static_cast<int>(blockIdx.x / a.tiles_x);
  const long long x0 = static_cast<long long>(tx) * kFTX - 1, y0 = static_cast<long long>(ty) * kFTY - 1;
  // an off-grid cell is not unknown and not a member: 0 serves both kinds
  for (int k = tid; k < (kFTY + 2) * kFPitch; k += kBlock) {
    const long long gy = y0 + k / kFPitch, gx = x0 + k % kFPitch;
    signed char v = 0;
    if (gy >= 0 && gy < static_cast<long long>(a.ysize) && gx >= 0 && gx < static_cast<long long>(a.xsize)) {
      v = grid[static_cast<size_t>(gy) * a.xsize + static_cast<size_t>(gx)];
    }
    s_val[k] = v;
  }
  __syncthreads();
  // this thread's cells: local index l = tid + m kBlock, row l / kFTX, column l % kFTX
  bool member[kFPerThread];
  size_t at[kFPerThread];
#pragma unroll
  for (int m = 0; m < kFPerThread; ++m) {
    const int l = tid + m * kBlock, ly = l / kFTX, lx = l % kFTX;
    const long long gy = y0 + 1 + ly, gx = x0 + 1 + lx;
    const bool in = gy < static_cast<long long>(a.ysize) && gx < static_cast<long long>(a.xsize);
    at[m] = in ? static_cast<size_t>(gy) * a.xsize + static_cast<size_t>(gx) : 0;
    const int s = (ly + 1) * kFPitch + lx + 1;
    const signed char v = s_val[s];
    bool is;
    if (a.kind == EEA_FRONTIER_OF_MASK) {
      is = v != 0;
    } else {
      is = v >= 0 && !occupied(a.c, v) && (s_val[s + 1] < 0 || s_val[s - 1] < 0 || s_val[s + kFPitch] < 0 || s_val[s - kFPitch] < 0);
    }
    is = is && in;
    if (is && geo != nullptr) is = geo[at[m]] >= 0;
    member[m] = is;
    s_parent[l] = is ? l : -1;
  }
  __syncthreads();
#pragma unroll
  for (int m = 0; m < kFPerThread; ++m) {
    if (!member[m]) continue;
    const int l = tid + m * kBlock, ly = l / kFTX, lx = l % kFTX;
    if (lx > 0 && s_parent[l - 1] >= 0) unite<false>(s_parent, l, l - 1);
    if (ly > 0) {
      if (lx > 0 && s_parent[l - kFTX - 1] >= 0) unite<false>(s_parent, l, l - kFTX - 1);
      if (s_parent[l - kFTX] >= 0) unite<false>(s_parent, l, l - kFTX);
      if (lx < kFTX - 1 && s_parent[l - kFTX + 1] >= 0) unite<false>(s_parent, l, l - kFTX + 1);
    }
  }
  __syncthreads();
#pragma unroll
  for (int m = 0; m < kFPerThread; ++m) {
    const int l = tid + m * kBlock, ly = l / kFTX, lx = l % kFTX;
    if (!(y0 + 1 + ly < static_cast<long long>(a.ysize) && x0 + 1 + lx < static_cast<long long>(a.xsize))) continue;
    int out = -1;
    if (member[m]) {
      const int r = find_root<false>(s_parent, l);
      out = static_cast<int>((y0 + 1 + r / kFTX) * a.xsize + (x0 + 1 + r % kFTX));
    }
    root[at[m]] = out;
  }
}

// ---- merge ------------------------------------------------------------------------------------------------------------------
// the cells of a tile with a neighbour to the W, NW, N or NE in another tile: its top row, its left and its right column.  One
// lane per (such cell, direction)
constexpr int kBorderCells = kFTX + 2 * kFTY;
__global__ __launch_bounds__(kBlock) void frontier_merge_kernel(unsigned xsize, unsigned ysize, unsigned tiles_x, int* parent)
{
  const int tx = static_cast<int>(blockIdx.x % tiles_x), ty = static_cast<int>(blockIdx.x / tiles_x);
  for (int k = threadIdx.x; k < 4 * kBorderCells; k += kBlock) {
    const int cell = k / 4, dir = k % 4;
    int lx, ly;
    if (cell < kFTX) {
      lx = cell;
      ly = 0;
    } else if (cell < kFTX + kFTY) {
      lx = 0;
      ly = cell - kFTX;
    } else {
      lx = kFTX - 1;
      ly = cell - kFTX - kFTY;
    }
    if (cell >= kFTX && ly == 0) continue;                  // (the corners belong to the top row)
    const int dy = dir == 0 ? 0 : -1, dx = dir == 0 ? -1 : dir - 2;  // W, NW, N, NE
    const int nlx = lx + dx, nly = ly + dy;
    if (nlx >= 0 && nlx < kFTX && nly >= 0) continue;       // the neighbour is in this tile: the local launch united them
    const long long gy = static_cast<long long>(ty) * kFTY + ly, gx = static_cast<long long>(tx) * kFTX + lx;
    const long long ny = gy + dy, nx = gx + dx;
    if (gy >= static_cast<long long>(ysize) || gx >= static_cast<long long>(xsize)) continue;
    if (ny < 0 || nx < 0 || nx >= static_cast<long long>(xsize)) continue;
    const int here = static_cast<int>(gy * xsize + gx), there = static_cast<int>(ny * xsize + nx);
    if (plane_load(&parent[here]) < 0 || plane_load(&parent[there]) < 0) continue;
    unite<true>(parent, here, there);
  }
}

// ---- flatten and count ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void frontier_flatten_kernel(size_t cells, int* root, const FrontierWs w)
{
  __shared__ unsigned s_count[2];
  if (threadIdx.x < 2) s_count[threadIdx.x] = 0u;
  __syncthreads();
  const size_t base = static_cast<size_t>(blockIdx.x) * kChunk;
  unsigned members = 0u, roots = 0u;
#pragma unroll
  for (unsigned m = 0; m < kChunk / kBlock; ++m) {
    const size_t g = base + m * kBlock + threadIdx.x;
    if (g >= cells) continue;
    int x = root[g];
    if (x < 0) continue;
    // (a cell on the way may have been flattened by its own lane: old parent or root, both of this tree and both <= the cell)
    for (int p = root[x]; p != x; p = root[x]) x = p;
    root[g] = x;
    ++members;
    roots += static_cast<size_t>(x) == g ? 1u : 0u;
  }
  if (members != 0u) atomicAdd(&s_count[0], members);
  if (roots != 0u) atomicAdd(&s_count[1], roots);
  __syncthreads();
  if (threadIdx.x == 0) {
    w.members[blockIdx.x] = s_count[0];
    w.roots[blockIdx.x] = s_count[1];
  }
}

// ---- rank -------------------------------------------------------------------------------------------------------------------
// one workgroup: the root counts into exclusive offsets in place, and d_state
__global__ __launch_bounds__(kBlock) void frontier_rank_kernel(const FrontierWs w, unsigned max_regions, unsigned* __restrict__ state)
{
  __shared__ unsigned s_roots[kBlock], s_members[kBlock];
  const unsigned tid = threadIdx.x;
  const unsigned share = (w.chunks - 1u) / kBlock + 1u;
  const unsigned lo = tid * share < w.chunks ? tid * share : w.chunks;
  const unsigned hi = lo + share < w.chunks ? lo + share : w.chunks;
  unsigned roots = 0u, members = 0u;
  for (unsigned k = lo; k < hi; ++k) {
    roots += w.roots[k];
    members += w.members[k];
  }
  s_roots[tid] = roots;
  s_members[tid] = members;
  __syncthreads();
  unsigned before = 0u, n = 0u, total = 0u;
  for (unsigned t = 0; t < kBlock; ++t) {
    before += t < tid ? s_roots[t] : 0u;
    n += s_roots[t];
    total += s_members[t];
  }
  for (unsigned k = lo; k < hi; ++k) {
    const unsigned c = w.roots[k];
    w.roots[k] = before;
    before += c;
  }
  if (tid == 0u) {
    state[0] = n;
    state[1] = n < max_regions ? n : max_regions;
    state[2] = total;
    state[3] = 0u;
  }
}

// ---- scatter ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void frontier_scatter_kernel(size_t cells, const int* __restrict__ root, const FrontierWs w,
                                                                 unsigned max_regions, int* __restrict__ region,
                                                                 Region* __restrict__ regions)
{
  __shared__ unsigned s_seg[kSegs];
  const unsigned lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  const size_t base = static_cast<size_t>(blockIdx.x) * kChunk;
  int r_[kChunk / kBlock];
  u64 ballot_[kChunk / kBlock];
#pragma unroll
  for (unsigned m = 0; m < kChunk / kBlock; ++m) {
    const size_t g = base + m * kBlock + threadIdx.x;  // run m * (kBlock / kWave) + wave of the chunk, cell `lane` of it
    r_[m] = g < cells ? root[g] : -1;
    ballot_[m] = __ballot(r_[m] >= 0 && static_cast<size_t>(r_[m]) == g);
    if (lane == 0u) s_seg[m * (kBlock / kWave) + wave] = static_cast<unsigned>(__popcll(ballot_[m]));
  }
  __syncthreads();
  const unsigned offset = w.roots[blockIdx.x];
#pragma unroll
  for (unsigned m = 0; m < kChunk / kBlock; ++m) {
    const size_t g = base + m * kBlock + threadIdx.x;
    if (g >= cells) continue;
    const unsigned seg = m * (kBlock / kWave) + wave;
    if (r_[m] < 0) {
      region[g] = -1;
      continue;
    }
    if (static_cast<size_t>(r_[m]) != g) continue;  // (the stats launch copies its root's rank)
    unsigned rank = offset;
    for (unsigned t = 0; t < seg; ++t) rank += s_seg[t];
    rank += static_cast<unsigned>(__popcll(ballot_[m] & ((1ull << lane) - 1ull)));
    region[g] = static_cast<int>(rank);
    if (rank < max_regions) {
      Region e;
      e.sum_i = e.sum_j = 0ull;
      e.entry_cell = e.entry_cost = -1;  // (kNoEntry as two halves)
      e.root = static_cast<int>(g);
      e.size = 0u;
      e.i_min = e.j_min = 0x7fffffff;
      e.i_max = e.j_max = -1;
      e.entry_owner = -1;
      e.reserved = 0;
      regions[rank] = e;
    }
  }
}

// ---- stats ------------------------------------------------------------------------------------------------------------------
template <typename T, typename Op>
__device__ __forceinline__ T wave_reduce(T v, Op op)
{
#pragma unroll
  for (int m = kWave / 2; m >= 1; m >>= 1) v = op(v, __shfl_xor(v, m, kWave));
  return v;
}

// what a wavefront carries for one rank (uniform)
struct RunStats
{
  int label = -1;
  unsigned size = 0u;
  u64 sum_i = 0ull, sum_j = 0ull, entry = kNoEntry;
  int i_min = 0x7fffffff, i_max = -1, j_min = 0x7fffffff, j_max = -1;
};

__global__ __launch_bounds__(kBlock) void frontier_stats_kernel(size_t cells, unsigned xsize, const int* __restrict__ root,
                                                               const int* __restrict__ geo, unsigned max_regions, int* region,
                                                               Region* regions)
{
  const unsigned lane = threadIdx.x % kWave;
  const size_t wave = (static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x) / kWave;
  const size_t first = wave * (kStatChunks * kWave);
  RunStats run;
  const auto flush = [&]() {
    if (run.label < 0 || lane != 0u) return;
    Region* const e = &regions[run.label];
    atomicAdd(&e->size, run.size);
    atomicAdd(reinterpret_cast<u64*>(&e->sum_i), run.sum_i);
    atomicAdd(reinterpret_cast<u64*>(&e->sum_j), run.sum_j);
    atomicMin(&e->i_min, run.i_min);
    atomicMax(&e->i_max, run.i_max);
    atomicMin(&e->j_min, run.j_min);
    atomicMax(&e->j_max, run.j_max);
    if (run.entry != kNoEntry) atomicMin(reinterpret_cast<u64*>(&e->entry_cell), run.entry);
  };
  // the span's loads first, independent of one another; then the ranks of the roots
  int root_[kStatChunks], geo_[kStatChunks], lab_[kStatChunks];
#pragma unroll
  for (unsigned ch = 0; ch < kStatChunks; ++ch) {
    const size_t g = first + static_cast<size_t>(ch) * kWave + lane;
    const bool in = g < cells;
    root_[ch] = in ? root[g] : -1;
    geo_[ch] = in && geo != nullptr ? geo[g] : -1;
  }
#pragma unroll
  for (unsigned ch = 0; ch < kStatChunks; ++ch) lab_[ch] = root_[ch] >= 0 ? region[root_[ch]] : -1;  // (a root's: not written here)
#pragma unroll
  for (unsigned ch = 0; ch < kStatChunks; ++ch) {
    const size_t base = first + static_cast<size_t>(ch) * kWave;
    if (base >= cells) break;  // (uniform)
    const size_t g = base + lane;
    int lab = lab_[ch];
    if (lab >= 0 && static_cast<size_t>(root_[ch]) != g) region[g] = lab;
    if (lab >= 0 && static_cast<unsigned>(lab) >= max_regions) lab = -1;  // no record
    const int i = static_cast<int>(g / xsize), j = static_cast<int>(g % xsize);
    const u64 key = geo_[ch] >= 0 ? static_cast<u64>(static_cast<unsigned>(geo_[ch])) << 32 | static_cast<unsigned>(g) : kNoEntry;
    u64 left = __ballot(lab >= 0);
    while (left != 0ull) {  // (uniform: one turn per distinct rank of the run)
      const int lead = __ffsll(static_cast<long long>(left)) - 1;
      const int l = __builtin_amdgcn_readlane(lab, lead);
      const bool mine = lab == l;
      const u64 group = __ballot(mine);
      left &= ~group;
      if (l != run.label) {
        flush();
        run = RunStats{};
        run.label = l;
      }
      run.size += static_cast<unsigned>(__popcll(group));
      // (a run of 64 cells: its sums stay far inside 32 bits)
      run.sum_i += wave_reduce(mine ? static_cast<unsigned>(i) : 0u, [](unsigned x, unsigned y) { return x + y; });
      run.sum_j += wave_reduce(mine ? static_cast<unsigned>(j) : 0u, [](unsigned x, unsigned y) { return x + y; });
      const int lo_i = wave_reduce(mine ? i : 0x7fffffff, [](int x, int y) { return x < y ? x : y; });
      const int hi_i = wave_reduce(mine ? i : -1, [](int x, int y) { return x > y ? x : y; });
      const int lo_j = wave_reduce(mine ? j : 0x7fffffff, [](int x, int y) { return x < y ? x : y; });
      const int hi_j = wave_reduce(mine ? j : -1, [](int x, int y) { return x > y ? x : y; });
      const u64 k = wave_reduce(mine ? key : kNoEntry, [](u64 x, u64 y) { return x < y ? x : y; });
      run.i_min = lo_i < run.i_min ? lo_i : run.i_min;
      run.i_max = hi_i > run.i_max ? hi_i : run.i_max;
      run.j_min = lo_j < run.j_min ? lo_j : run.j_min;
      run.j_max = hi_j > run.j_max ? hi_j : run.j_max;
      run.entry = k < run.entry ? k : run.entry;
    }
  }
  flush();
}

__global__ __launch_bounds__(kBlock) void frontier_finish_kernel(const unsigned* __restrict__ state, const int* __restrict__ geo,
                                                                const int* __restrict__ owner, Region* __restrict__ regions)
{
  const unsigned n = state[1];
  const size_t step = static_cast<size_t>(gridDim.x) * kBlock;
  for (size_t r = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x; r < n; r += step) {
    Region* const e = &regions[r];
    int who = -1;
    if (geo == nullptr) {
      e->entry_cell = -1;
      e->entry_cost = -1;
    } else if (owner != nullptr && e->entry_cell >= 0) {
      who = owner[e->entry_cell];
    }
    e->entry_owner = who;
    e->reserved = 0;
  }
}

// ---- goals ------------------------------------------------------------------------------------------------------------------
// a double as an unsigned integer of the same order (no NaN reaches it); above 0 for every double, so 0 is "no record"
// (partition_kernel.hip's pair, written again here: that object's code stays as it is)
__device__ __forceinline__ u64 score_key(double s)
{
  const u64 b = static_cast<u64>(__double_as_longlong(s));
  return (b >> 63) != 0ull ? ~b : b | (1ull << 63);
}
__device__ __forceinline__ double key_score(u64 k)
{
  return __longlong_as_double(static_cast<long long>((k >> 63) != 0ull ? k & ~(1ull << 63) : ~k));
}

constexpr int kNoRegion = 0x7fffffff;

__global__ __launch_bounds__(kBlock) void frontier_goals_init_kernel(unsigned P, int* __restrict__ goal_region, u64* __restrict__ goal_key)
{
  const size_t step = static_cast<size_t>(gridDim.x) * kBlock;
  for (size_t q = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x; q < P; q += step) {
    goal_region[q] = kNoRegion;
    goal_key[q] = 0ull;
  }
}

struct FrontierGoalArgs
{
  unsigned max_regions, P, min_size;
  double w_size, w_cost;
};

// PASS 0: the greatest key per robot; PASS 1: the lowest record among those that hold it
template <int PASS>
__global__ __launch_bounds__(kBlock) void frontier_goals_pass_kernel(const FrontierGoalArgs a, const Region* __restrict__ regions,
                                                                    const unsigned* __restrict__ state, int* goal_region, u64* goal_key)
{
  const unsigned n = state[1] < a.max_regions ? state[1] : a.max_regions;
  const size_t step = static_cast<size_t>(gridDim.x) * kBlock;
  for (size_t r = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x; r < n; r += step) {
    const Region e = regions[r];
    if (e.entry_owner < 0 || static_cast<unsigned>(e.entry_owner) >= a.P || e.entry_cell < 0 || e.size < a.min_size) continue;
    const double gain = a.w_size * static_cast<double>(e.size), cost = a.w_cost * static_cast<double>(e.entry_cost);
    const u64 key = score_key(gain - cost);
    if (PASS == 0) {
      atomicMax(&goal_key[e.entry_owner], key);
    } else if (key == goal_key[e.entry_owner]) {  // (the pass before has ended: a plain load)
      atomicMin(&goal_region[e.entry_owner], static_cast<int>(r));
    }
  }
}

__global__ __launch_bounds__(kBlock) void frontier_goals_finish_kernel(unsigned P, const Region* __restrict__ regions,
                                                                      int* __restrict__ goal_cell, int* __restrict__ goal_region,
                                                                      u64* __restrict__ goal_key)
{
  const size_t step = static_cast<size_t>(gridDim.x) * kBlock;
  for (size_t q = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x; q < P; q += step) {
    const u64 k = goal_key[q];
    if (k == 0ull) {
      goal_cell[q] = -1;
      goal_region[q] = -1;
      reinterpret_cast<double*>(goal_key)[q] = 0.0;
    } else {
      goal_cell[q] = regions[goal_region[q]].entry_cell;
      reinterpret_cast<double*>(goal_key)[q] = key_score(k);
    }
  }
}

// blocks of a grid-stride pass over n items, within [1, 4096]
inline unsigned item_blocks(size_t n)
{
  const size_t b = (n + kBlock - 1) / kBlock;
  return static_cast<unsigned>(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}
}  // namespace

size_t frontier_ws_bytes(unsigned xsize, unsigned ysize)
{
  return 2 * sizeof(unsigned) * static_cast<size_t>(chunk_count(static_cast<size_t>(xsize) * ysize));
}

hipError_t launch_frontier_regions(const CollisionParams& c, int kind, const int8_t* d_grid, const int* d_geo, const int* d_owner,
                                   unsigned max_regions, int* d_root, int* d_region, eea_frontier_region* d_regions, void* d_ws,
                                   unsigned* d_state, hipStream_t s)
{
  const size_t cells = static_cast<size_t>(c.xsize) * c.ysize;
  const FrontierWs w = workspace(cells, d_ws);
  const unsigned tiles_x = (c.xsize - 1u) / kGeodesicTileX + 1u, tiles_y = (c.ysize - 1u) / kGeodesicTileY + 1u;
  const MemberArgs a{ c.xsize, c.ysize, tiles_x, kind, c };
  hipLaunchKernelGGL(frontier_local_kernel, dim3(tiles_x * tiles_y), dim3(kBlock), 0, s, a, d_grid, d_geo, d_root);
  hipLaunchKernelGGL(frontier_merge_kernel, dim3(tiles_x * tiles_y), dim3(kBlock), 0, s, c.xsize, c.ysize, tiles_x, d_root);
  hipLaunchKernelGGL(frontier_flatten_kernel, dim3(w.chunks), dim3(kBlock), 0, s, cells, d_root, w);
  hipLaunchKernelGGL(frontier_rank_kernel, dim3(1), dim3(kBlock), 0, s, w, max_regions, d_state);
  hipLaunchKernelGGL(frontier_scatter_kernel, dim3(w.chunks), dim3(kBlock), 0, s, cells, d_root, w, max_regions, d_region, d_regions);
  constexpr size_t per_block = static_cast<size_t>(kBlock) * kStatChunks;
  hipLaunchKernelGGL(frontier_stats_kernel, dim3(static_cast<unsigned>((cells - 1) / per_block + 1)), dim3(kBlock), 0, s, cells, c.xsize,
                     d_root, d_geo, max_regions, d_region, d_regions);
  if (max_regions != 0u) {
    hipLaunchKernelGGL(frontier_finish_kernel, dim3(item_blocks(max_regions)), dim3(kBlock), 0, s, d_state, d_geo, d_owner, d_regions);
  }
  return hipGetLastError();
}

hipError_t launch_frontier_goals(const eea_frontier_region* d_regions, const unsigned* d_state, unsigned max_regions, unsigned P,
                                 unsigned min_size, double w_size, double w_cost, int* d_goal_cell, int* d_goal_region,
                                 double* d_goal_score, hipStream_t s)
{
  const FrontierGoalArgs a{ max_regions, P, min_size, w_size, w_cost };
  u64* const d_key = reinterpret_cast<u64*>(d_goal_score);
  const unsigned pb = item_blocks(P), rb = item_blocks(max_regions);
  hipLaunchKernelGGL(frontier_goals_init_kernel, dim3(pb), dim3(kBlock), 0, s, P, d_goal_region, d_key);
  hipLaunchKernelGGL((frontier_goals_pass_kernel<0>), dim3(rb), dim3(kBlock), 0, s, a, d_regions, d_state, d_goal_region, d_key);
  hipLaunchKernelGGL((frontier_goals_pass_kernel<1>), dim3(rb), dim3(kBlock), 0, s, a, d_regions, d_state, d_goal_region, d_key);
  hipLaunchKernelGGL(frontier_goals_finish_kernel, dim3(pb), dim3(kBlock), 0, s, P, d_regions, d_goal_cell, d_goal_region, d_key);
  return hipGetLastError();
}
}  // namespace eea
