// What the geodesic field (geodesic_kernel.hip) and the geodesic partition (partition_kernel.hip) share: the build of a field of
// 5-7 chamfer costs by rounds over tiles, and the one-step descent of their paths.  The field keeps a 32-bit cost per cell, the
// partition a 64-bit key cost << 32 | label; the two cell policies below are all that tells them apart, so the partition's cost
// plane is the field's bit for bit.  Integers only; the result is the unique fixed point of "no cell can be lowered", so it does
// not depend on the schedule.  Every translation unit that includes this is compiled with -ffp-contract=off.
//
//  - begin (two launches): one pass writes the traversability byte of every cell into the workspace -- bit 0: a move may enter
//    the cell; the plane is what the rounds read, so grid, d_sq and the flags are looked at once --, fills the cells with "none"
//    (or keeps them), marks every tile pending in flag plane 0 and clears plane 1 and the round words; a second launch, one lane
//    per source, seeds the accepted sources' cells and counts them.
//  - a round is one launch, one workgroup of 256 threads per tile of 32 x 32 cells.  A workgroup whose flag in the round's
//    plane is 0 exits at once.  A pending one clears its flag, stages its tile of the cells and of the plane with a one-cell
//    halo in LDS (an off-grid halo cell: no value, not traversable) and relaxes in place -- every thread lowers its four cells
//    to the least of neighbour moved by 5 (axis) / by 7 (diagonal, both passed-between cells traversable) -- until a sweep
//    changes nothing (one workgroup-wide OR per sweep).  In-place means a thread may read a neighbour's value of this sweep or
//    of the last: both are values of real move sequences, and the loop ends only at the tile's fixed point for its halo.
//    Cells that went down are stored; for each of the eight neighbouring tiles whose halo holds one of them the workgroup
//    stores 1 into that tile's flag of the OTHER plane (idempotent) and ORs 1 into the word "something is pending for round
//    r + 1"; a workgroup that lowered anything ORs 1 into "round r changed something".
//  - the halo is read while the neighbour may be storing: a lane sees an older or a newer value of a cell, each the value of a
//    real move sequence, and the neighbour's mark makes this tile run again behind the next kernel boundary, where it sees the
//    final ones.  Kernel boundaries are the only synchronisation between workgroups; nothing waits.
//  - a reader of a key must never pair a new cost with an old label: that key would be lower than any real one and, since keys
//    only go down, would stick.  So a key is one aligned 8-byte word, every load of the key plane in a round and every store to
//    it is a relaxed agent-scope 64-bit atomic, and in LDS a key is read and written whole.  A 32-bit cost cannot tear: plain
//    loads and stores.
//  - the round words rotate over three slots so that a word is cleared in a launch that neither reads nor sets it: round r
//    sets pend[(r + 1) % 3] and chg[r % 3]; its first workgroup adds chg[(r - 1) % 3] to d_state[1] and clears it and
//    pend[(r - 1) % 3].  A closing one-lane launch does the same for the last round and writes d_state[0] from pend.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.hpp"
#include "grid_cell.hpp"  // world_to_grid (grid.cpp:143-159), occupied

namespace eea
{
constexpr int kTX = static_cast<int>(kGeodesicTileX), kTY = static_cast<int>(kGeodesicTileY);
constexpr int kPitch = kTX + 2;                 // a staged row: the tile and its halo
constexpr int kPerThread = kTX * kTY / kBlock;  // cells of a tile per thread
constexpr int kRowStep = kBlock / kTX;          // rows between a thread's cells
static_assert(kBlock % kTX == 0 && (kTX * kTY) % kBlock == 0, "a thread owns whole cells of one column");

// ---- the workspace ---------------------------------------------------------------------------------------------------------
// the traversability plane, then (4-byte aligned) two planes of tile flags and the round words: the field's whole workspace,
// and the tail of the partition's behind its key plane
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
// the planes from `trav`, where the traversability plane starts
inline GeodesicWs tile_workspace(unsigned xsize, unsigned ysize, void* trav)
{
  GeodesicWs w;
  w.tiles_x = (xsize - 1u) / kGeodesicTileX + 1u;
  w.tiles_y = (ysize - 1u) / kGeodesicTileY + 1u;
  w.trav = static_cast<unsigned char*>(trav);
  w.flags = reinterpret_cast<unsigned*>(w.trav + trav_bytes(xsize, ysize));
  w.pend = w.flags + 2u * static_cast<size_t>(w.tiles_x) * w.tiles_y;
  w.chg = w.pend + 3;
  return w;
}
// ... and the bytes they take
inline size_t tile_workspace_bytes(unsigned xsize, unsigned ysize)
{
  const size_t tiles = static_cast<size_t>((xsize - 1u) / kGeodesicTileX + 1u) * ((ysize - 1u) / kGeodesicTileY + 1u);
  return trav_bytes(xsize, ysize) + sizeof(unsigned) * (2 * tiles + 6);
}

// blocks of a grid-stride pass over the cells: four cells per thread, within [1, 4096]
inline unsigned cell_pass_blocks(size_t cells)
{
  const size_t b = cells / (4 * kBlock);
  return static_cast<unsigned>(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

// ---- begin -----------------------------------------------------------------------------------------------------------------
// whether a move may enter cell g of value v: not occupied, known unless unknown cells pass, and with a d_sq clear of clear_sq
__device__ __forceinline__ bool traversable(const CollisionParams& c, const GeodesicArgs& a, int8_t v, const int* __restrict__ sq,
                                            size_t g)
{
  bool ok = !occupied(c, v) && !(a.unknown_blocks && v < 0);
  if (ok && sq != nullptr) {
    const int d = sq[g];
    ok = d == -1 || d > a.clear_sq;
  }
  return ok;
}

// thread t0 of n's share of the state before round 0: every tile pending in flag plane 0, plane 1, the round words and d_state
// cleared
__device__ __forceinline__ void reset_rounds(const GeodesicWs& w, unsigned* __restrict__ state, size_t t0, size_t n)
{
  const size_t tiles = static_cast<size_t>(w.tiles_x) * w.tiles_y;
  for (size_t t = t0; t < 2 * tiles; t += n) w.flags[t] = t < tiles ? 1u : 0u;
  if (t0 < 3) {
    w.pend[t0] = 0u;
    w.chg[t0] = 0u;
  }
  if (t0 < 4) state[t0] = 0u;
}

// the cell of source q, the poses first, then the cells; false where the source is not accepted: a pose off the grid, an
// index outside it, an occupied cell
__device__ __forceinline__ bool source_cell(const CollisionParams& c, const GeodesicArgs& a, const int8_t* __restrict__ grid,
                                            const double* __restrict__ pose, const int* __restrict__ src, size_t q, size_t& at)
{
  if (q < a.P) {
    unsigned j, i;
    world_to_grid(c, pose[3 * q], pose[3 * q + 1], j, i);
    if (!((i <= c.ysize - 1u) && (j <= c.xsize - 1u))) return false;  // gridBounds (grid.cpp:96-100)
    at = static_cast<size_t>(i) * c.xsize + j;
  } else {
    const int k = src[q - a.P];
    if (k < 0 || static_cast<size_t>(k) >= static_cast<size_t>(c.xsize) * c.ysize) return false;
    at = static_cast<size_t>(k);
  }
  return !occupied(c, grid[at]);
}

// ---- the rounds ------------------------------------------------------------------------------------------------------------
// what a cell holds: the stored type, "no move sequence known", the access to the plane in a round, and a value moved on
struct CostCell  // the field: -1 as the plane stores it
{
  using T = unsigned;
  static constexpr T kNone = 0xffffffffu;
  static __device__ __forceinline__ T load(const T* p) { return *p; }
  static __device__ __forceinline__ void store(T* p, T v) { *p = v; }
  // (kNone + 5 wraps to 4: the round skips a neighbour without a value, it does not add to it)
  static __device__ __forceinline__ T moved(T v, unsigned cost) { return v + cost; }
};
struct KeyCell  // the partition: cost << 32 | label, ordered as unsigned integers, which is the order of (cost, label)
{
  using T = unsigned long long;
  static constexpr T kNone = ~0ull;
  static __device__ __forceinline__ T load(const T* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  static __device__ __forceinline__ void store(T* p, T v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  // (a cost stays below 2^31, so the sum keeps the label's half)
  static __device__ __forceinline__ T moved(T v, unsigned cost) { return v + (static_cast<T>(cost) << 32); }
};

// what block 0 does at the start of round r (and the closing launch for the round after the last): the words of round r - 1
__device__ __forceinline__ void tally(const GeodesicWs& w, unsigned* state, unsigned r)
{
  if (r == 0u) return;
  const unsigned prev = (r - 1u) % 3u;
  state[1] += w.chg[prev];
  w.chg[prev] = 0u;
  w.pend[prev] = 0u;
}

// round r of tile blockIdx.x on `plane` [ysize][xsize], by the whole workgroup
template <typename Cell>
__device__ __forceinline__ void tile_round(const GeodesicWs& w, typename Cell::T* plane, unsigned xsize, unsigned ysize, unsigned r,
                                           unsigned* state)
{
  using T = typename Cell::T;
  __shared__ __attribute__((aligned(sizeof(T)))) T s_cell[(kTY + 2) * kPitch];
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
    T v = Cell::kNone;
    unsigned char t = 0;
    if (gy >= 0 && gy < static_cast<long long>(ysize) && gx >= 0 && gx < static_cast<long long>(xsize)) {
      const size_t g = static_cast<size_t>(gy) * xsize + static_cast<size_t>(gx);
      v = Cell::load(&plane[g]);  // (the halo's cells may be stored to by their own tile in this launch)
      t = w.trav[g];
    }
    s_cell[k] = v;
    s_trav[k] = t;
  }
  __syncthreads();
  // this thread's cells: column tid % kTX, rows tid / kTX + m kRowStep
  const int col = tid % kTX, row0 = tid / kTX;
  T before[kPerThread];
  bool open[kPerThread];  // a move may enter the cell
#pragma unroll
  for (int m = 0; m < kPerThread; ++m) {
    const int at = (row0 + m * kRowStep + 1) * kPitch + col + 1;
    before[m] = s_cell[at];
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
      const T was = s_cell[at];
      T best = was;
      const auto take = [&](T v, unsigned cost, bool ok) {
        const T cand = Cell::moved(v, cost);
        best = (ok && v != Cell::kNone && cand < best) ? cand : best;
      };
      take(s_cell[at + 1], 5u, true);
      take(s_cell[at + kPitch], 5u, true);
      take(s_cell[at - 1], 5u, true);
      take(s_cell[at - kPitch], 5u, true);
      take(s_cell[at + kPitch + 1], 7u, te && tn);
      take(s_cell[at + kPitch - 1], 7u, tw && tn);
      take(s_cell[at - kPitch - 1], 7u, tw && ts);
      take(s_cell[at - kPitch + 1], 7u, te && ts);
      if (best < was) {
        s_cell[at] = best;  // (the cell's only writer; one LDS store of the whole value)
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
    const T v = s_cell[(row + 1) * kPitch + col + 1];
    if (v == before[m]) continue;
    const long long gy = y0 + 1 + row, gx = x0 + 1 + col;  // (on the grid: an off-grid cell is not open)
    Cell::store(&plane[static_cast<size_t>(gy) * xsize + static_cast<size_t>(gx)], v);
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

// behind round `last`, by one lane: its words into d_state; final when nothing is pending for the round after it
__device__ __forceinline__ void close_rounds(const GeodesicWs& w, unsigned last, unsigned* state)
{
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  // (the round after `last` would clear pend[last % 3] too: nobody reads it any more)
  tally(w, state, last + 1u);
  state[0] = w.pend[(last + 1u) % 3u] == 0u ? 1u : 0u;
  state[3] = 0u;
}

// ---- the paths -------------------------------------------------------------------------------------------------------------
// headings of the eight moves in the order a walk tries them, (di, dj) = (0,+1) (+1,0) (0,-1) (-1,0) (+1,+1) (+1,-1) (-1,-1)
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

// grid2World's arithmetic (grid.cpp:161-175): the centre of column jj / of row ii
__device__ __forceinline__ double centre_x(const CollisionParams& c, unsigned jj)
{
  return static_cast<double>(jj * c.resolution) + c.resolution / 2.0 + c.xmin;
}
__device__ __forceinline__ double centre_y(const CollisionParams& c, unsigned ii)
{
  return static_cast<double>(ii * c.resolution) + c.resolution / 2.0 + c.ymin;
}

// the field at row ii, column jj; -1 off the grid
__device__ __forceinline__ int field_at(const CollisionParams& c, const int* geo, int ii, int jj)
{
  return (ii >= 0 && ii < static_cast<int>(c.ysize) && jj >= 0 && jj < static_cast<int>(c.xsize))
             ? geo[static_cast<size_t>(ii) * c.xsize + static_cast<size_t>(jj)]
             : -1;
}

// one step of the descent from (ci, cj) of cost `here`: the first move of the table onto a cell that accounts for `here`
// (OWNED: and that `label` owns), a diagonal one only between two cells of the field; the move index, or 8 when there is none
// (a field that is not final may have no step)
template <bool OWNED>
__device__ __forceinline__ int descend(const CollisionParams& c, const int* geo, const int* owner, int label, int& ci, int& cj, int& here)
{
  for (int k = 0; k < 8; ++k) {
    const int di = k < 4 ? (k == 1 ? 1 : k == 3 ? -1 : 0) : (k < 6 ? 1 : -1);
    const int dj = k < 4 ? (k == 0 ? 1 : k == 2 ? -1 : 0) : ((k == 4 || k == 7) ? 1 : -1);
    const int g = field_at(c, geo, ci + di, cj + dj);
    if (g < 0 || g + (k < 4 ? 5 : 7) != here) continue;
    if (OWNED && owner[static_cast<size_t>(ci + di) * c.xsize + static_cast<size_t>(cj + dj)] != label) continue;
    if (k >= 4 && (field_at(c, geo, ci + di, cj) < 0 || field_at(c, geo, ci, cj + dj) < 0)) continue;
    ci += di;
    cj += dj;
    here = g;
    return k;
  }
  return 8;
}
}  // namespace eea
