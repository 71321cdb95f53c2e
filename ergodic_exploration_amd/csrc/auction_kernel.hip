// Frontier auction (include/ergodic_amd.h, eea_frontier_auction): a frontier region for every robot, by distance and capacity.
// The partition of partition_kernel.hip sourced at the REGIONS of frontier_kernel.hip gives, in one build, the distance from any
// robot to its nearest open region; the robots bid for it, a region takes as many of the nearest bidders as it has room for, and
// the build is repeated with the full regions closed.  Integers with a unique answer; a way-point is geodesic_tile.hpp's.
//
//  - once per call (three launches): the traversability plane by traversable(), the state words and both counter pairs; one
//    lane per robot: its cell (or -1) into the workspace, the byte of that cell set in the plane (a robot is where it is: a
//    placed robot's cell may be entered, by every robot, in every auction round -- so the plane is built once), the five outputs
//    in their "unassigned" state, and the placed robots counted; one lane per region: rem_r = its capacity, 0 where it is not
//    eligible, and the open regions counted.
//  - an auction round is begin, the tile rounds, close, unpack, bid, rank, update:
//    begin   a grid-stride pass writes the key plane -- label r for a seed, a member of an open region that does not block, "none"
//            otherwise -- and the state before tile round 0 (reset_rounds).  In an idle round it writes no key and leaves every
//            tile flag 0, so the round launches behind it exit at once.
//    rounds  tile_round<KeyCell> / close_rounds of geodesic_tile.hpp on the key plane; their state words are four words of the
//            workspace, which the bid launch adds into d_state.
//    unpack  the key plane into a cost and a label plane in the workspace: what descend<true> walks.
//    bid     one lane per robot: an unassigned placed robot with a key (cost, r) at its cell stores r and K = cost << 32 | q;
//            the bidders of a region are counted with one integer atomic per distinct region of a wavefront.
//    rank    a robot's rank is the number of bids for its region with a smaller K, counted against all P bids streamed through
//            LDS in tiles of kBlock.  K is unique per robot, so the ranks of a region are a permutation: no atomics.  A robot
//            with rank < rem_r writes its outputs and walks down the field once, writing rows while there is room.
//    update  one lane per region: rem_r -= min(rem_r, bidders_r), the count cleared, the open regions and the unassigned
//            robots counted for the next round.
//  - "idle" (no placed robot unassigned, or no region open) is decided on the device by every launch of a round from the
//    counter pair of that round; the update launch writes the pair of the NEXT round, and rem_r likewise has two copies: no word
//    is read by one workgroup and written by another in the same launch.  An idle round changes nothing, so every later one is
//    idle too.
//  - a robot is unassigned while d_goal_region[q] < 0: the output is the flag, written -1 by the call's own first launches.
// Nothing waits inside a kernel; kernel boundaries are the only synchronisation.
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
using Region = eea_frontier_region;
constexpr u64 kNone = KeyCell::kNone;

// the workspace, 8-byte words first: the key plane and the bids' K [P]; the unpacked cost and label planes; per robot its cell
// and the region it bids for; rem [2][max_regions] and the bidders [max_regions]; eight words -- the tile rounds' state
// {final, rounds that changed something, -, -}, then the counter pairs {unassigned placed robots, open regions} of the even and
// of the odd auction rounds --; the field's workspace
struct AuctionWs
{
  u64* key;
  u64* bid_key;
  int* geo;
  int* owner;
  int* cell;
  int* bid_region;
  unsigned* rem;
  unsigned* bidders;
  unsigned* words;
  GeodesicWs tile;
};
constexpr unsigned kWords = 8;

inline AuctionWs workspace(const CollisionParams& c, unsigned P, unsigned max_regions, void* d_ws)
{
  const size_t cells = static_cast<size_t>(c.xsize) * c.ysize;
  AuctionWs w;
  w.key = static_cast<u64*>(d_ws);
  w.bid_key = w.key + cells;
  w.geo = reinterpret_cast<int*>(w.bid_key + P);
  w.owner = w.geo + cells;
  w.cell = w.owner + cells;
  w.bid_region = w.cell + P;
  w.rem = reinterpret_cast<unsigned*>(w.bid_region + P);
  w.bidders = w.rem + 2 * static_cast<size_t>(max_regions);
  w.words = w.bidders + max_regions;
  w.tile = tile_workspace(c.xsize, c.ysize, w.words + kWords);
  return w;
}

// the counter pair auction round a reads, the one it writes, and whether the round is idle
__device__ __forceinline__ const unsigned* counters(const AuctionWs& w, unsigned a) { return w.words + 4u + 2u * (a & 1u); }
__device__ __forceinline__ unsigned* next_counters(const AuctionWs& w, unsigned a) { return w.words + 4u + 2u * ((a + 1u) & 1u); }
__device__ __forceinline__ bool idle_round(const AuctionWs& w, unsigned a)
{
  const unsigned* const n = counters(w, a);
  return n[0] == 0u || n[1] == 0u;
}

// blocks of a grid-stride pass over n items, within [1, 4096]
inline unsigned item_blocks(size_t n)
{
  const size_t b = (n + kBlock - 1) / kBlock;
  return static_cast<unsigned>(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

// ---- once per call ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void auction_plane_kernel(const CollisionParams c, const AuctionWs w, const GeodesicArgs a,
                                                              const int8_t* __restrict__ grid, const int* __restrict__ sq,
                                                              unsigned* __restrict__ state)
{
  const size_t cells = static_cast<size_t>(c.xsize) * c.ysize;
  const size_t n = static_cast<size_t>(gridDim.x) * kBlock, t0 = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  for (size_t g = t0; g < cells; g += n) w.tile.trav[g] = traversable(c, a, grid[g], sq, g) ? 1 : 0;
  if (t0 < kWords) w.words[t0] = 0u;
  if (t0 < 4) state[t0] = t0 == 0 ? 1u : 0u;
}

// what the call leaves of an empty fleet: d_state alone
__global__ void auction_state_kernel(unsigned* __restrict__ state)
{
  if (threadIdx.x < 4) state[threadIdx.x] = threadIdx.x == 0 ? 1u : 0u;
}

// one lane per robot; every lane of a wavefront stays to the end (the count is a ballot)
__global__ __launch_bounds__(kBlock) void auction_robots_kernel(const CollisionParams c, const AuctionWs w, unsigned P, unsigned n_steps,
                                                               const int8_t* __restrict__ grid, const double* __restrict__ pose,
                                                               int* __restrict__ goal_region, int* __restrict__ goal_cell,
                                                               int* __restrict__ goal_cost, double* __restrict__ path,
                                                               int* __restrict__ len)
{
  const size_t q = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  int at = -1;
  if (q < P) {
    const double wx = pose[3 * q], wy = pose[3 * q + 1], wth = pose[3 * q + 2];
    unsigned j, i;
    world_to_grid(c, wx, wy, j, i);
    if ((i <= c.ysize - 1u) && (j <= c.xsize - 1u)) {  // gridBounds (grid.cpp:96-100)
      const size_t g = static_cast<size_t>(i) * c.xsize + j;
      if (!occupied(c, grid[g])) at = static_cast<int>(g);
    }
    w.cell[q] = at;
    if (at >= 0) w.tile.trav[at] = 1;  // (the plane was written by the launch before; every writer here stores 1)
    goal_region[q] = -1;
    goal_cell[q] = -1;
    goal_cost[q] = -1;
    if (len != nullptr) len[q] = -1;
    double* const out = path + q * n_steps * 3;
    for (unsigned t = 0; t < n_steps; ++t) {
      out[3 * static_cast<size_t>(t)] = wx;
      out[3 * static_cast<size_t>(t) + 1] = wy;
      out[3 * static_cast<size_t>(t) + 2] = wth;
    }
  }
  const u64 placed = __ballot(at >= 0);
  if (threadIdx.x % kWave == 0 && placed != 0ull) atomicAdd(&w.words[4], static_cast<unsigned>(__popcll(placed)));
}

// one lane per record slot; the passes over them are uniform per workgroup (ballots)
__global__ __launch_bounds__(kBlock) void auction_capacity_kernel(const AuctionWs w, unsigned max_regions, unsigned min_size,
                                                                 unsigned cells_per_robot, const Region* __restrict__ regions,
                                                                 const unsigned* __restrict__ fstate)
{
  const unsigned n = fstate[1] < max_regions ? fstate[1] : max_regions;
  const size_t step = static_cast<size_t>(gridDim.x) * kBlock;
  for (size_t base = static_cast<size_t>(blockIdx.x) * kBlock; base < max_regions; base += step) {
    const size_t r = base + threadIdx.x;
    unsigned cap = 0u;
    if (r < n) {
      const unsigned size = regions[r].size;
      if (size >= min_size) {
        cap = cells_per_robot == 0u ? 1u : static_cast<unsigned>((static_cast<u64>(size) + cells_per_robot - 1u) / cells_per_robot);
      }
    }
    if (r < max_regions) {
      w.rem[r] = cap;
      w.bidders[r] = 0u;
    }
    const u64 open = __ballot(cap != 0u);
    if (threadIdx.x % kWave == 0 && open != 0ull) atomicAdd(&w.words[5], static_cast<unsigned>(__popcll(open)));
  }
}

// ---- an auction round: begin, the tile rounds, unpack -----------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void auction_begin_kernel(const CollisionParams c, const AuctionWs w, unsigned round,
                                                              unsigned max_regions, const int8_t* __restrict__ grid,
                                                              const int* __restrict__ region)
{
  const size_t cells = static_cast<size_t>(c.xsize) * c.ysize;
  const size_t n = static_cast<size_t>(gridDim.x) * kBlock, t0 = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  const bool idle = idle_round(w, round);
  if (t0 == 0) {  // the next round's pair before the update launch counts into it
    next_counters(w, round)[0] = counters(w, round)[0];
    next_counters(w, round)[1] = 0u;
  }
  reset_rounds(w.tile, w.words, t0, n);
  if (idle) {  // (uniform) nothing is pending: this thread's share of flag plane 0 again
    const size_t tiles = static_cast<size_t>(w.tile.tiles_x) * w.tile.tiles_y;
    for (size_t t = t0; t < tiles; t += n) w.tile.flags[t] = 0u;
    return;
  }
  const unsigned* const rem = w.rem + static_cast<size_t>(round & 1u) * max_regions;
  for (size_t g = t0; g < cells; g += n) {
    const int r = region[g];
    u64 k = kNone;
    if (r >= 0 && static_cast<unsigned>(r) < max_regions && rem[r] != 0u && !occupied(c, grid[g])) k = static_cast<u64>(r);
    KeyCell::store(&w.key[g], k);
  }
}

__global__ __launch_bounds__(kBlock) void auction_round_kernel(const AuctionWs w, unsigned xsize, unsigned ysize, unsigned r)
{
  tile_round<KeyCell>(w.tile, w.key, xsize, ysize, r, w.words);
}

__global__ void auction_close_kernel(const AuctionWs w, unsigned last) { close_rounds(w.tile, last, w.words); }

__global__ __launch_bounds__(kBlock) void auction_unpack_kernel(const AuctionWs w, unsigned round, size_t cells)
{
  if (idle_round(w, round)) return;
  const size_t n = static_cast<size_t>(gridDim.x) * kBlock;
  for (size_t g = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x; g < cells; g += n) {
    const u64 k = w.key[g];
    w.geo[g] = k == kNone ? -1 : static_cast<int>(k >> 32);
    w.owner[g] = k == kNone ? -1 : static_cast<int>(k & 0xffffffffull);
  }
}

// ---- bid --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void auction_bid_kernel(const AuctionWs w, unsigned round, unsigned P,
                                                            const int* __restrict__ goal_region, unsigned* __restrict__ state)
{
  const size_t q = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  const unsigned lane = threadIdx.x % kWave;
  if (q == 0) {  // the build behind this launch: final or not, and its rounds (an idle round's: final, none)
    state[0] &= w.words[0];
    state[1] += w.words[1];
  }
  int r = -1;
  u64 bid = 0ull;
  if (q < P && !idle_round(w, round)) {
    const int at = w.cell[q];
    if (at >= 0 && goal_region[q] < 0) {
      const u64 k = w.key[at];
      if (k != kNone) {
        r = static_cast<int>(k & 0xffffffffull);
        bid = (k & 0xffffffff00000000ull) | static_cast<u64>(q);
      }
    }
  }
  if (q < P) {
    w.bid_region[q] = r;
    w.bid_key[q] = bid;
  }
  u64 left = __ballot(r >= 0);
  while (left != 0ull) {  // (uniform: one turn per distinct region of the wavefront)
    const int lead = __ffsll(static_cast<long long>(left)) - 1;
    const int l = __builtin_amdgcn_readlane(r, lead);
    const u64 group = __ballot(r == l);
    left &= ~group;
    if (lane == static_cast<unsigned>(lead)) atomicAdd(&w.bidders[l], static_cast<unsigned>(__popcll(group)));
  }
}

// ---- rank, accept and walk --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void auction_rank_kernel(const CollisionParams c, const AuctionWs w, unsigned round, unsigned P,
                                                             unsigned max_regions, unsigned n_steps, const double* __restrict__ pose,
                                                             int* __restrict__ goal_region, int* __restrict__ goal_cell,
                                                             int* __restrict__ goal_cost, double* __restrict__ path,
                                                             int* __restrict__ len)
{
  __shared__ int s_region[kBlock];
  __shared__ u64 s_key[kBlock];
  const unsigned tid = threadIdx.x;
  const size_t q = static_cast<size_t>(blockIdx.x) * kBlock + tid;
  const int mine = q < P ? w.bid_region[q] : -1;
  const u64 my_key = q < P ? w.bid_key[q] : 0ull;
  if (__syncthreads_or(mine >= 0 ? 1 : 0) == 0) return;  // (uniform) nobody here bids: an idle round, too
  unsigned rank = 0u;
  for (size_t base = 0; base < P; base += kBlock) {  // (uniform)
    const size_t j = base + tid;
    s_region[tid] = j < P ? w.bid_region[j] : -1;
    s_key[tid] = j < P ? w.bid_key[j] : 0ull;
    __syncthreads();
    if (mine >= 0) {
      // (every lane reads the same word of LDS: a broadcast)
      for (int t = 0; t < kBlock; ++t) rank += (s_region[t] == mine && s_key[t] < my_key) ? 1u : 0u;
    }
    __syncthreads();
  }
  if (mine < 0 || rank >= w.rem[static_cast<size_t>(round & 1u) * max_regions + static_cast<unsigned>(mine)]) return;
  // accepted: down the field from the robot's own cell until the cost is 0 (a field that is not final may have no step)
  const int at = w.cell[q];
  int ci = at / static_cast<int>(c.xsize), cj = at % static_cast<int>(c.xsize), here = static_cast<int>(my_key >> 32);
  goal_region[q] = mine;
  goal_cost[q] = here;
  // until a step is written the rows hold the centre of the robot's own cell with the pose's heading
  double wx = centre_x(c, static_cast<unsigned>(cj)), wy = centre_y(c, static_cast<unsigned>(ci)), wth = pose[3 * q + 2];
  double* const out = path + q * n_steps * 3;
  unsigned moves = 0u;
  while (here > 0) {
    const int k = descend<true>(c, w.geo, w.owner, mine, ci, cj, here);
    if (k == 8) break;
    if (moves < n_steps) {
      wx = centre_x(c, static_cast<unsigned>(cj));
      wy = centre_y(c, static_cast<unsigned>(ci));
      wth = move_heading(k);
      out[3 * static_cast<size_t>(moves)] = wx;
      out[3 * static_cast<size_t>(moves) + 1] = wy;
      out[3 * static_cast<size_t>(moves) + 2] = wth;
    }
    ++moves;
  }
  goal_cell[q] = ci * static_cast<int>(c.xsize) + cj;
  for (unsigned t = moves; t < n_steps; ++t) {
    out[3 * static_cast<size_t>(t)] = wx;
    out[3 * static_cast<size_t>(t) + 1] = wy;
    out[3 * static_cast<size_t>(t) + 2] = wth;
  }
  if (len != nullptr) len[q] = static_cast<int>(moves < n_steps ? moves : n_steps);
}

// ---- update -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void auction_update_kernel(const AuctionWs w, unsigned round, unsigned max_regions,
                                                               unsigned* __restrict__ state)
{
  const unsigned lane = threadIdx.x % kWave;
  const unsigned* const rem = w.rem + static_cast<size_t>(round & 1u) * max_regions;
  unsigned* const rem_next = w.rem + static_cast<size_t>((round + 1u) & 1u) * max_regions;
  unsigned* const next = next_counters(w, round);
  if (blockIdx.x == 0 && threadIdx.x == 0 && !idle_round(w, round)) state[3] += 1u;
  const size_t step = static_cast<size_t>(gridDim.x) * kBlock;
  for (size_t base = static_cast<size_t>(blockIdx.x) * kBlock; base < max_regions; base += step) {  // (uniform)
    const size_t r = base + threadIdx.x;
    unsigned taken = 0u, left = 0u;
    if (r < max_regions) {
      const unsigned room = rem[r], bidders = w.bidders[r];
      taken = room < bidders ? room : bidders;
      left = room - taken;
      rem_next[r] = left;
      w.bidders[r] = 0u;
    }
    const u64 open = __ballot(left != 0u);
#pragma unroll
    for (int m = kWave / 2; m >= 1; m >>= 1) taken += __shfl_xor(taken, m, kWave);
    if (lane == 0u) {
      if (open != 0ull) atomicAdd(&next[1], static_cast<unsigned>(__popcll(open)));
      if (taken != 0u) {
        atomicSub(&next[0], taken);
        atomicAdd(&state[2], taken);
      }
    }
  }
}
}  // namespace

size_t auction_ws_bytes(unsigned xsize, unsigned ysize, unsigned P, unsigned max_regions)
{
  const size_t cells = static_cast<size_t>(xsize) * ysize;
  return (sizeof(u64) + 2 * sizeof(int)) * (cells + P) + 3 * sizeof(unsigned) * static_cast<size_t>(max_regions) +
         sizeof(unsigned) * kWords + tile_workspace_bytes(xsize, ysize);
}

const unsigned* auction_words(const CollisionParams& c, const AuctionArgs& a, void* d_ws)
{
  return workspace(c, a.P, a.max_regions, d_ws).words;
}

hipError_t launch_auction_state(unsigned* d_state, hipStream_t s)
{
  hipLaunchKernelGGL(auction_state_kernel, dim3(1), dim3(kWave), 0, s, d_state);
  return hipGetLastError();
}

hipError_t launch_auction_setup(const CollisionParams& c, const AuctionArgs& a, const int8_t* d_grid, const int* d_sq,
                                const eea_frontier_region* d_regions, const unsigned* d_fstate, const double* d_pose,
                                int* d_goal_region, int* d_goal_cell, int* d_goal_cost, double* d_path, int* d_len, void* d_ws,
                                unsigned* d_state, hipStream_t s)
{
  const AuctionWs w = workspace(c, a.P, a.max_regions, d_ws);
  const unsigned blocks = cell_pass_blocks(static_cast<size_t>(c.xsize) * c.ysize);
  hipLaunchKernelGGL(auction_plane_kernel, dim3(blocks), dim3(kBlock), 0, s, c, w, a.g, d_grid, d_sq, d_state);
  hipLaunchKernelGGL(auction_robots_kernel, dim3((a.P - 1u) / kBlock + 1u), dim3(kBlock), 0, s, c, w, a.P, a.n_steps, d_grid, d_pose,
                     d_goal_region, d_goal_cell, d_goal_cost, d_path, d_len);
  if (a.max_regions != 0u) {
    hipLaunchKernelGGL(auction_capacity_kernel, dim3(item_blocks(a.max_regions)), dim3(kBlock), 0, s, w, a.max_regions, a.min_size,
                       a.cells_per_robot, d_regions, d_fstate);
  }
  return hipGetLastError();
}

hipError_t launch_auction_begin(const CollisionParams& c, const AuctionArgs& a, unsigned round, const int8_t* d_grid,
                                const int* d_region, void* d_ws, hipStream_t s)
{
  const AuctionWs w = workspace(c, a.P, a.max_regions, d_ws);
  const unsigned blocks = cell_pass_blocks(static_cast<size_t>(c.xsize) * c.ysize);
  hipLaunchKernelGGL(auction_begin_kernel, dim3(blocks), dim3(kBlock), 0, s, c, w, round, a.max_regions, d_grid, d_region);
  return hipGetLastError();
}

hipError_t launch_auction_rounds(const CollisionParams& c, const AuctionArgs& a, unsigned first, unsigned count, void* d_ws,
                                 hipStream_t s)
{
  const AuctionWs w = workspace(c, a.P, a.max_regions, d_ws);
  for (unsigned r = first; r < first + count; ++r) {
    hipLaunchKernelGGL(auction_round_kernel, dim3(w.tile.tiles_x * w.tile.tiles_y), dim3(kBlock), 0, s, w, c.xsize, c.ysize, r);
  }
  hipLaunchKernelGGL(auction_close_kernel, dim3(1), dim3(64), 0, s, w, first + count - 1u);
  return hipGetLastError();
}

hipError_t launch_auction_settle(const CollisionParams& c, const AuctionArgs& a, unsigned round, const double* d_pose,
                                 int* d_goal_region, int* d_goal_cell, int* d_goal_cost, double* d_path, int* d_len, void* d_ws,
                                 unsigned* d_state, hipStream_t s)
{
  const AuctionWs w = workspace(c, a.P, a.max_regions, d_ws);
  const size_t cells = static_cast<size_t>(c.xsize) * c.ysize;
  const unsigned pb = (a.P - 1u) / kBlock + 1u;
  hipLaunchKernelGGL(auction_unpack_kernel, dim3(cell_pass_blocks(cells)), dim3(kBlock), 0, s, w, round, cells);
  hipLaunchKernelGGL(auction_bid_kernel, dim3(pb), dim3(kBlock), 0, s, w, round, a.P, d_goal_region, d_state);
  hipLaunchKernelGGL(auction_rank_kernel, dim3(pb), dim3(kBlock), 0, s, c, w, round, a.P, a.max_regions, a.n_steps, d_pose,
                     d_goal_region, d_goal_cell, d_goal_cost, d_path, d_len);
  hipLaunchKernelGGL(auction_update_kernel, dim3(item_blocks(a.max_regions)), dim3(kBlock), 0, s, w, round, a.max_regions, d_state);
  return hipGetLastError();
}
}  // namespace eea
