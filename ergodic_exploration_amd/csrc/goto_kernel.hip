// Goal paths (include/ergodic_amd.h, eea_geodesic_goto_batch): every robot's shortest way to its OWN goal cell, inside a bounded
// window around the two.  The field of geodesic_tile.hpp with one source, the goal, on the cells of the window only; the walk
// down it is that header's descend.  Integers with a unique answer; a way-point is geodesic_tile.hpp's.
//
//  - one launch clears the four counts; the launch behind it does everything else: one workgroup of kBlock threads per robot, a
//    launch of fewer workgroups than robots strides over them.
//  - a workgroup decides the robot's status from the pose, the goal and the grid (every thread the same few loads), stages the
//    window in LDS -- one 32-bit word per cell: "wall" where traversable() says no (the robot's own cell excepted), else "none",
//    0 at the goal; the word a sweep reads for a neighbour's cost is the one that says whether a diagonal may pass it, so there
//    is no plane of bytes: 16384 cells are 64 KB and two workgroups share a CU --, and relaxes in place as tile_round does: a
//    thread lowers the cells k = tid, tid + kBlock, ... of the row-major window (lanes hold consecutive cells: a 4-byte stride
//    over the banks) to the least of neighbour moved by 5 / by 7 (both passed-between cells traversable), until a sweep changes
//    nothing (one workgroup-wide OR per sweep).
//    The window has no halo -- a 1 x 16384 one would triple --: a move that would leave it is masked by the cell's row and column.
//    Values only go down and every value is the cost of a real move sequence, so the loop ends, at the window's fixed point.
//  - only per-robot outputs leave the window, so a candidate value >= the cost the robot's own cell holds is not stored
//    (EEA_GOTO_PRUNE): every cell of the walk costs less than the robot's, so do both cells beside a diagonal step, and a cell
//    whose final cost is below the robot's still reaches it, through cells that cost less still.  What the pruned window holds
//    elsewhere is not final, and is not read.
//  - thread 0 walks down from the robot's cell and writes a row per move while there is room; every thread then repeats the
//    last row to the end.  A robot without a path gets its pose in every row, written by every thread.
//  - the counts are kept per workgroup in registers of thread 0 and added to d_state once at the end: at most four atomics
//    per workgroup.  Nothing waits on another workgroup; no workspace.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/ergodic_amd.h"
#include "common.hpp"
#include "geodesic_tile.hpp"

#ifndef EEA_GOTO_PRUNE
#define EEA_GOTO_PRUNE 1
#endif

namespace eea
{
static_assert(kGotoMaxCells == EEA_GOTO_MAX_CELLS, "the header publishes the cap");

namespace
{
constexpr unsigned kNone = CostCell::kNone;
constexpr unsigned kWall = kNone - 1u;  // no move may enter the cell (as an int it is < 0, like "none": descend sees no cost)

__global__ void goto_state_kernel(unsigned* __restrict__ state)
{
  if (threadIdx.x < 4) state[threadIdx.x] = 0u;
}

// the pose of robot q into rows first .. n_steps - 1 of its path, by the whole workgroup
__device__ __forceinline__ void fill_rows(double* __restrict__ out, unsigned first, unsigned n_steps, double wx, double wy, double wth)
{
  for (unsigned t = first + threadIdx.x; t < n_steps; t += kBlock) {
    out[3 * static_cast<size_t>(t)] = wx;
    out[3 * static_cast<size_t>(t) + 1] = wy;
    out[3 * static_cast<size_t>(t) + 2] = wth;
  }
}

__global__ __launch_bounds__(kBlock) void goto_kernel(const CollisionParams c, const GotoArgs a, unsigned max_cells,
                                                     const int8_t* __restrict__ grid, const int* __restrict__ sq,
                                                     const double* __restrict__ pose, const int* __restrict__ goal,
                                                     const int* __restrict__ mask, int* __restrict__ cost, int* __restrict__ status,
                                                     double* __restrict__ path, int* __restrict__ len, unsigned* __restrict__ state)
{
  extern __shared__ __attribute__((aligned(16))) unsigned s_cell[];  // [h][w]
  __shared__ unsigned s_moves;
  __shared__ double s_last[3];
  const int tid = threadIdx.x;
  const size_t cells = static_cast<size_t>(c.xsize) * c.ysize;
  unsigned n_ok = 0u, n_window = 0u, n_cut = 0u, n_bad = 0u;  // (thread 0's are the workgroup's)
  for (unsigned q = blockIdx.x; q < a.P; q += gridDim.x) {
    if (mask != nullptr && mask[q] == 0) continue;  // (uniform)
    __syncthreads();                                // the robot before has read the window
    const double px = pose[3 * static_cast<size_t>(q)], py = pose[3 * static_cast<size_t>(q) + 1], pth = pose[3 * static_cast<size_t>(q) + 2];
    double* const out = path + static_cast<size_t>(q) * a.n_steps * 3;
    // ---- the status, by every thread alike ----
    int st = EEA_GOTO_OK;
    unsigned cj, ci;
    world_to_grid(c, px, py, cj, ci);
    int i0 = 0, j0 = 0, h = 0, w = 0, gi = 0, gj = 0;
    bool goal_open = true;  // a diagonal move may pass the goal's cell
    if (!((ci <= c.ysize - 1u) && (cj <= c.xsize - 1u)) || occupied(c, grid[static_cast<size_t>(ci) * c.xsize + cj])) {
      st = EEA_GOTO_NO_ROBOT;  // gridBounds (grid.cpp:96-100), then blocks
    } else {
      const int g = goal[q];
      if (g < 0 || static_cast<size_t>(g) >= cells || occupied(c, grid[g])) {
        st = EEA_GOTO_NO_GOAL;
      } else {
        goal_open = traversable(c, a.g, grid[g], sq, static_cast<size_t>(g)) || static_cast<size_t>(g) == static_cast<size_t>(ci) * c.xsize + cj;
        gi = g / static_cast<int>(c.xsize);
        gj = g % static_cast<int>(c.xsize);
        const long long m = static_cast<long long>(a.margin), ri = static_cast<long long>(ci), rj = static_cast<long long>(cj);
        long long lo_i = (ri < gi ? ri : gi) - m, hi_i = (ri > gi ? ri : gi) + m;
        long long lo_j = (rj < gj ? rj : gj) - m, hi_j = (rj > gj ? rj : gj) + m;
        lo_i = lo_i < 0 ? 0 : lo_i;
        lo_j = lo_j < 0 ? 0 : lo_j;
        hi_i = hi_i > static_cast<long long>(c.ysize) - 1 ? static_cast<long long>(c.ysize) - 1 : hi_i;
        hi_j = hi_j > static_cast<long long>(c.xsize) - 1 ? static_cast<long long>(c.xsize) - 1 : hi_j;
        // (a side is at most the grid's, so the product stays far inside 64 bits; max_cells = min(cells, the cap))
        if ((hi_i - lo_i + 1) * (hi_j - lo_j + 1) > static_cast<long long>(max_cells)) {
          st = EEA_GOTO_WINDOW;
        } else {
          i0 = static_cast<int>(lo_i);
          j0 = static_cast<int>(lo_j);
          h = static_cast<int>(hi_i - lo_i + 1);
          w = static_cast<int>(hi_j - lo_j + 1);
        }
      }
    }
    int here = -1;
    if (st == EEA_GOTO_OK) {  // (uniform)
      // ---- stage ----
      const int n = h * w;
      const int at_robot = (static_cast<int>(ci) - i0) * w + (static_cast<int>(cj) - j0), at_goal = (gi - i0) * w + (gj - j0);
      {
        int r = tid / w, col = tid % w;
        const int dr = kBlock / w, dc = kBlock % w;
        for (int k = tid; k < n; k += kBlock) {
          const size_t g = static_cast<size_t>(i0 + r) * c.xsize + static_cast<size_t>(j0 + col);
          s_cell[k] = k == at_goal ? 0u : ((k == at_robot || traversable(c, a.g, grid[g], sq, g)) ? kNone : kWall);
          r += dr;
          col += dc;
          if (col >= w) {
            col -= w;
            ++r;
          }
        }
      }
      __syncthreads();
      // ---- relax ----
      const int col0 = tid % w, dc = kBlock % w;
      for (;;) {
        int changed = 0;
#if EEA_GOTO_PRUNE
        const unsigned bound = s_cell[at_robot];  // (this sweep's or the last's: either is the cost of a real move sequence)
#endif
        int col = col0;
        for (int k = tid; k < n; k += kBlock) {
          const unsigned was = s_cell[k];
          if (was != kWall && k != at_goal) {  // (the goal's 0 cannot go down)
            // the four axis neighbours' words; outside the window: a wall
            const unsigned ve = col + 1 < w ? s_cell[k + 1] : kWall, vn = k + w < n ? s_cell[k + w] : kWall;
            const unsigned vw = col > 0 ? s_cell[k - 1] : kWall, vs = k >= w ? s_cell[k - w] : kWall;
            // a diagonal move may pass the cell: no wall, and not a goal that is seeded through the waiver alone
            const bool te = ve != kWall && (goal_open || k + 1 != at_goal), tn = vn != kWall && (goal_open || k + w != at_goal);
            const bool tw = vw != kWall && (goal_open || k - 1 != at_goal), ts = vs != kWall && (goal_open || k - w != at_goal);
#if EEA_GOTO_PRUNE
            unsigned best = (k == at_robot || was < bound) ? was : bound;
#else
            unsigned best = was;
#endif
            const unsigned start = best;
            const auto take = [&](unsigned v, unsigned move) {  // (a wall or "none" has no cost to move on)
              const unsigned cand = CostCell::moved(v, move);
              best = (v < kWall && cand < best) ? cand : best;
            };
            take(ve, 5u);
            take(vn, 5u);
            take(vw, 5u);
            take(vs, 5u);
            // (both passed cells are in the window, so the diagonal one is)
            if (te && tn) take(s_cell[k + w + 1], 7u);
            if (tw && tn) take(s_cell[k + w - 1], 7u);
            if (tw && ts) take(s_cell[k - w - 1], 7u);
            if (te && ts) take(s_cell[k - w + 1], 7u);
            if (best < start) {
              s_cell[k] = best;  // (the cell's only writer; one LDS store of the whole value)
              changed = 1;
            }
          }
          col += dc;
          if (col >= w) col -= w;
        }
        if (__syncthreads_or(changed) == 0) break;
      }
      here = static_cast<int>(s_cell[at_robot]);  // (-1: none; the robot's own cell is no wall)
      if (here < 0) st = EEA_GOTO_CUT_OFF;
    }
    // ---- the outputs ----
    if (st != EEA_GOTO_OK) {
      if (tid == 0) {
        cost[q] = -1;
        status[q] = st;
        if (len != nullptr) len[q] = -1;
        n_window += st == EEA_GOTO_WINDOW ? 1u : 0u;
        n_cut += st == EEA_GOTO_CUT_OFF ? 1u : 0u;
        n_bad += (st == EEA_GOTO_NO_ROBOT || st == EEA_GOTO_NO_GOAL) ? 1u : 0u;
      }
      fill_rows(out, 0u, a.n_steps, px, py, pth);
      continue;
    }
    if (tid == 0) {
      // down the field from the robot's own cell: descend on the window as a grid of its own, the centres on the whole grid's
      CollisionParams win = c;
      win.xsize = static_cast<unsigned>(w);
      win.ysize = static_cast<unsigned>(h);
      const int* const geo = reinterpret_cast<const int*>(s_cell);
      int wi = static_cast<int>(ci) - i0, wj = static_cast<int>(cj) - j0, left = here;
      // until a step is written the rows hold the centre of the robot's own cell with the pose's heading
      double wx = centre_x(c, cj), wy = centre_y(c, ci), wth = pth;
      unsigned moves = 0u;
      while (left > 0 && moves < a.n_steps) {
        const int k = descend<false>(win, geo, nullptr, 0, wi, wj, left);
        if (k == 8) break;  // (not in a final field)
        wx = centre_x(c, static_cast<unsigned>(j0 + wj));
        wy = centre_y(c, static_cast<unsigned>(i0 + wi));
        wth = move_heading(k);
        out[3 * static_cast<size_t>(moves)] = wx;
        out[3 * static_cast<size_t>(moves) + 1] = wy;
        out[3 * static_cast<size_t>(moves) + 2] = wth;
        ++moves;
      }
      cost[q] = here;
      status[q] = EEA_GOTO_OK;
      if (len != nullptr) len[q] = static_cast<int>(moves);
      n_ok += 1u;
      s_moves = moves;
      s_last[0] = wx;
      s_last[1] = wy;
      s_last[2] = wth;
    }
    __syncthreads();
    fill_rows(out, s_moves, a.n_steps, s_last[0], s_last[1], s_last[2]);
  }
  if (tid == 0) {
    if (n_ok != 0u) atomicAdd(&state[0], n_ok);
    if (n_window != 0u) atomicAdd(&state[1], n_window);
    if (n_cut != 0u) atomicAdd(&state[2], n_cut);
    if (n_bad != 0u) atomicAdd(&state[3], n_bad);
  }
}
}  // namespace

hipError_t launch_goto(const CollisionParams& c, const GotoArgs& a, const int8_t* d_grid, const int* d_sq, const double* d_pose,
                       const int* d_goal, const int* d_mask, int* d_cost, int* d_status, double* d_path, int* d_len,
                       unsigned* d_state, hipStream_t s)
{
  hipLaunchKernelGGL(goto_state_kernel, dim3(1), dim3(kWave), 0, s, d_state);
  if (a.P == 0u) return hipGetLastError();
  // the largest window the launch can meet: no side is longer than the grid's
  const size_t cells = static_cast<size_t>(c.xsize) * c.ysize;
  const unsigned max_cells = static_cast<unsigned>(cells < kGotoMaxCells ? cells : kGotoMaxCells);
  const size_t lds = sizeof(unsigned) * max_cells;
  if (lds + 1024 > 64 * 1024) {  // (with the kernel's few static words: past what a launch gets unasked)
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(goto_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             static_cast<int>(lds));
    if (e != hipSuccess) return e;
  }
  const unsigned blocks = a.P < kGotoMaxBlocks ? a.P : kGotoMaxBlocks;
  hipLaunchKernelGGL(goto_kernel, dim3(blocks), dim3(kBlock), lds, s, c, a, max_cells, d_grid, d_sq, d_pose, d_goal, d_mask, d_cost,
                     d_status, d_path, d_len, d_state);
  return hipGetLastError();
}
}  // namespace eea
