// Footprint planning for gfx950: validate_control (numerics.hpp:312-330) and DynamicWindow::control
// (dynamic_window.cpp:92-286) for a convex polygon base.  The poses of a rollout are those of validate_control_kernel /
// dwa_control_kernel (collision_kernel.hip) bit for bit -- the twist step is twist_step.hpp's, this file is compiled without FMA
// contraction like that one -- and the verdict of a pose is footprint_kernel.hip's: some occupied in-grid cell has its centre in
// the closed polygon placed at the pose (footprint_cell_test.hpp: classify through one int of the distance field, then the
// exact test).  Sine and cosine of a pose's heading come from tick_sincos, as the rollout's own do.
//
// footprint_validate_kernel   One lane per robot.  The step loop is wavefront-uniform: a lane with a verdict stays in it, masked,
//            until every lane has one; the ambiguous poses of a step are resolved by the wavefront together (resolve), their
//            cells read from the grid in memory -- the robots of a wavefront are anywhere on the map.
// footprint_dwa_kernel        One workgroup per robot, one lane per velocity sample (64 or 128 threads, one cost per sample in
//            dynamic LDS; the scan for the first strict minimum and the fleet tick's bookkeeping are dwa_control_kernel's).
//            Every pose of every sample lies within a known reach of x0: a step of a constant twist moves the body by a chord
//            of at most |(u0, u1)| dt, so no pose's cell is farther than
//                reach = ceil(steps * |dt| * sqrt(mx^2 + my^2) / res) + 1   cells
//            from x0's, mx / my the largest |lower|, |upper| of the robot's window.  The workgroup stages the occupancy of the
//            cells within reach + box of x0's cell ONCE, as bit rows in LDS (a ballot over 64 consecutive cells of a grid row
//            is one 64-bit word), and every ambiguous lane then resolves ITS OWN pose from those bits: no lane waits for
//            another's pose and no cell load leaves the CU inside the step loop -- only the one int of the distance field
//            per step does.  Per row of its box a lane keeps the occupied cells in the columns the polygon can cover (row_span:
//            an fp32 filter, a cell wider than the truth on either side) and tests those with resolve's products and sums --
//            beside a solid obstacle a box holds hundreds of occupied cells, and a wavefront waits for its slowest lane.  The host sizes the window from vmin / vmax; a robot whose own reach is larger (vb outside the
//            limits: lower above vmax), whose x0 is not finite, or a launch whose window does not fit the LDS takes its cells
//            from memory through the cooperative resolve instead, with the same verdicts: a workgroup-uniform choice.
//
// Both kernels are templates over their last argument: NoBodies (the instances above, unchanged) or BodyArgs, the body layer
// (body_layer_kernel.hip): a cell is then occupied when the grid says so or a stamped robot other than the pose's own covers
// it.  The window's staging ORs those cells into the LDS bit rows (the robot's own body taken out where cover > 0) and leaves
// one workgroup-uniform flag, "the window holds a body bit": without it a pose the field calls free is free; with it -- and on
// the memory path wherever the layer's near map does not prove the opposite -- such a pose takes the exact test.
#include <cmath>
#include <cstdint>

#include "../../include/ergodic_amd.h"
#include "common.hpp"
#include "footprint_cell_test.hpp"
#include "footprint_planes.hpp"
#include "grid_cell.hpp"
#include "twist_step.hpp"

namespace eea
{
namespace
{
constexpr int kPlanBlock = 128;  // dwa_control_kernel's block rule: 64 threads up to 64 samples, 128 beyond
constexpr size_t kLdsLimit = 64 * 1024;
constexpr size_t kBodyFlagBytes = sizeof(unsigned long long) * (kPlanBlock / kWave);

// the ambiguous lanes of one step, resolved by the wavefront one after the other; true in the lanes whose pose collides.
// Called by all lanes of a wavefront together
template <class BV = NoBodies>
__device__ __forceinline__ bool resolve_together(const CollisionParams& c, const FootprintArgs& f, const PlaneRegs& pl,
                                                 const int8_t* __restrict__ grid, bool ambiguous, double px, double py, double th,
                                                 const Box& b, int lane, BV bv = BV{})
{
  unsigned long long todo = __ballot(ambiguous);
  double sn = 0.0, cs = 0.0;
  if (ambiguous) tick_sincos(th, &sn, &cs);
  bool hit = false;
  while (todo != 0ull) {
    const int src = __ffsll(static_cast<long long>(todo)) - 1;
    todo &= todo - 1ull;
    const bool h = resolve(c, f, pl, grid, src, px, py, sn, cs, b, lane, bv);
    if (lane == src) hit = h;
  }
  return hit;
}

// what a kernel instance judges poses with: nothing, or the layer as the lane sees it
template <class VIEW>
struct BodiesOf
{
  using type = NoBodies;
};
template <>
struct BodiesOf<BodyArgs>
{
  using type = Bodies;
};

template <class VIEW>
__global__ __launch_bounds__(kBlock) void footprint_validate_kernel(const CollisionParams c, const FootprintArgs f,
                                                                    const int8_t* __restrict__ grid, const int* __restrict__ d_sq,
                                                                    const double* __restrict__ x0, const double* __restrict__ u,
                                                                    double dt, unsigned steps, unsigned P, int* __restrict__ valid,
                                                                    const VIEW view)
{
  const int lane = threadIdx.x % kWave;
  const size_t q = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  const PlaneRegs pl = load_planes(f, lane);
  const bool live = q < P;
  double x = 0.0, y = 0.0, th = 0.0, d0 = 0.0, d1 = 0.0, d2 = 0.0;
  typename BodiesOf<VIEW>::type bv{};
  if constexpr (std::is_same_v<VIEW, BodyArgs>) {
    bv.v = view.v;
    if (live) bv = load_bodies(view, q);
  }
  if (live) {
    x = x0[3 * q];
    y = x0[3 * q + 1];
    th = x0[3 * q + 2];
    body_displacement<true>(u[3 * q], u[3 * q + 1], u[3 * q + 2], dt, d0, d1, d2);
  }
  bool done = !live;
  int ok = 1;
  for (unsigned i = 0; i < steps; ++i) {
    if (__all(done)) break;
    Box b{ 0, -1, 0, -1 };
    int cls = kFree;
    if (!done) {
      advance_pose<true>(x, y, th, d0, d1, d2, true);
      cls = classify_with(c, f, d_sq, x, y, th, b, bv);
    }
    const bool h = resolve_together(c, f, pl, grid, cls == kAmbiguous, x, y, th, b, lane, bv);
    if (cls == kHit || h) {
      ok = 0;
      done = true;
    }
  }
  if (live) valid[q] = ok;
}

// the robot's window of the grid as bit rows in LDS: cell (wy0 + r, wx0 + 64 k + bit) is bit `bit` of word r * nw + k
struct Window
{
  const unsigned long long* bits;
  int nw;                  // words per row
  int wx0, wx1, wy0, wy1;  // inclusive, inside the grid; wx1 < wx0: no cell
};

// Which columns of grid row `dy` can hold a centre inside the polygon: in a row the body coordinates are linear in dx, so every
// half-plane is a * dx + c <= 0 with a = nx cs - ny sn, c = (nx sn + ny cs) dy - h, and their intersection is an interval of
// columns.  A FILTER in fp32, wider than the truth by one cell on either side (r_out / res <= 1024: every length here is below
// 1025 cells, fp32 keeps it to 1e-3 of a cell; a half-plane within 1e-3 of parallel to the row moves by less than 1.1 cells over
// the box and only empties the row when it misses it by two cells).  Returns the columns relative to the box's first as
// [lo, hi], lo > hi: none.  dx0 = the first column's dx
__device__ __forceinline__ void row_span(const FootprintArgs& f, const PlaneRegs& pl, float res, float inv_res, float sn, float cs,
                                         float dx0, float dy, int width, int& lo, int& hi)
{
  float flo = 0.0f, fhi = static_cast<float>(width - 1);
  for (int kk = 0; kk < static_cast<int>(f.n); ++kk) {
    const int ku = __builtin_amdgcn_readfirstlane(kk);
    const float nx = static_cast<float>(lane_value(pl.nx, ku)), ny = static_cast<float>(lane_value(pl.ny, ku));
    const float h = static_cast<float>(lane_value(pl.h, ku));
    const float a = nx * cs - ny * sn, c = (nx * sn + ny * cs) * dy - h;
    if (fabsf(a) < 1.0e-3f) {
      if (c > 2.0f * res) fhi = -1.0f;
    } else {
      const float t = (-c * __builtin_amdgcn_rcpf(a) - dx0) * inv_res;  // the crossing, in columns from the box's first
      if (a > 0.0f) fhi = fminf(fhi, t + 1.0f);
      else flo = fmaxf(flo, t - 1.0f);
    }
  }
  lo = static_cast<int>(ceilf(flo));
  hi = static_cast<int>(floorf(fhi));
}

// the exact test of the lane's own pose over its box, the occupancy from the window's bits; the box lies inside the window.
// Products and sums in resolve's order, on the occupied cells row_span leaves.  The trip counts differ from lane to lane, k of
// the plane loops does not: the lanes inside one run it together from 0
__device__ __forceinline__ bool resolve_window(const CollisionParams& c, const FootprintArgs& f, const PlaneRegs& pl, const Window& w,
                                               double px, double py, double sn, double cs, const Box& b)
{
  const int c0 = b.x0 - w.wx0, c1 = b.x1 - w.wx0;
  const float res = static_cast<float>(c.resolution), inv_res = 1.0f / res, fs = static_cast<float>(sn), fc = static_cast<float>(cs);
  const float dx0 = static_cast<float>(static_cast<double>(b.x0) * c.resolution + c.resolution / 2.0 + c.xmin - px);
  constexpr int kRows = 4;  // row words read from LDS before the first of them is looked at
  // every word of a window row the box touches: one or two up to 65 columns, eleven at most where the window still fits the LDS
  // (tests/test_gpu_footprint_edges.py runs one to ten words, c0 on either side of a word seam, every box height modulo kRows)
  for (int k = c0 >> 6; k <= (c1 >> 6); ++k) {
    const int lo = max(c0 - 64 * k, 0), hi = min(c1 - 64 * k, 63);
    const unsigned long long in_box = (~0ull << lo) & (~0ull >> (63 - hi));
    for (int i0 = b.y0; i0 <= b.y1; i0 += kRows) {
      unsigned long long words[kRows];
#pragma unroll
      for (int u = 0; u < kRows; ++u) {
        const int i = min(i0 + u, b.y1);  // (a row past the box reads the last one and is dropped)
        words[u] = w.bits[static_cast<size_t>(i - w.wy0) * w.nw + k] & in_box;
        if (i0 + u > b.y1) words[u] = 0ull;
      }
#pragma unroll
      for (int u = 0; u < kRows; ++u) {
        unsigned long long word = words[u];
        if (word == 0ull) continue;  // no occupied cell of this row in the box
        const int i = i0 + u;
        const double cyw = static_cast<double>(i) * c.resolution + c.resolution / 2.0 + c.ymin;
        const double dy = cyw - py;
        int s0, s1;
        row_span(f, pl, res, inv_res, fs, fc, dx0, static_cast<float>(dy), c1 - c0 + 1, s0, s1);
        const int l2 = max(s0 + c0 - 64 * k, 0), h2 = min(s1 + c0 - 64 * k, 63);
        if (l2 > h2) continue;
        word &= (~0ull << l2) & (~0ull >> (63 - h2));
        while (word != 0ull) {
          const int j = w.wx0 + 64 * k + (__ffsll(static_cast<long long>(word)) - 1);
          word &= word - 1ull;
          const double cxw = static_cast<double>(j) * c.resolution + c.resolution / 2.0 + c.xmin;
          const double dx = cxw - px;
          const double bx = cs * dx + sn * dy, by = (-sn) * dx + cs * dy;
          bool in = true;
          for (int kk = 0; kk < static_cast<int>(f.n); ++kk) {
            const int ku = __builtin_amdgcn_readfirstlane(kk);
            in = in & (lane_value(pl.nx, ku) * bx + lane_value(pl.ny, ku) * by <= lane_value(pl.h, ku));
          }
          if (in) return true;
        }
      }
    }
  }
  return false;
}

// ... the same by one lane alone from the grid in memory: for a box that is not inside the window (the reach bound says there
// is none; a wrong answer would be silent, this is only slow)
template <class BV = NoBodies>
__device__ __forceinline__ bool resolve_alone(const CollisionParams& c, const FootprintArgs& f, const PlaneRegs& pl,
                                              const int8_t* __restrict__ grid, double px, double py, double sn, double cs, const Box& b,
                                              BV bv = BV{})
{
  for (int i = b.y0; i <= b.y1; ++i) {
    const double cyw = static_cast<double>(i) * c.resolution + c.resolution / 2.0 + c.ymin;
    const double dy = cyw - py;
    for (int j = b.x0; j <= b.x1; ++j) {
      if constexpr (kWithBodies<BV>) {
        const size_t at = static_cast<size_t>(i) * c.xsize + static_cast<size_t>(j);
        if (grid[at] < f.v_min && !other_body(c, f, pl, bv.v.cover[at], i, j, bv.stamped, bv.px, bv.py, bv.sn, bv.cs)) continue;
      } else {
        if (grid[static_cast<size_t>(i) * c.xsize + static_cast<size_t>(j)] < f.v_min) continue;
      }
      const double cxw = static_cast<double>(j) * c.resolution + c.resolution / 2.0 + c.xmin;
      const double dx = cxw - px;
      const double bx = cs * dx + sn * dy, by = (-sn) * dx + cs * dy;
      bool in = true;
      for (int kk = 0; kk < static_cast<int>(f.n); ++kk) {
        const int ku = __builtin_amdgcn_readfirstlane(kk);
        in = in & (lane_value(pl.nx, ku) * bx + lane_value(pl.ny, ku) * by <= lane_value(pl.h, ku));
      }
      if (in) return true;
    }
  }
  return false;
}

// eea_tick_batch_footprint (FLEET): dwa_control_kernel's FleetTick
struct PlanTick
{
  const int* valid;
  int* follow;
  unsigned* count;
  double* u;
  int* source;
};

// win_reach: the reach in cells the launch reserved a window for (after the costs in dynamic LDS), -1: none
template <bool FLEET, class VIEW>
__global__ __launch_bounds__(kPlanBlock) void footprint_dwa_kernel(const CollisionParams c, const DwaParams d, const FootprintArgs f,
                                                                  const int8_t* __restrict__ grid, const int* __restrict__ d_sq,
                                                                  const double* __restrict__ x0s, const double* __restrict__ vbs,
                                                                  const double* __restrict__ vrefs,
                                                                  const double* __restrict__ xt_refs, unsigned n_ref, double dt_ref,
                                                                  double* __restrict__ u_opt, int* __restrict__ found,
                                                                  const PlanTick ft, int win_reach, const VIEW view)
{
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  double* const s_cost = reinterpret_cast<double*>(smem_raw);
  const unsigned r = blockIdx.x;
  const int lane = threadIdx.x % kWave;
  bool following = false;
  if (FLEET) {
    following = ft.follow[r] != 0;  // (after step 1 of the tick)
    if (ft.valid[r] != 0) {         // workgroup-uniform
      if (threadIdx.x == 0 && ft.source != nullptr) ft.source[r] = following ? 1 : 0;
      return;
    }
    if (following) {
      xt_refs = nullptr;
      vrefs = ft.u;
    }
    u_opt = ft.u;
  }
  const PlaneRegs pl = load_planes(f, lane);
  // (with the layer: the workgroup's robot, the same in every lane, and whether its window holds a body bit)
  typename BodiesOf<VIEW>::type bv{};
  [[maybe_unused]] bool body_in_window = false;  // (never read without the layer)
  if constexpr (std::is_same_v<VIEW, BodyArgs>) bv = load_bodies(view, r);
  const double* const x0 = x0s + 3 * static_cast<size_t>(r);
  const double* const vb = vbs + 3 * static_cast<size_t>(r);
  const unsigned nsamp = d.ns[0] * d.ns[1] * d.ns[2];
  constexpr double kMax = 1.7976931348623157e308;

  // window (dynamic_window.cpp:191-235)
  double lower[3], upper[3], delta[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    lower[a] = fmax(vb[a] - d.acc_lim[a] * d.acc_dt, d.vmin[a]);
    upper[a] = fmin(vb[a] + d.acc_lim[a] * d.acc_dt, d.vmax[a]);
    delta[a] = (d.ns[a] > 1) ? (upper[a] - lower[a]) / static_cast<double>(d.ns[a] - 1) : 0.0;
  }
  const double tf = static_cast<double>(n_ref) * dt_ref;
  const double* const xr = (xt_refs != nullptr) ? xt_refs + 3 * static_cast<size_t>(n_ref) * r : nullptr;
  const double px0 = x0[0], py0 = x0[1], th0 = x0[2];

  // the robot's own reach against the one the launch reserved (a NaN fails the comparison), then the window's bits
  Window w{ nullptr, 0, 0, -1, 0, -1 };
  bool use_window = false;
  if (win_reach >= 0 && d.steps > 0 && isfinite(px0) && isfinite(py0)) {
    const double mx = fmax(fabs(lower[0]), fabs(upper[0])), my = fmax(fabs(lower[1]), fabs(upper[1]));
    const double reach = ceil(static_cast<double>(d.steps) * fabs(d.dt) * sqrt(mx * mx + my * my) / c.resolution) + 1.0;
    use_window = reach <= static_cast<double>(win_reach);
  }
  if (use_window) {  // workgroup-uniform
    const int side = 2 * (win_reach + f.box) + 1;
    w.nw = (side + 63) / 64;
    unsigned long long* const s_bits = reinterpret_cast<unsigned long long*>(smem_raw + sizeof(double) * nsamp);
    w.bits = s_bits;
    // clamped to the grid as doubles before any conversion, as classify clamps a box
    const double fx = floor((px0 - c.xmin) / c.resolution), fy = floor((py0 - c.ymin) / c.resolution);
    const double xlast = static_cast<double>(c.xsize - 1u), ylast = static_cast<double>(c.ysize - 1u);
    const double rw = static_cast<double>(win_reach + f.box);
    if (fx + rw >= 0.0 && fx - rw <= xlast && fy + rw >= 0.0 && fy - rw <= ylast) {
      w.wx0 = static_cast<int>(fmax(fx - rw, 0.0));
      w.wx1 = static_cast<int>(fmin(fx + rw, xlast));
      w.wy0 = static_cast<int>(fmax(fy - rw, 0.0));
      w.wy1 = static_cast<int>(fmin(fy + rw, ylast));
    }
    const int rows = w.wy1 - w.wy0 + 1, cols = w.wx1 - w.wx0 + 1;  // <= side each; <= 0: nothing to stage
    const int n_waves = static_cast<int>(blockDim.x) / kWave, wave = static_cast<int>(threadIdx.x) / kWave;
    if (cols > 0) {
      // word idx = row * nw + k; a wavefront takes kStage words at a time: their loads first, then the ballots
      constexpr int kStage = 4;
      const int total = rows * w.nw;
      for (int first = wave * kStage; first < total; first += n_waves * kStage) {
        bool occ[kStage];
        if constexpr (kWithBodies<decltype(bv)>) {
          // (the layer: the cell's byte and its count, both loads of all kStage words first -- a lane past the window reads
          // the window's first cell and drops it --, then the own-body test where a count is above 0)
          int8_t gv[kStage];
          int nb[kStage], ri[kStage], cj[kStage];
          bool in[kStage];
          const size_t first_at = static_cast<size_t>(w.wy0) * c.xsize + static_cast<size_t>(w.wx0);
#pragma unroll
          for (int u = 0; u < kStage; ++u) {
            const int idx = first + u, row = idx / w.nw, col = 64 * (idx - row * w.nw) + lane;
            in[u] = idx < total && col < cols;
            ri[u] = w.wy0 + row;
            cj[u] = w.wx0 + col;
            const size_t at = in[u] ? static_cast<size_t>(ri[u]) * c.xsize + static_cast<size_t>(cj[u]) : first_at;
            gv[u] = grid[at];
            nb[u] = bv.v.cover[at];
          }
#pragma unroll
          for (int u = 0; u < kStage; ++u) {
            const bool body = in[u] && other_body(c, f, pl, nb[u], ri[u], cj[u], bv.stamped, bv.px, bv.py, bv.sn, bv.cs);
            body_in_window = body_in_window || body;
            occ[u] = in[u] && (gv[u] >= f.v_min || body);
          }
        } else {
#pragma unroll
          for (int u = 0; u < kStage; ++u) {
            const int idx = first + u, row = idx / w.nw, col = 64 * (idx - row * w.nw) + lane;
            occ[u] = idx < total && col < cols &&
                     grid[static_cast<size_t>(w.wy0 + row) * c.xsize + static_cast<size_t>(w.wx0 + col)] >= f.v_min;
          }
        }
#pragma unroll
        for (int u = 0; u < kStage; ++u) {
          const unsigned long long word = __ballot(occ[u]);
          if (lane == 0 && first + u < total) s_bits[first + u] = word;
        }
      }
    }
    if constexpr (kWithBodies<decltype(bv)>) {  // one word per wavefront behind the bit rows (PlanGeometry reserves them)
      unsigned long long* const s_flag = s_bits + static_cast<size_t>(side) * w.nw;
      const bool mine = __any(body_in_window) != 0;
      if (lane == 0) s_flag[wave] = mine ? 1ull : 0ull;
      __syncthreads();
      body_in_window = false;
      for (int k = 0; k < n_waves; ++k) body_in_window = body_in_window || s_flag[k] != 0ull;
    } else {
      __syncthreads();
    }
  }

  for (unsigned base = 0; base < nsamp; base += blockDim.x) {  // wavefront-uniform: resolve_together needs every lane
    const unsigned sidx = base + threadIdx.x;
    const bool live = sidx < nsamp;
    double u0 = 0.0, u1 = 0.0, u2 = 0.0, d0 = 0.0, d1 = 0.0, d2 = 0.0;
    if (live) {
      sample_twist(d, lower, delta, sidx, u0, u1, u2);
      body_displacement<true>(u0, u1, u2, d.dt, d0, d1, d2);
    }
    double x = px0, y = py0, th = th0;
    double cost = 0.0, t = 0.0;
    bool hit = false, done = !live;
    for (unsigned st = 0; st < d.steps; ++st) {
      if (__all(done)) break;  // every sample of the wavefront has hit
      Box b{ 0, -1, 0, -1 };
      int cls = kFree;
      if (!done) {
        advance_pose<true>(x, y, th, d0, d1, d2, true);
        if constexpr (kWithBodies<decltype(bv)>) {
          if (use_window) {  // the filter is the staging flag (a box outside the window -- there is none -- asks the near map)
            cls = classify(c, f, d_sq, x, y, th, b);
            if (cls == kFree && b.x1 >= b.x0) {
              const bool inside = b.x0 >= w.wx0 && b.x1 <= w.wx1 && b.y0 >= w.wy0 && b.y1 <= w.wy1;
              const bool clear = (bv.v.flags & kBodyLayerNoFilter) != 0u ? false : inside ? !body_in_window : nobody_near(c, bv, x, y);
              if (!clear) cls = kAmbiguous;
            }
          } else {
            cls = classify_with(c, f, d_sq, x, y, th, b, bv);
          }
        } else {
          cls = classify(c, f, d_sq, x, y, th, b);
        }
      }
      bool h = cls == kHit;
      if (use_window) {
        if (cls == kAmbiguous) {
          double sn, cs;
          tick_sincos(th, &sn, &cs);
          const bool inside = b.x0 >= w.wx0 && b.x1 <= w.wx1 && b.y0 >= w.wy0 && b.y1 <= w.wy1;
          h = inside ? resolve_window(c, f, pl, w, x, y, sn, cs, b) : resolve_alone(c, f, pl, grid, x, y, sn, cs, b, bv);
        }
      } else {
        h = resolve_together(c, f, pl, grid, cls == kAmbiguous, x, y, th, b, lane, bv) || h;
      }
      if (h) {
        hit = true;
        done = true;
      }
      if (!done && xr != nullptr) {
        const unsigned jj = cast_u32_x86(round(static_cast<double>(n_ref - 1) * t / tf));
        const double ex = xr[3 * jj + 0] - x, ey = xr[3 * jj + 1] - y;
        cost += sqrt(ex * ex + ey * ey);
        cost += fabs(wrap_pi_d(wrap_pi_d(xr[3 * jj + 2]) - th));
        t += d.dt;
      }
    }
    if (hit) {
      cost = kMax;
    } else if (xr == nullptr) {
      // (FLEET: vrefs is the robot's own u, read here by every lane before lane 0 overwrites it behind the barrier)
      const double* const vref = vrefs + 3 * static_cast<size_t>(r);
      const double e0 = vref[0] - u0, e1 = vref[1] - u1, e2 = vref[2] - u2;
      cost = (e0 * e0 + e2 * e2) + e1 * e1;
    }
    if (live) s_cost[sidx] = cost;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double best = kMax;
    unsigned arg = 0;
    for (unsigned sidx = 0; sidx < nsamp; ++sidx) {
      if (s_cost[sidx] < best) {
        best = s_cost[sidx];
        arg = sidx;
      }
    }
    const bool ok = !(fabs(best - kMax) < 1.0e-12);
    double o0 = 0.0, o1 = 0.0, o2 = 0.0;  // u_opt stays zero when nothing beat the initial maximum
    if (best < kMax) sample_twist(d, lower, delta, arg, o0, o1, o2);
    u_opt[3 * static_cast<size_t>(r) + 0] = o0;
    u_opt[3 * static_cast<size_t>(r) + 1] = o1;
    u_opt[3 * static_cast<size_t>(r) + 2] = o2;
    if (FLEET) {
      if (following) {  // the followed twist led into a collision: whatever the window found, control() replans next tick
        ft.follow[r] = 0;
        if (ft.source != nullptr) ft.source[r] = 3;
      } else {          // follow the solution if there is one
        ft.follow[r] = ok ? 1 : 0;
        if (ok) ft.count[r] = 0u;
        if (ft.source != nullptr) ft.source[r] = 2;
      }
    } else {
      found[r] = ok ? 1 : 0;
    }
  }
}

// launch geometry of footprint_dwa_kernel: dwa_control_kernel's block and costs, then the window the limits' reach needs --
// none when costs and window together exceed the LDS, or the reach is not a number of cells
struct PlanGeometry
{
  size_t nsamp, lds;
  unsigned block;
  int win_reach = -1;
  // flag_bytes: what the layer's instance keeps behind the window (a word per wavefront)
  PlanGeometry(const CollisionParams& c, const DwaParams& d, const FootprintArgs& f, size_t flag_bytes = 0)
    : nsamp(static_cast<size_t>(d.ns[0]) * d.ns[1] * d.ns[2]), lds(sizeof(double) * nsamp), block(nsamp <= 64 ? 64 : kPlanBlock)
  {
    const double mx = std::fmax(std::fabs(d.vmin[0]), std::fabs(d.vmax[0])), my = std::fmax(std::fabs(d.vmin[1]), std::fabs(d.vmax[1]));
    const double reach = std::ceil(static_cast<double>(d.steps) * std::fabs(d.dt) * std::sqrt(mx * mx + my * my) / c.resolution) + 1.0;
    if (!(reach >= 0.0 && reach <= 4096.0)) return;
    const size_t side = 2 * (static_cast<size_t>(reach) + static_cast<size_t>(f.box)) + 1;
    const size_t bytes = side * ((side + 63) / 64) * sizeof(unsigned long long) + flag_bytes;
    if (lds + bytes > kLdsLimit) return;
    win_reach = static_cast<int>(reach);
    lds += bytes;
  }
  bool fits() const { return sizeof(double) * nsamp <= kLdsLimit; }  // a larger sample window is refused
};

// One launch in the instance the call takes: launch(NoBodies{}) without a layer, launch(the BodyArgs) with one -- the view is
// the kernel's last argument and its type the kernel's last template argument.  The launch error is taken here, behind it.
template <typename Launch>
hipError_t with_or_without_bodies(const BodyArgs* bodies, Launch launch)
{
  if (bodies != nullptr) launch(*bodies);
  else launch(NoBodies{});
  return hipGetLastError();
}
// ... and what PlanGeometry keeps behind the window by the same choice
size_t flag_bytes(const void* bodies) { return bodies != nullptr ? kBodyFlagBytes : 0; }

// footprint_dwa_kernel in the launch geometry g; ft: the tick's bookkeeping (FLEET), PlanTick{} otherwise
template <bool FLEET>
hipError_t launch_plan_dwa(const PlanGeometry& g, const CollisionParams& c, const DwaParams& d, const FootprintArgs& f,
                           const BodyArgs* bodies, const int8_t* d_grid, const int* d_sq, const double* d_x0, const double* d_vb,
                           const double* d_vref, const double* d_xt_ref, unsigned n_ref, double dt_ref, unsigned P, double* d_u_opt,
                           int* d_found, const PlanTick& ft, hipStream_t s)
{
  return with_or_without_bodies(bodies, [&](const auto& view) {
    hipLaunchKernelGGL((footprint_dwa_kernel<FLEET, std::decay_t<decltype(view)>>), dim3(P), dim3(g.block), g.lds, s, c, d, f, d_grid,
                       d_sq, d_x0, d_vb, d_vref, d_xt_ref, n_ref, dt_ref, d_u_opt, d_found, ft, g.win_reach, view);
  });
}
}  // namespace

hipError_t launch_footprint_validate(const CollisionParams& c, const FootprintArgs& f, const BodyArgs* bodies, const int8_t* d_grid,
                                     const int* d_sq, const double* d_x0, const double* d_u, double dt, unsigned steps, unsigned P,
                                     int* d_valid, hipStream_t s)
{
  if (P == 0) return hipSuccess;
  const dim3 blocks(static_cast<unsigned>((static_cast<size_t>(P) + kBlock - 1) / kBlock));
  return with_or_without_bodies(bodies, [&](const auto& view) {
    hipLaunchKernelGGL(footprint_validate_kernel<std::decay_t<decltype(view)>>, blocks, dim3(kBlock), 0, s, c, f, d_grid, d_sq, d_x0,
                       d_u, dt, steps, P, d_valid, view);
  });
}

hipError_t launch_footprint_dwa(const CollisionParams& c, const DwaParams& d, const FootprintArgs& f, const BodyArgs* bodies,
                                const int8_t* d_grid, const int* d_sq, const double* d_x0, const double* d_vb, const double* d_vref,
                                const double* d_xt_ref, unsigned n_ref, double dt_ref, unsigned P, double* d_u_opt, int* d_found,
                                hipStream_t s)
{
  if (P == 0) return hipSuccess;
  const PlanGeometry g(c, d, f, flag_bytes(bodies));
  if (!g.fits()) return hipErrorInvalidValue;
  return launch_plan_dwa<false>(g, c, d, f, bodies, d_grid, d_sq, d_x0, d_vb, d_vref, d_xt_ref, n_ref, dt_ref, P, d_u_opt, d_found,
                                PlanTick{}, s);
}

// steps 3 and 4 of a fleet tick with the footprint: validate_control of every robot's twist, then the dynamic window of the
// robots whose twist was rejected.  With a layer, robot r of the tick is robot r of the layer
hipError_t launch_footprint_validate_and_dwa_fleet(const CollisionParams& c, const DwaParams& d, const FootprintArgs& f,
                                                   const BodyView* bodies, const int8_t* d_grid, const int* d_sq, const double* d_x0,
                                                   const double* d_vb, const double* d_traj, unsigned n_ref, double dt_ref,
                                                   double val_dt, unsigned val_steps, int* d_valid, int* d_follow, unsigned* d_count,
                                                   double* d_u, int* d_source, unsigned P, hipStream_t s)
{
  if (P == 0) return hipSuccess;
  const PlanGeometry g(c, d, f, flag_bytes(bodies));
  if (!g.fits()) return hipErrorInvalidValue;
  const BodyArgs own{ bodies != nullptr ? *bodies : BodyView{}, nullptr, 1 };
  const BodyArgs* const a = bodies != nullptr ? &own : nullptr;
  const hipError_t e = launch_footprint_validate(c, f, a, d_grid, d_sq, d_x0, d_u, val_dt, val_steps, P, d_valid, s);
  if (e != hipSuccess) return e;
  return launch_plan_dwa<true>(g, c, d, f, a, d_grid, d_sq, d_x0, d_vb, nullptr, d_traj, n_ref, dt_ref, P, nullptr, nullptr,
                               PlanTick{ d_valid, d_follow, d_count, d_u, d_source }, s);
}
}  // namespace eea
