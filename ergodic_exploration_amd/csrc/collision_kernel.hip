// Batched collision lookups for gfx950: Collision::collisionCheck (reference
// collision.cpp:126-243) on a GridMap (grid.cpp:96-184) and validate_control
// (numerics.hpp:273-330).  Integer work, one pose per lane; results are bit-exact with the
// reference's x86-64 build, including the wrap of negative world coordinates in world2Grid.
//
// Large batches go through an inflated map: the boolean result of the ring search does not depend on
// the visiting order (the search only stops at a hit), so it equals "some occupied cell lies at one
// of the offsets the Bresenham rings r_bnd..r_max visit and within r_col" -- a dilation of the
// occupied cells by a fixed offset set.  That set is enumerated on the host by the same ring walk,
// the occupied cells scatter a 1 to every centre that would see them, and a collision check becomes
// one byte lookup (a robot centred inside a small obstacle still reports no collision: cells closer
// than r_bnd are not in the set, as in the reference).
#include <array>
#include <cstdint>
#include <cstdlib>
#include <mutex>
#include <type_traits>
#include <vector>

#include "../../include/ergodic_amd.h"
#include "common.hpp"
#include "grid_cell.hpp"      // cast_u32_x86, world_to_grid (grid.cpp:143-159), occupied
#include "hit_map_table.hpp"  // ring_offsets, HitMapTable: the host-side policy of the inflated map
#include "device_tables.hpp"  // DeviceTables: ... and of the offset lists kept per device
#include "grid_buffers.hpp"   // upload_block, acquire_map_buffer, launch_then_free: the effects of both
#include "fleet_spans.hpp"    // FleetSpan: the row spans of the fleet layer's offset set
#include "twist_step.hpp"     // wrap_pi_d, tick_sincos, body_displacement, advance_pose, sample_twist: the twist step

namespace eea
{
namespace
{
struct RingState
{
  int cx, cy, sqrd_obs;
};

// collision.cpp:216-243 (+ grid.cpp:96-100, 109-117, 177-184)
__device__ __forceinline__ bool check_cell(const CollisionParams& c, const int8_t* __restrict__ grid,
                                           RingState& st, unsigned cj, unsigned ci)
{
  if ((ci <= c.ysize - 1u) && (cj <= c.xsize - 1u)) {
    if (occupied(c, grid[ci * c.xsize + cj])) {
      const unsigned ddx = static_cast<unsigned>(st.cx) - cj, ddy = static_cast<unsigned>(st.cy) - ci;
      const int sq = static_cast<int>(ddx * ddx + ddy * ddy);
      if (sq < st.sqrd_obs || st.sqrd_obs == -1) st.sqrd_obs = sq;
      if (sq <= c.r_col * c.r_col) return true;
    }
  }
  return false;
}

// collision.cpp:166-214
__device__ __forceinline__ bool bresenham_circle(const CollisionParams& c,
                                                 const int8_t* __restrict__ grid, RingState& st, int r)
{
  int x = -r, y = 0, err = 2 - 2 * r;
  while (x < 0) {
    if (check_cell(c, grid, st, static_cast<unsigned>(st.cx - x), static_cast<unsigned>(st.cy + y))) return true;
    if (check_cell(c, grid, st, static_cast<unsigned>(st.cx - y), static_cast<unsigned>(st.cy - x))) return true;
    if (check_cell(c, grid, st, static_cast<unsigned>(st.cx + x), static_cast<unsigned>(st.cy - y))) return true;
    if (check_cell(c, grid, st, static_cast<unsigned>(st.cx + y), static_cast<unsigned>(st.cy + x))) return true;
    r = err;
    if (r <= y) {
      y++;
      err += 2 * y + 1;
    }
    if (r > x || err > y) {
      x++;
      err += 2 * x + 1;
    }
  }
  return false;
}

// collision.cpp:126-164 with grid.cpp:143-159
__device__ __forceinline__ bool collision_check(const CollisionParams& c,
                                                const int8_t* __restrict__ grid, double px, double py)
{
  unsigned j, i;
  world_to_grid(c, px, py, j, i);
  RingState st;
  st.cx = static_cast<int>(j);
  st.cy = static_cast<int>(i);
  st.sqrd_obs = -1;
  for (int r = c.r_bnd; r <= c.r_max; ++r) {
    if (bresenham_circle(c, grid, st, r)) return true;
  }
  return false;
}

// ---- inflated map ----------------------------------------------------------------------------
// hit map over the centres [-R, xsize + R) x [-R, ysize + R), R = r_col, row-major
struct HitMap
{
  const uint8_t* cells = nullptr;  // (all zero: the ring-search instances take a map they never read)
  int R = 0, w = 0, h = 0;         // w = xsize + 2R, h = ysize + 2R
  uint8_t stamp = 0;               // a cell is marked iff it holds this build's stamp (older stamps are stale, no clear)
};

// grid cell of a world point as collisionCheck derives it (grid.cpp:143-159), as signed ints
__device__ __forceinline__ void centre_of(const CollisionParams& c, double px, double py, int& cx, int& cy)
{
  unsigned j, i;
  world_to_grid(c, px, py, j, i);
  cx = static_cast<int>(j);
  cy = static_cast<int>(i);
}

__device__ __forceinline__ bool hit_lookup(const HitMap& m, int cx, int cy)
{
  const int hx = cx + m.R, hy = cy + m.R;
  // centres further than R outside the grid see no cell at all (the unsigned cell indices of
  // collision.cpp:216-243 fall outside gridBounds)
  if (hx < 0 || hy < 0 || hx >= m.w || hy >= m.h) return false;
  return m.cells[static_cast<size_t>(hy) * m.w + hx] == m.stamp;
}

// ---- fleet layer (fleet_layer_kernel.hip): the other robots' bodies ------------------------------------
// The robot a pose belongs to: its cell at the layer's last update, x = kFleetNotStamped when it is no obstacle (or the pose is
// nobody's)
struct FleetSelf
{
  int x = kFleetNotStamped, y = kFleetNotStamped;
};
__device__ __forceinline__ FleetSelf fleet_self(const FleetView& f, int robot)
{
  FleetSelf own;
  if (static_cast<unsigned>(robot) < f.B) {  // (-1: none)
    own.x = f.cell[2 * static_cast<size_t>(robot)];
    own.y = f.cell[2 * static_cast<size_t>(robot) + 1];
  }
  return own;
}

// "the pose centred at (cx, cy) collides with a robot other than its own": count[c] robots reach c through F; the pose's own
// robot is one of them iff it was stamped and (c - own) in F (one or two spans per row: fleet_spans.hpp)
__device__ __forceinline__ bool fleet_lookup(const FleetView& f, const FleetSelf& own, int cx, int cy)
{
  const int hx = cx + f.R, hy = cy + f.R;
  if (hx < 0 || hy < 0 || hx >= f.w || hy >= f.h) return false;  // centres outside the map see nothing: F lies within R
  int n = f.count[static_cast<size_t>(hy) * f.w + hx];
  if (n > 0 && own.x != kFleetNotStamped) {
    // (cx, cy is inside the map and own inside the grid: the differences cannot overflow)
    const int dx = cx - own.x, dy = cy - own.y;
    if (dy >= -f.R && dy <= f.R) {
      for (int k = f.row_start[dy + f.R]; k < f.row_start[dy + f.R + 1]; ++k) {
        if (f.spans[k].x0 <= dx && dx <= f.spans[k].x1) {
          n -= 1;
          break;
        }
      }
    }
  }
  return n > 0;
}
struct NoFleetLayer
{
};

// occupied cells mark every centre that reaches them through one of the ring offsets
__global__ __launch_bounds__(kBlock) void inflate_kernel(const CollisionParams c, const int8_t* __restrict__ grid,
                                                         const short2* __restrict__ offsets, int n_off,
                                                         uint8_t* __restrict__ cells, int R, int w,
                                                         uint8_t stamp)
{
  // Occupied cells are few and the ring has hundreds of offsets: a lane that walked its own cell's ring alone made the
  // launch as long as that walk (27 us on the 240 x 120 demo map, profiles/r05_tick_kernels.txt).  The block first lists
  // its occupied cells, then ALL its threads walk the ring of each listed cell together.
  __shared__ unsigned s_list[kBlock];
  __shared__ unsigned s_n;
  if (threadIdx.x == 0) s_n = 0u;
  __syncthreads();
  const size_t q = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  const size_t n = static_cast<size_t>(c.xsize) * c.ysize;
  if (q < n && occupied(c, grid[q])) s_list[atomicAdd(&s_n, 1u)] = threadIdx.x;
  __syncthreads();
  const unsigned cnt = s_n;
  for (unsigned k = 0; k < cnt; ++k) {
    const size_t qq = static_cast<size_t>(blockIdx.x) * kBlock + s_list[k];
    const int i = static_cast<int>(qq / c.xsize), j = static_cast<int>(qq - static_cast<size_t>(i) * c.xsize);
    for (int o = threadIdx.x; o < n_off; o += kBlock) {
      const short2 d = offsets[o];  // cell = centre + d
      cells[static_cast<size_t>(i - d.y + R) * w + (j - d.x + R)] = stamp;  // same value from every writer
    }
  }
}

__global__ __launch_bounds__(kBlock) void collision_check_map_kernel(const CollisionParams c, const HitMap m,
                                                                     const double* __restrict__ pose,
                                                                     unsigned P, int* __restrict__ hit)
{
  const unsigned q = blockIdx.x * kBlock + threadIdx.x;
  if (q >= P) return;
  int cx, cy;
  centre_of(c, pose[3 * static_cast<size_t>(q)], pose[3 * static_cast<size_t>(q) + 1], cx, cy);
  hit[q] = hit_lookup(m, cx, cy) ? 1 : 0;
}

__global__ __launch_bounds__(kBlock) void collision_check_kernel(const CollisionParams c,
                                                                 const int8_t* __restrict__ grid,
                                                                 const double* __restrict__ pose,
                                                                 unsigned P, int* __restrict__ hit)
{
  const unsigned q = blockIdx.x * kBlock + threadIdx.x;
  if (q >= P) return;
  hit[q] = collision_check(c, grid, pose[3 * static_cast<size_t>(q)], pose[3 * static_cast<size_t>(q) + 1]) ? 1 : 0;
}

// one collision test through the inflated map (MAP) or by the ring search
template <bool MAP>
__device__ __forceinline__ bool pose_collides(const CollisionParams& c, const int8_t* __restrict__ grid,
                                              const HitMap& m, double px, double py)
{
  if (MAP) {
    int cx, cy;
    centre_of(c, px, py, cx, cy);
    return hit_lookup(m, cx, cy);
  }
  return collision_check(c, grid, px, py);
}

// ... OR a collision with another robot's body when Layer is the FleetView of a fleet layer (NoFleetLayer: the static
// verdict alone, the code of the instances without a layer)
template <bool LAYER>
using LayerArg = std::conditional_t<LAYER, FleetView, NoFleetLayer>;  // (the last kernel argument; empty without a layer)
template <typename Layer>
constexpr bool kWithLayer = std::is_same<Layer, FleetView>::value;
template <bool MAP, typename Layer>
__device__ __forceinline__ bool pose_collides(const CollisionParams& c, const int8_t* __restrict__ grid, const HitMap& m,
                                              const Layer& layer, const FleetSelf& own, double px, double py)
{
  if constexpr (kWithLayer<Layer>) {
    int cx, cy;
    centre_of(c, px, py, cx, cy);
    const bool hit = MAP ? hit_lookup(m, cx, cy) : collision_check(c, grid, px, py);
    return hit || fleet_lookup(layer, own, cx, cy);
  } else {
    return pose_collides<MAP>(c, grid, m, px, py);
  }
}

// numerics.hpp:273-330; LAYER: with a fleet layer, pose q is robot q's
template <bool MAP, bool LAYER = false>
__global__ __launch_bounds__(kBlock) void validate_control_kernel(const CollisionParams c, const HitMap m,
                                                                  const int8_t* __restrict__ grid,
                                                                  const double* __restrict__ x0,
                                                                  const double* __restrict__ u,
                                                                  double dt, unsigned steps, unsigned P,
                                                                  int* __restrict__ valid, const LayerArg<LAYER> layer)
{
  const unsigned q = blockIdx.x * kBlock + threadIdx.x;
  if (q >= P) return;
  double x = x0[3 * static_cast<size_t>(q)], y = x0[3 * static_cast<size_t>(q) + 1],
         th = x0[3 * static_cast<size_t>(q) + 2];
  const double u0 = u[3 * static_cast<size_t>(q)], u1 = u[3 * static_cast<size_t>(q) + 1],
               u2 = u[3 * static_cast<size_t>(q) + 2];
  FleetSelf own;
  if constexpr (LAYER) own = fleet_self(layer, static_cast<int>(q));
  double d0, d1, d2;
  body_displacement<true>(u0, u1, u2, dt, d0, d1, d2);
  int ok = 1;
  for (unsigned i = 0; i < steps; ++i) {
    advance_pose<true>(x, y, th, d0, d1, d2, true);
    if (pose_collides<MAP>(c, grid, m, layer, own, x, y)) {
      ok = 0;
      break;
    }
  }
  valid[q] = ok;
}

// collisionCheck of P poses with a fleet layer: the static verdict (grid == null: none) OR another robot's body
template <bool MAP>
__global__ __launch_bounds__(kBlock) void fleet_collision_check_kernel(const CollisionParams c, const HitMap m, const FleetView f,
                                                                       const int8_t* __restrict__ grid,
                                                                       const double* __restrict__ pose,
                                                                       const int* __restrict__ self, unsigned P,
                                                                       int* __restrict__ hit)
{
  const unsigned q = blockIdx.x * kBlock + threadIdx.x;
  if (q >= P) return;
  const double px = pose[3 * static_cast<size_t>(q)], py = pose[3 * static_cast<size_t>(q) + 1];
  const FleetSelf own = fleet_self(f, self != nullptr ? self[q] : -1);
  bool h;
  if (grid != nullptr) {
    h = pose_collides<MAP>(c, grid, m, f, own, px, py);
  } else {
    int cx, cy;
    centre_of(c, px, py, cx, cy);
    h = fleet_lookup(f, own, cx, cy);
  }
  hit[q] = h ? 1 : 0;
}
// DynamicWindow::control (dynamic_window.cpp:92-286): one workgroup per robot, one lane per
// velocity sample; lane 0 then takes the first strict minimum in the reference's loop order.
constexpr int kDwaBlock = 128;
// eea_tick_batch (FLEET): the robots of a fleet tick.  A robot whose twist validate_control accepted does nothing here
// (its source is recorded); the others run the dynamic window in THEIR mode -- a follower towards its own twist
// (exploration.hpp:243-251), the rest along their optTraj (:254-277) -- and lane 0 updates u, follow_dwa and i.
struct FleetTick
{
  const int* valid;
  int* follow;
  unsigned* count;
  double* u;
  int* source;
};
// LAYER: with a fleet layer; robot r of the launch is robot r of the layer
template <bool MAP, bool FLEET, bool LAYER = false>
__global__ __launch_bounds__(kDwaBlock) void dwa_control_kernel(const CollisionParams c, const DwaParams d,
                                                               const HitMap m,
                                                               const int8_t* __restrict__ grid,
                                                               const double* __restrict__ x0s,
                                                               const double* __restrict__ vbs,
                                                               const double* __restrict__ vrefs,
                                                               const double* __restrict__ xt_refs,
                                                               unsigned n_ref, double dt_ref,
                                                               double* __restrict__ u_opt,
                                                               int* __restrict__ found, const FleetTick ft,
                                                               const LayerArg<LAYER> layer)
{
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  double* const s_cost = reinterpret_cast<double*>(smem_raw);
  const unsigned r = blockIdx.x;
  FleetSelf own;
  if constexpr (LAYER) own = fleet_self(layer, static_cast<int>(r));
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
  const double* const x0 = x0s + 3 * static_cast<size_t>(r);
  const double* const vb = vbs + 3 * static_cast<size_t>(r);
  const unsigned nsamp = d.ns[0] * d.ns[1] * d.ns[2];
  constexpr double kMax = 1.7976931348623157e308;

  // window (dynamic_window.cpp:191-235)
  double lower[3], delta[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    lower[a] = fmax(vb[a] - d.acc_lim[a] * d.acc_dt, d.vmin[a]);
    const double upper = fmin(vb[a] + d.acc_lim[a] * d.acc_dt, d.vmax[a]);
    delta[a] = (d.ns[a] > 1) ? (upper - lower[a]) / static_cast<double>(d.ns[a] - 1) : 0.0;
  }
  const double tf = static_cast<double>(n_ref) * dt_ref;
  const double* const xr = (xt_refs != nullptr) ? xt_refs + 3 * static_cast<size_t>(n_ref) * r : nullptr;

  for (unsigned sidx = threadIdx.x; sidx < nsamp; sidx += blockDim.x) {
    double u0, u1, u2, d0, d1, d2;
    sample_twist(d, lower, delta, sidx, u0, u1, u2);
    body_displacement<true>(u0, u1, u2, d.dt, d0, d1, d2);
    double x = x0[0], y = x0[1], th = x0[2];
    double cost = 0.0, t = 0.0;
    bool hit = false;
    for (unsigned st = 0; st < d.steps; ++st) {
      advance_pose<true>(x, y, th, d0, d1, d2, true);
      if (pose_collides<MAP>(c, grid, m, layer, own, x, y)) {
        hit = true;
        break;
      }
      if (xr != nullptr) {
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
    s_cost[sidx] = cost;
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

// step 1 of the fleet tick (exploration.hpp:223-228): a follower counts a step and replans after dwa_steps of them
__global__ __launch_bounds__(256) void tick_begin_kernel(int* __restrict__ follow, unsigned* __restrict__ count,
                                                         int* __restrict__ skip, unsigned dwa_steps, unsigned P)
{
  const unsigned r = blockIdx.x * 256 + threadIdx.x;
  if (r >= P) return;
  int f = follow[r];
  if (f != 0) {
    const unsigned i = count[r] + 1u;
    count[r] = i;
    f = (i != dwa_steps) ? 1 : 0;
    follow[r] = f;
  }
  skip[r] = f;
}
}  // namespace

namespace
{
// The offset list depends on three small integers only: built once per (device, radii) and kept until
// release_collision_caches (a few KB), so that building a map needs no host synchronisation.
using RingKey = std::array<int, 3>;  // r_bnd, r_col, r_max
struct RingTable
{
  const short2* offsets = nullptr;
  int n = 0;
};
std::mutex g_offsets_mutex;
DeviceTables<RingKey, RingTable> g_offsets;

hipError_t device_offsets(int device, const CollisionParams& c, RingTable& t)
{
  std::lock_guard<std::mutex> lock(g_offsets_mutex);
  const RingKey key{ c.r_bnd, c.r_col, c.r_max };
  if (const auto* hit = g_offsets.find(device, key)) {
    t = hit->view;
    return hipSuccess;
  }
  const std::vector<short2> off = ring_offsets(c.r_bnd, c.r_col, c.r_max);
  void* block = nullptr;
  const hipError_t e = upload_block(off.data(), off.size() * sizeof(short2), nullptr, 0, &block);
  if (e != hipSuccess) return e;
  t = g_offsets.insert(device, key, block, RingTable{ static_cast<const short2*>(block), static_cast<int>(off.size()) }).view;
  return hipSuccess;
}

// the map buffers kept between calls: the policy is HitMapTable's (hit_map_table.hpp), the effects are acquire_map_buffer's
std::mutex g_maps_mutex;
HitMapTable g_maps;

// epoch != 0: the caller vouches that (d_grid, epoch) names one content -- the inflated map of the last build on this
// stream is reused when it was built from the same (grid, epoch, parameters).  async_cells: a stream-ordered allocation (only
// when the buffer table is full) that the caller frees behind the map's readers, whatever is returned
hipError_t build_hit_map(const CollisionParams& c, const int8_t* d_grid, hipStream_t s, unsigned long long epoch, HitMap& map,
                         void*& async_cells)
{
  if (c.r_col < 0 || c.r_col > 8192 || c.r_max < c.r_bnd) return hipErrorInvalidValue;
  int device = 0;
  RingTable ring;
  hipError_t e = hipGetDevice(&device);
  if (e == hipSuccess) e = device_offsets(device, c, ring);
  if (e != hipSuccess) return e;
  const int R = c.r_col;
  const int w = static_cast<int>(c.xsize) + 2 * R, h = static_cast<int>(c.ysize) + 2 * R;

  std::lock_guard<std::mutex> lock(g_maps_mutex);  // (held through the launch and built())
  MapBuffer b;
  e = acquire_map_buffer(g_maps, device, s, static_cast<size_t>(w) * h, d_grid, epoch, c, b);
  async_cells = b.async_cells;
  if (e != hipSuccess) return e;
  const HitMapPlan& p = b.plan;
  if (p.clear) {
    e = hipMemsetAsync(b.cells, 0, p.cap, s);
    if (e != hipSuccess) return e;
  }
  if (!p.reuse) {
    if (ring.n > 0) {
      const size_t n = static_cast<size_t>(c.xsize) * c.ysize;
      hipLaunchKernelGGL(inflate_kernel, dim3(static_cast<unsigned>((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, c,
                         d_grid, ring.offsets, ring.n, static_cast<uint8_t*>(b.cells), R, w, static_cast<uint8_t>(p.stamp));
      e = hipGetLastError();
      if (e != hipSuccess) return e;
    }
    if (p.slot >= 0) g_maps.built(p, d_grid, epoch, c);
  }
  map = HitMap{ static_cast<const uint8_t*>(b.cells), R, w, h, static_cast<uint8_t>(p.stamp) };
  return hipSuccess;
}

// Inflated map or ring search?  A ring search is a chain of ~200 dependent byte loads per pose
// (~40 us on MI355X, and the steps of one rollout follow each other in one lane), the map costs a
// fixed ~25 us of stream operations plus a pass over the grid (measured: profiles/r01_tick_kernels.txt).
// EEA_OPT_COLLISION_IMPL = 1 / 2 forces one of them.
bool use_hit_map(size_t poses, unsigned sequential_steps, const CollisionParams& c)
{
  const int forced = option(EEA_OPT_COLLISION_IMPL);
  if (forced != 0) return forced == 2;
  if (poses >= 4096) return true;
  const double cells = static_cast<double>(c.xsize) * c.ysize;
  const double t_map_us = 25.0 + 2.0e-6 * cells, t_ring_us = 40.0 * (sequential_steps ? sequential_steps : 1u);
  return t_map_us < t_ring_us;
}

// One call's collision lookups: launch(map, std::true_type) behind a build of the inflated map when the cost model takes it
// for `poses` lookups in chains of `sequential_steps`, launch(HitMap{}, std::false_type) -- the ring search -- otherwise.
// `launch` enqueues the caller's kernels on s; the launch error is taken here, once, behind them.
template <typename Launch>
hipError_t with_map_or_ring(size_t poses, unsigned sequential_steps, const CollisionParams& c, const int8_t* d_grid,
                            unsigned long long epoch, hipStream_t s, Launch launch)
{
  if (!use_hit_map(poses, sequential_steps, c)) {
    launch(HitMap{}, std::false_type{});
    return hipGetLastError();
  }
  HitMap map;
  void* async_cells = nullptr;
  const hipError_t built = build_hit_map(c, d_grid, s, epoch, map, async_cells);
  return launch_then_free(built, async_cells, s, [&] { launch(map, std::true_type{}); });
}

// launch geometry of dwa_control_kernel: one lane per velocity sample -- a single wavefront when the window has at most 64
// samples -- and one cost per sample in LDS
struct DwaGeometry
{
  size_t nsamp, lds;
  unsigned block;
  explicit DwaGeometry(const DwaParams& d)
    : nsamp(static_cast<size_t>(d.ns[0]) * d.ns[1] * d.ns[2]), lds(sizeof(double) * nsamp), block(nsamp <= 64 ? 64 : kDwaBlock)
  {
  }
  bool fits() const { return lds <= 64 * 1024; }  // a larger window is refused
};
}  // namespace

void release_collision_caches()
{
  const CurrentDeviceGuard guard;
  {
    std::lock_guard<std::mutex> lock(g_maps_mutex);
    g_maps.release(free_on_device);
  }
  std::lock_guard<std::mutex> lock(g_offsets_mutex);
  g_offsets.release(free_on_device);
}

hipError_t launch_dwa_control(const CollisionParams& c, const DwaParams& d, const int8_t* d_grid,
                              const double* d_x0, const double* d_vb, const double* d_vref,
                              const double* d_xt_ref, unsigned n_ref, double dt_ref, unsigned P,
                              double* d_u_opt, int* d_found, hipStream_t s)
{
  if (P == 0) return hipSuccess;
  const DwaGeometry g(d);
  if (!g.fits()) return hipErrorInvalidValue;
  return with_map_or_ring(static_cast<size_t>(P) * g.nsamp * d.steps, d.steps, c, d_grid, 0, s, [&](const HitMap& m, auto map) {
    hipLaunchKernelGGL((dwa_control_kernel<decltype(map)::value, false>), dim3(P), dim3(g.block), g.lds, s, c, d, m, d_grid, d_x0,
                       d_vb, d_vref, d_xt_ref, n_ref, dt_ref, d_u_opt, d_found, FleetTick{}, NoFleetLayer{});
  });
}

hipError_t launch_tick_begin(int* d_follow, unsigned* d_count, int* d_skip, unsigned dwa_steps, unsigned P, hipStream_t s)
{
  if (P == 0) return hipSuccess;
  hipLaunchKernelGGL(tick_begin_kernel, dim3((P + 255) / 256), dim3(256), 0, s, d_follow, d_count, d_skip, dwa_steps, P);
  return hipGetLastError();
}

// Steps 3 and 4 of a fleet tick: validate_control of every robot's twist, then the dynamic window of the robots whose twist
// was rejected (one workgroup per robot as above; robots with a valid twist leave at once).  ONE inflated map serves both
// launches (and, with grid_epoch != 0, the ticks that follow on an unchanged grid).  The cost model takes every robot as
// one that searches (the worst case: the inflated map pays for itself at a fraction of that).
// layer: null, or the fleet layer in every collision test of both launches (eea_tick_batch_fleet)
hipError_t launch_validate_and_dwa_fleet(const CollisionParams& c, const DwaParams& d, const FleetView* layer, const int8_t* d_grid,
                                         unsigned long long grid_epoch, const double* d_x0, const double* d_vb,
                                         const double* d_traj, unsigned n_ref, double dt_ref, double val_dt, unsigned val_steps,
                                         int* d_valid, int* d_follow, unsigned* d_count, double* d_u, int* d_source, unsigned P,
                                         hipStream_t s)
{
  if (P == 0) return hipSuccess;
  const DwaGeometry g(d);
  if (!g.fits()) return hipErrorInvalidValue;
  const FleetTick ft{ d_valid, d_follow, d_count, d_u, d_source };
  // both launches in the instance <MAP, LAYER>; view: the kernels' last argument (LayerArg<LAYER>)
  const auto launch = [&](const HitMap& m, auto map, auto with_layer, const auto& view) {
    constexpr bool MAP = decltype(map)::value, LAYER = decltype(with_layer)::value;
    hipLaunchKernelGGL((validate_control_kernel<MAP, LAYER>), dim3((P + kBlock - 1) / kBlock), dim3(kBlock), 0, s, c, m, d_grid, d_x0,
                       d_u, val_dt, val_steps, P, d_valid, view);
    hipLaunchKernelGGL((dwa_control_kernel<MAP, true, LAYER>), dim3(P), dim3(g.block), g.lds, s, c, d, m, d_grid, d_x0, d_vb,
                       static_cast<const double*>(nullptr), d_traj, n_ref, dt_ref, static_cast<double*>(nullptr),
                       static_cast<int*>(nullptr), ft, view);
  };
  return with_map_or_ring(static_cast<size_t>(P) * (val_steps + g.nsamp * d.steps), d.steps, c, d_grid, grid_epoch, s,
                          [&](const HitMap& m, auto map) {
    if (layer != nullptr) launch(m, map, std::true_type{}, *layer);
    else launch(m, map, std::false_type{}, NoFleetLayer{});
  });
}

hipError_t launch_fleet_collision_check(const CollisionParams& c, const FleetView& v, const int8_t* d_grid, const double* d_pose,
                                        const int* d_self, unsigned P, int* d_hit, hipStream_t s)
{
  if (P == 0) return hipSuccess;
  const dim3 grid((P + kBlock - 1) / kBlock);
  if (d_grid == nullptr) {  // robots only: no static part, no inflated map
    hipLaunchKernelGGL(fleet_collision_check_kernel<false>, grid, dim3(kBlock), 0, s, c, HitMap{}, v, d_grid, d_pose, d_self, P,
                       d_hit);
    return hipGetLastError();
  }
  return with_map_or_ring(P, 1, c, d_grid, 0, s, [&](const HitMap& m, auto map) {
    hipLaunchKernelGGL(fleet_collision_check_kernel<decltype(map)::value>, grid, dim3(kBlock), 0, s, c, m, v, d_grid, d_pose, d_self,
                       P, d_hit);
  });
}

hipError_t launch_collision_check(const CollisionParams& c, const int8_t* d_grid,
                                  const double* d_pose, unsigned P, int* d_hit, hipStream_t s)
{
  if (P == 0) return hipSuccess;
  const dim3 grid((P + kBlock - 1) / kBlock);
  return with_map_or_ring(P, 1, c, d_grid, 0, s, [&](const HitMap& m, auto map) {
    if constexpr (decltype(map)::value) {
      hipLaunchKernelGGL(collision_check_map_kernel, grid, dim3(kBlock), 0, s, c, m, d_pose, P, d_hit);
    } else {
      hipLaunchKernelGGL(collision_check_kernel, grid, dim3(kBlock), 0, s, c, d_grid, d_pose, P, d_hit);
    }
  });
}

// integrate_twist (numerics.hpp:273-297) for P poses: x + Rot(theta) dq_b, the heading NOT wrapped (the reference's callers
// normalise it: validate_control :325, the nodes' motion updates).  One thread per pose; this translation unit is compiled
// without FMA contraction, the sums in the reference's order.
__global__ __launch_bounds__(kBlock) void integrate_twist_kernel(const double* __restrict__ x0, const double* __restrict__ u, double dt,
                                                                 unsigned P, double* __restrict__ out, int wrap)
{
  const unsigned q = blockIdx.x * kBlock + threadIdx.x;
  if (q >= P) return;
  double x = x0[3 * static_cast<size_t>(q)], y = x0[3 * static_cast<size_t>(q) + 1], th = x0[3 * static_cast<size_t>(q) + 2];
  const double u0 = u[3 * static_cast<size_t>(q)], u1 = u[3 * static_cast<size_t>(q) + 1], u2 = u[3 * static_cast<size_t>(q) + 2];
  // <false>: the device library's sincos -- one call per robot and tick, kept closest to libm
  double d0, d1, d2;
  body_displacement<false>(u0, u1, u2, dt, d0, d1, d2);
  advance_pose<false>(x, y, th, d0, d1, d2, wrap != 0);
  out[3 * static_cast<size_t>(q)] = x;
  out[3 * static_cast<size_t>(q) + 1] = y;
  out[3 * static_cast<size_t>(q) + 2] = th;
}

hipError_t launch_integrate_twist(const double* d_x0, const double* d_u, double dt, unsigned P, double* d_out, bool wrap, hipStream_t s)
{
  if (P == 0) return hipSuccess;
  hipLaunchKernelGGL(integrate_twist_kernel, dim3((P + kBlock - 1) / kBlock), dim3(kBlock), 0, s, d_x0, d_u, dt, P, d_out, wrap ? 1 : 0);
  return hipGetLastError();
}

hipError_t launch_validate_control(const CollisionParams& c, const int8_t* d_grid,
                                   const double* d_x0, const double* d_u, double dt, unsigned steps,
                                   unsigned P, int* d_valid, hipStream_t s)
{
  if (P == 0) return hipSuccess;
  return with_map_or_ring(static_cast<size_t>(P) * steps, steps, c, d_grid, 0, s, [&](const HitMap& m, auto map) {
    hipLaunchKernelGGL(validate_control_kernel<decltype(map)::value>, dim3((P + kBlock - 1) / kBlock), dim3(kBlock), 0, s, c, m,
                       d_grid, d_x0, d_u, dt, steps, P, d_valid, NoFleetLayer{});
  });
}
}  // namespace eea
