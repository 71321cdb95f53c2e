// Clearance queries for gfx950: Collision::minDistance and Collision::minDirection (reference collision.cpp:65-124) of a
// batch of poses, or of the centre of every grid cell, on a GridMap.  Integer work up to the last two lines; bit-exact with
// the reference's x86-64 build (this translation unit is compiled without FMA contraction).
//
// The reference's search (collision.cpp:148-243) walks the Bresenham rings r_bnd..r_max, keeps the occupied cell of the
// smallest squared distance -- by a strict <, so the FIRST one visited among equals -- and stops with "crash" at the first
// cell within r_col.  Order-free form: enumerate the walk once, in visit order with duplicates, as offsets d_0..d_{n-1}
// (hit_map_table.hpp: clearance_walk); an occupied in-grid cell reached through offset k has the key (|d_k|^2, k), and the
// answer of a centre is its smallest key.  No key: none.  |d|^2 <= r_col^2: crash -- the search stopped at SOME cell
// within r_col, and every output of a crash is a constant, so which cell is irrelevant.  Otherwise the search ran to its
// end and kept exactly that key's cell.  The key is one word, |d_k|^2 * n + k.
//
//   ring form   one wavefront per pose: lanes take the offsets lane, lane + 64, ..., test their cell as checkCell does and
//               the wavefront takes the minimum over its lanes' keys -- n / 64 independent byte loads per lane.
//   map form    a key map over the centres [-reach, xsize + reach) x [-reach, ysize + reach), filled with "no key" and
//               built by scatter (the occupied cells atomicMin their key into every centre that reaches them); a query is
//               one load.  The buffers are kept per (device, stream) like the inflated map's.
// Which form a call takes: use_key_map below (measured: profiles/clearance.txt).
#include <array>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <mutex>
#include <vector>

#include "../../include/ergodic_amd.h"
#include "common.hpp"
#include "grid_cell.hpp"      // world_to_grid (grid.cpp:143-159), occupied, write_answer
#include "hit_map_table.hpp"  // clearance_walk, kNoClearanceKey, HitMapTable
#include "device_tables.hpp"  // DeviceTables: the walk kept per device
#include "grid_buffers.hpp"   // upload_block, acquire_map_buffer, launch_then_free

namespace eea
{
namespace
{
// the walk on the device: off [n] in visit order, root [n] = sqrt((double)|d_k|^2) as the host's IEEE sqrt gives it (one
// allocation: the doubles first)
struct ClearTable
{
  const short2* off = nullptr;
  const double* root = nullptr;
  int n = 0;
};
struct ClearOut
{
  int* out;      // [.][4]: msg, sqrd_obs, dx, dy
  double* dmin;  // [.]
  double* disp;  // [.][2]
};
// key map over the centres [-R, xsize + R) x [-R, ysize + R), row-major
struct KeyMap
{
  const unsigned* keys = nullptr;
  int R = 0;
  long long w = 0, h = 0;
};

// centre q of a launch: pose q's cell as collisionCheck derives it (FIELD: cell q of the grid itself)
template <bool FIELD>
__device__ __forceinline__ void clearance_centre(const CollisionParams& c, const double* __restrict__ pose, size_t q, int& cx,
                                                 int& cy)
{
  if (FIELD) {
    cy = static_cast<int>(q / c.xsize);
    cx = static_cast<int>(q - static_cast<size_t>(cy) * c.xsize);
  } else {
    unsigned j, i;
    world_to_grid(c, pose[3 * q], pose[3 * q + 1], j, i);
    cx = static_cast<int>(j);
    cy = static_cast<int>(i);
  }
}

// collision.cpp:79-92 and :107-123 from the smallest key of a centre
__device__ __forceinline__ ClearanceAnswer clearance_answer(const CollisionParams& c, const ClearTable& t, double boundary_radius,
                                                            unsigned key)
{
  ClearanceAnswer a{ EEA_COLLISION_NONE, -1, 0, 0, DBL_MAX, DBL_MAX, DBL_MAX };
  if (key != kNoClearanceKey) {
    const unsigned ksq = key / static_cast<unsigned>(t.n), k = key - ksq * static_cast<unsigned>(t.n);
    if (static_cast<int>(ksq) <= c.r_col * c.r_col) {  // collision.cpp:239
      a.msg = EEA_COLLISION_CRASH;
      a.sq = 0;
      a.dmin = a.d0 = a.d1 = 0.0;
    } else {
      const short2 d = t.off[k];
      a.msg = EEA_COLLISION_OBSTACLE;
      a.sq = static_cast<int>(ksq);
      a.dx = d.x;
      a.dy = d.y;
      a.dmin = t.root[k] * c.resolution - boundary_radius;  // collision.cpp:86-87
      a.d0 = c.resolution * static_cast<double>(a.dx);       // collision.cpp:116-117
      a.d1 = c.resolution * static_cast<double>(a.dy);
    }
  }
  return a;
}

// ring form: wavefront q / 64 of the launch answers centre q / 64
template <bool FIELD>
__global__ __launch_bounds__(kBlock) void clearance_ring_kernel(const CollisionParams c, const ClearTable t,
                                                                double boundary_radius, const int8_t* __restrict__ grid,
                                                                const double* __restrict__ pose, size_t n, const ClearOut o)
{
  const size_t q = static_cast<size_t>(blockIdx.x) * (kBlock / kWave) + threadIdx.x / kWave;  // wavefront-uniform
  if (q >= n) return;
  const int lane = threadIdx.x % kWave;
  int cx, cy;
  clearance_centre<FIELD>(c, pose, q, cx, cy);
  unsigned best = kNoClearanceKey;
  for (int k = lane; k < t.n; k += kWave) {
    const short2 d = t.off[k];
    // collision.cpp:216-243: the cell's indices are unsigned (a centre outside the map wraps), in bounds by grid.cpp:96-100
    const unsigned cj = static_cast<unsigned>(cx) + static_cast<unsigned>(static_cast<int>(d.x));
    const unsigned ci = static_cast<unsigned>(cy) + static_cast<unsigned>(static_cast<int>(d.y));
    if ((ci <= c.ysize - 1u) && (cj <= c.xsize - 1u)) {
      if (occupied(c, grid[ci * c.xsize + cj])) {
        const unsigned key = static_cast<unsigned>(d.x * d.x + d.y * d.y) * static_cast<unsigned>(t.n) + static_cast<unsigned>(k);
        best = key < best ? key : best;  // (k ascends within a lane)
      }
    }
  }
#pragma unroll
  for (int m = kWave / 2; m >= 1; m >>= 1) {
    const unsigned other = __shfl_xor(best, m, kWave);
    best = other < best ? other : best;
  }
  if (lane == 0) write_answer(o.out, o.dmin, o.disp, q, clearance_answer(c, t, boundary_radius, best));
}

// map form, build: occupied cells put their key into every centre that reaches them (listed and walked as in inflate_kernel)
__global__ __launch_bounds__(kBlock) void clearance_scatter_kernel(const CollisionParams c, const int8_t* __restrict__ grid,
                                                                   const ClearTable t, unsigned* __restrict__ keys, int R,
                                                                   long long w)
{
  __shared__ unsigned s_list[kBlock];
  __shared__ unsigned s_n;
  if (threadIdx.x == 0) s_n = 0u;
  __syncthreads();
  const size_t q = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  const size_t n = static_cast<size_t>(c.xsize) * c.ysize;
  if (q < n && occupied(c, grid[q])) s_list[atomicAdd(&s_n, 1u)] = threadIdx.x;
  __syncthreads();
  const unsigned cnt = s_n;
  for (unsigned l = 0; l < cnt; ++l) {
    const size_t qq = static_cast<size_t>(blockIdx.x) * kBlock + s_list[l];
    const long long i = static_cast<long long>(qq / c.xsize), j = static_cast<long long>(qq - static_cast<size_t>(i) * c.xsize);
    for (int k = threadIdx.x; k < t.n; k += kBlock) {
      const short2 d = t.off[k];  // cell = centre + d; |d.x|, |d.y| <= R
      const unsigned key = static_cast<unsigned>(d.x * d.x + d.y * d.y) * static_cast<unsigned>(t.n) + static_cast<unsigned>(k);
      unsigned* const at = &keys[static_cast<size_t>((i - d.y + R) * w + (j - d.x + R))];
      // (keys only fall during a build: a plain read that already shows a smaller one spares the atomic, a stale larger one
      // costs an atomic that changes nothing)
      if (*at > key) atomicMin(at, key);
    }
  }
}

// map form, query: one lane per centre
template <bool FIELD>
__global__ __launch_bounds__(kBlock) void clearance_map_kernel(const CollisionParams c, const ClearTable t, double boundary_radius,
                                                               const KeyMap m, const double* __restrict__ pose, size_t n,
                                                               const ClearOut o)
{
  const size_t q = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (q >= n) return;
  int cx, cy;
  clearance_centre<FIELD>(c, pose, q, cx, cy);
  // centres further than R outside the grid reach no cell (their unsigned cell indices fall outside gridBounds)
  const long long hx = static_cast<long long>(cx) + m.R, hy = static_cast<long long>(cy) + m.R;
  unsigned key = kNoClearanceKey;
  if (hx >= 0 && hy >= 0 && hx < m.w && hy < m.h) key = m.keys[static_cast<size_t>(hy * m.w + hx)];
  write_answer(o.out, o.dmin, o.disp, q, clearance_answer(c, t, boundary_radius, key));
}

// ---- host side ----------------------------------------------------------------------------------------------------
// The walk depends on two small integers: enumerated once per (r_bnd, r_max) and kept, with the verdict on its key; its copy
// in a device's memory once per (device, r_bnd, r_max).
using WalkKey = std::array<int, 2>;  // r_bnd, r_max
struct WalkEntry
{
  WalkKey key;
  bool fits;
  ClearanceWalk walk;
};
struct DeviceWalk
{
  ClearTable t;
  int reach;
};
std::mutex g_walk_mutex;  // guards both lists
std::vector<WalkEntry> g_walks;
DeviceTables<WalkKey, DeviceWalk> g_tables;

const WalkEntry& host_walk(const CollisionParams& c)  // (g_walk_mutex held; the reference stays valid until the next call)
{
  const WalkKey key{ c.r_bnd, c.r_max };
  for (const WalkEntry& e : g_walks) {
    if (e.key == key) return e;
  }
  WalkEntry e{ key, false, {} };
  e.fits = clearance_walk(c.r_bnd, c.r_max, e.walk);
  if (!e.fits) e.walk = ClearanceWalk{};
  g_walks.push_back(std::move(e));
  return g_walks.back();
}

hipError_t device_table(int device, const CollisionParams& c, ClearTable& t, int& reach)
{
  std::lock_guard<std::mutex> lock(g_walk_mutex);
  const DeviceTables<WalkKey, DeviceWalk>::Entry* ent = g_tables.find(device, WalkKey{ c.r_bnd, c.r_max });
  if (ent == nullptr) {
    const WalkEntry& we = host_walk(c);
    if (!we.fits) return hipErrorInvalidValue;
    const size_t n = we.walk.offsets.size();
    std::vector<double> root(n);
    for (size_t k = 0; k < n; ++k) {
      const short2 d = we.walk.offsets[k];
      root[k] = std::sqrt(static_cast<double>(d.x * d.x + d.y * d.y));
    }
    void* block = nullptr;  // (one allocation: the doubles first)
    const hipError_t e = upload_block(root.data(), n * sizeof(double), we.walk.offsets.data(), n * sizeof(short2), &block);
    if (e != hipSuccess) return e;
    const double* const d_root = static_cast<const double*>(block);
    const ClearTable table{ reinterpret_cast<const short2*>(d_root + n), d_root, static_cast<int>(n) };
    ent = &g_tables.insert(device, we.key, block, DeviceWalk{ n > 0 ? table : ClearTable{}, we.walk.reach });
  }
  t = ent->view.t;
  reach = ent->view.reach;
  return hipSuccess;
}

// the key-map buffer of a (device, stream) pair is kept between calls: HitMapTable's slots (hit_map_table.hpp) without its
// stamps -- atomicMin needs every word at "no key", so every build fills the buffer
std::mutex g_key_maps_mutex;
HitMapTable g_key_maps;

hipError_t build_key_map(const CollisionParams& c, const ClearTable& t, int reach, const int8_t* d_grid, int device, hipStream_t s,
                         KeyMap& map, void*& async_cells)
{
  const long long w = static_cast<long long>(c.xsize) + 2 * reach, h = static_cast<long long>(c.ysize) + 2 * reach;
  const size_t bytes = static_cast<size_t>(w) * static_cast<size_t>(h) * sizeof(unsigned);
  MapBuffer b;
  hipError_t e;
  {
    std::lock_guard<std::mutex> lock(g_key_maps_mutex);  // (for the plan and the allocation only)
    e = acquire_map_buffer(g_key_maps, device, s, bytes, nullptr, 0, c, b);
  }
  async_cells = b.async_cells;
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(b.cells, 0xff, bytes, s);  // kNoClearanceKey in every word
  if (e != hipSuccess) return e;
  if (t.n > 0) {
    const size_t n = static_cast<size_t>(c.xsize) * c.ysize;
    hipLaunchKernelGGL(clearance_scatter_kernel, dim3(static_cast<unsigned>((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, c,
                       d_grid, t, static_cast<unsigned*>(b.cells), reach, w);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  map = KeyMap{ static_cast<const unsigned*>(b.cells), reach, w, h };
  return hipSuccess;
}

// Key map or ring form?  EEA_OPT_COLLISION_IMPL = 1 / 2 forces one of them, as for collisionCheck.  Otherwise the n
// centres of a call (the poses of a batch, the cells of a field) take the cheaper of
//   ring   kRingFixedUs + kRingPassUs * n * ceil(n_off / 64)     one wavefront per centre, a pass = 64 offsets
//   map    kMapCentreUs * centres of the key map                  fill + scatter; the one load per centre of the call is
//                                                                 not resolved by the measurement (86.7 us at 64 poses,
//                                                                 86.5 us at 32768)
// Measured on an MI355X (profiles/clearance.txt: the 240 x 120 demo map with 1480 occupied cells, 744 offsets = 12 passes,
// a key map of 280 x 160 centres): the ring form takes 9.1 - 9.5 us up to 4096 poses and 33.0 us at 32768, 26.9 us for
// the field's 28800 cells; the map form takes 86 - 88 us at every P, all of it the build: 14.5 us for the fill and the three
// launches (an empty grid), the rest for 1.1 million keyed scatters.  The build's real cost follows occupied cells x
// offsets, which the host does not know; the model charges it per centre of the map, as that one map measured it.  With
// these numbers the ring form answers every batch the tool ran and the field; the map pays from about 1.3 million
// centre-passes per call on.
constexpr double kRingFixedUs = 9.1, kRingPassUs = 6.1e-5;
constexpr double kMapCentreUs = 1.92e-3;
bool use_key_map(size_t n, const CollisionParams& c, const ClearTable& t, int reach)
{
  const int forced = option(EEA_OPT_COLLISION_IMPL);
  if (forced != 0) return forced == 2;
  const double centres = (static_cast<double>(c.xsize) + 2.0 * reach) * (static_cast<double>(c.ysize) + 2.0 * reach);
  const double passes = static_cast<double>((t.n + kWave - 1) / kWave);
  const double t_ring = kRingFixedUs + kRingPassUs * static_cast<double>(n) * passes;
  const double t_map = kMapCentreUs * centres;
  return t_map < t_ring;
}
}  // namespace

bool clearance_supported(const CollisionParams& c)
{
  std::lock_guard<std::mutex> lock(g_walk_mutex);
  return host_walk(c).fits;
}

hipError_t launch_clearance(const CollisionParams& c, double boundary_radius, const int8_t* d_grid, const double* d_pose, size_t n,
                            int* d_out, double* d_dmin, double* d_disp, hipStream_t s)
{
  if (n == 0) return hipSuccess;
  int device = 0, reach = 0;
  ClearTable t;
  hipError_t e = hipGetDevice(&device);
  if (e == hipSuccess) e = device_table(device, c, t, reach);
  if (e != hipSuccess) return e;
  const bool field = d_pose == nullptr;
  const ClearOut o{ d_out, d_dmin, d_disp };
  if (!use_key_map(n, c, t, reach)) {
    const dim3 blocks(static_cast<unsigned>((n + kBlock / kWave - 1) / (kBlock / kWave)));
    const auto ring = field ? clearance_ring_kernel<true> : clearance_ring_kernel<false>;
    hipLaunchKernelGGL(ring, blocks, dim3(kBlock), 0, s, c, t, boundary_radius, d_grid, d_pose, n, o);
    return hipGetLastError();
  }
  KeyMap map;
  void* async_cells = nullptr;
  e = build_key_map(c, t, reach, d_grid, device, s, map, async_cells);
  return launch_then_free(e, async_cells, s, [&] {
    const auto query = field ? clearance_map_kernel<true> : clearance_map_kernel<false>;
    hipLaunchKernelGGL(query, dim3(static_cast<unsigned>((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, c, t, boundary_radius, map,
                       d_pose, n, o);
  });
}

void release_clearance_caches()
{
  const CurrentDeviceGuard guard;
  {
    std::lock_guard<std::mutex> lock(g_key_maps_mutex);
    g_key_maps.release(free_on_device);
  }
  std::lock_guard<std::mutex> lock(g_walk_mutex);
  g_tables.release(free_on_device);
  g_walks.clear();
}
}  // namespace eea
