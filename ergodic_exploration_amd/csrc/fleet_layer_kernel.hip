// Fleet layer for gfx950: the robots of a fleet as obstacles to one another, built from their poses every tick.
//
// The rule (integer arithmetic; include/ergodic_amd.h states it for callers): with S = ring_offsets(r_bnd, r_col, r_max) and a
// body radius `body` in cells, F = { o + d : o in S, d.d <= body^2 } (fleet_spans.hpp).  Every active robot whose cell --
// world_to_grid of its pose, the x86 wrap included -- lies inside the grid is an obstacle, and a pose with centre cell c
// collides with robot j iff c - cell_j in F.  That is Collision::collisionCheck (reference collision.cpp:126-243) on a grid in
// which the cells within d.d <= body^2 of cell_j are occupied, whenever that disc lies inside the grid; near the edge the rule
// keeps the whole body, it does not clip the disc to the grid.
//
// The inflated collision map (collision_kernel.hip) turns the ring search into a byte lookup per pose; this is the same idea
// with a COUNT per centre cell instead of a mark: count[c] = the robots j with c - cell_j in F.  A robot takes its own body
// out of the count it reads by the membership test (c - own) in F (fleet_lookup, collision_kernel.hip).
//
// An update is three stream operations, no host wait:
//   1. clear an int32 difference map over the centres [-R', xsize + R') x [-R', ysize + R'), R' = r_col + body;
//   2. stamp: one wavefront per robot, lanes over the robot's row spans of F: +1 at a span's start, -1 behind its end
//      (2 x spans atomics per robot instead of |F|: 122 instead of 2789 for the demo robot with body = r_bnd = 13);
//   3. prefix sum along every row, in place.  Integer sums: the result is exact whatever the order of the atomics.
#include <hip/hip_runtime.h>

#include <array>
#include <cstdint>
#include <mutex>
#include <vector>

#include "common.hpp"
#include "device_tables.hpp"  // DeviceTables: the span tables kept per device, counted by the layers that hold them
#include "fleet_spans.hpp"
#include "grid_buffers.hpp"  // upload_block, CurrentDeviceGuard
#include "grid_cell.hpp"  // world_to_grid: the cell of a pose as the collision kernels and the range sensor derive it

namespace eea
{
namespace
{
// One wavefront per robot.  Every write lands inside the map: the robot's cell is inside the grid and F within the reach R,
// so cell + offset + R is in [0, w) x [0, h); the -1 behind a span that ends at the map's last column is dropped (nothing
// follows it in the row).
__global__ __launch_bounds__(kWave) void fleet_stamp_kernel(const CollisionParams c, const double* __restrict__ pose,
                                                            const int* __restrict__ mask, unsigned B,
                                                            const FleetSpan* __restrict__ spans, int n_spans, int R, int w,
                                                            int* __restrict__ count, int* __restrict__ cell)
{
  const unsigned r = blockIdx.x;
  if (r >= B) return;
  unsigned j = 0, i = 0;
  bool stamped = mask == nullptr || mask[r] != 0;
  if (stamped) {
    world_to_grid(c, pose[3 * static_cast<size_t>(r)], pose[3 * static_cast<size_t>(r) + 1], j, i);
    stamped = j < c.xsize && i < c.ysize;  // (gridBounds, grid.cpp:109-117)
  }
  if (threadIdx.x == 0) {
    cell[2 * static_cast<size_t>(r)] = stamped ? static_cast<int>(j) : kFleetNotStamped;
    cell[2 * static_cast<size_t>(r) + 1] = stamped ? static_cast<int>(i) : kFleetNotStamped;
  }
  if (!stamped) return;  // (wavefront-uniform)
  const int cx = static_cast<int>(j) + R, cy = static_cast<int>(i) + R;
  for (int k = threadIdx.x; k < n_spans; k += kWave) {
    const FleetSpan sp = spans[k];
    int* const row = count + static_cast<size_t>(cy + sp.dy) * w;
    atomicAdd(row + (cx + sp.x0), 1);
    if (cx + sp.x1 + 1 < w) atomicAdd(row + (cx + sp.x1 + 1), -1);
  }
}

// In-place inclusive prefix sum along every row: one wavefront per row (four rows per workgroup), 64 cells per pass with the
// running sum carried from pass to pass; within a pass a 6-step shuffle scan.  Every lane of a wavefront runs every shuffle
// (the row index and the pass count are wavefront-uniform; lanes past the row's end carry zeros and store nothing).
constexpr int kScanRows = 4;
__global__ __launch_bounds__(kWave* kScanRows) void fleet_row_scan_kernel(int* __restrict__ count, int w, int h)
{
  const int lane = threadIdx.x % kWave;
  const int row = blockIdx.x * kScanRows + threadIdx.x / kWave;
  if (row >= h) return;
  int* const p = count + static_cast<size_t>(row) * w;
  int carry = 0;
  for (int x0 = 0; x0 < w; x0 += kWave) {
    const int x = x0 + lane;
    int v = x < w ? p[x] : 0;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
      const int up = __shfl_up(v, d, kWave);
      if (lane >= d) v += up;
    }
    v += carry;
    if (x < w) p[x] = v;
    carry = __shfl(v, kWave - 1, kWave);
  }
}
}  // namespace

// ---- the span tables in device memory -----------------------------------------------------------
namespace
{
using SpanKey = std::array<int, 4>;  // r_bnd, r_col, r_max, body
struct SpanTable
{
  const int* row_start;
  const FleetSpan* spans;
  int n_spans;
};
std::mutex g_spans_mutex;
DeviceTables<SpanKey, SpanTable> g_span_tables;  // (the layers hold their entry: a live layer reads it)
}  // namespace

hipError_t acquire_fleet_spans(int device, const CollisionParams& c, int body, const int** d_row_start, const FleetSpan** d_spans,
                               int* n_spans)
{
  std::lock_guard<std::mutex> lock(g_spans_mutex);
  const SpanKey key{ c.r_bnd, c.r_col, c.r_max, body };
  const DeviceTables<SpanKey, SpanTable>::Entry* ent = g_span_tables.find(device, key, true);
  if (ent == nullptr) {
    const FleetSpans t = fleet_spans(c.r_bnd, c.r_col, c.r_max, body);
    // (one allocation: the row index, then the spans -- 8-byte elements at the next multiple of 8 bytes)
    const size_t row_bytes = t.row_start.size() * sizeof(int);
    void* block = nullptr;
    const hipError_t e = upload_block(t.row_start.data(), row_bytes, t.spans.data(), t.spans.size() * sizeof(FleetSpan), &block);
    if (e != hipSuccess) return e;
    const SpanTable table{ static_cast<const int*>(block),
                           reinterpret_cast<const FleetSpan*>(static_cast<const char*>(block) + block_offset(row_bytes)),
                           static_cast<int>(t.spans.size()) };
    ent = &g_span_tables.insert(device, key, block, table, true);
  }
  *d_row_start = ent->view.row_start;
  *d_spans = ent->view.spans;
  *n_spans = ent->view.n_spans;
  return hipSuccess;
}

void release_fleet_spans(int device, const int* d_row_start)
{
  std::lock_guard<std::mutex> lock(g_spans_mutex);
  g_span_tables.give_back(device, d_row_start);
}

void release_fleet_span_cache()
{
  const CurrentDeviceGuard guard;
  std::lock_guard<std::mutex> lock(g_spans_mutex);
  g_span_tables.release(free_on_device);
}

hipError_t launch_fleet_layer_update(const CollisionParams& c, const FleetView& v, int n_spans, int* d_count, int* d_cell,
                                     const double* d_pose, const int* d_mask, hipStream_t s)
{
  hipError_t e = hipMemsetAsync(d_count, 0, sizeof(int) * static_cast<size_t>(v.w) * v.h, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(fleet_stamp_kernel, dim3(v.B), dim3(kWave), 0, s, c, d_pose, d_mask, v.B, v.spans, n_spans, v.R, v.w, d_count,
                     d_cell);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  return launch_fleet_row_scan(d_count, v.w, v.h, s);
}

hipError_t launch_fleet_row_scan(int* d_map, int w, int h, hipStream_t s)
{
  hipLaunchKernelGGL(fleet_row_scan_kernel, dim3((h + kScanRows - 1) / kScanRows), dim3(kWave * kScanRows), 0, s, d_map, w, h);
  return hipGetLastError();
}
}  // namespace eea
