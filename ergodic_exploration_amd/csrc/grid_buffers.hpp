// The HIP effects behind the host-side policies of the grid queries (hit_map_table.hpp, device_tables.hpp), written once for
// collision_kernel.hip, clearance_kernel.hip and fleet_layer_kernel.hip.  The caller holds the lock of the policy object.
#pragma once

#include <hip/hip_runtime.h>

#include "hit_map_table.hpp"

namespace eea
{
// a release visits every device that holds a buffer (free_on_device): the device that was current comes back with the guard
struct CurrentDeviceGuard
{
  int device = 0;
  const bool have = hipGetDevice(&device) == hipSuccess;
  ~CurrentDeviceGuard() { if (have) (void)hipSetDevice(device); }
};
inline void free_on_device(int device, void* block)
{
  if (hipSetDevice(device) == hipSuccess) (void)hipFree(block);  // waits for its users
}

// One allocation on the current device that holds host part a and, at the next multiple of 8 bytes (block_offset), part b;
// *block = null when there is nothing to hold.  Freed again on any failure.
constexpr size_t block_offset(size_t a_bytes) { return (a_bytes + 7u) & ~static_cast<size_t>(7u); }
inline hipError_t upload_block(const void* a, size_t a_bytes, const void* b, size_t b_bytes, void** block)
{
  *block = nullptr;
  if (a_bytes + b_bytes == 0) return hipSuccess;
  void* p = nullptr;
  hipError_t e = hipMalloc(&p, block_offset(a_bytes) + b_bytes);
  if (e == hipSuccess && a_bytes > 0) e = hipMemcpy(p, a, a_bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess && b_bytes > 0) e = hipMemcpy(static_cast<char*>(p) + block_offset(a_bytes), b, b_bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) *block = p;
  else if (p != nullptr) (void)hipFree(p);
  return e;
}

// The buffer one build of a map gets: HitMapTable's plan with its allocation carried out, `cells` is where to build.  A full
// table gives a stream-ordered `async_cells` instead, which the caller frees behind the map's readers whatever is returned.
struct MapBuffer
{
  HitMapPlan plan;
  void *cells, *async_cells = nullptr;
};
inline hipError_t acquire_map_buffer(HitMapTable& table, int device, hipStream_t s, size_t bytes, const void* grid,
                                     unsigned long long epoch, const CollisionParams& c, MapBuffer& b)
{
  b.plan = table.plan(device, s, bytes, grid, epoch, c);
  b.cells = b.plan.cells;
  if (b.plan.slot < 0) {
    const hipError_t e = hipMallocAsync(&b.async_cells, bytes, s);
    b.cells = b.async_cells;
    return e;
  }
  if (!b.plan.reallocate) return hipSuccess;
  if (b.plan.cells) (void)hipFree(b.plan.cells);  // waits for the kernels that still use it (the slot has forgotten it already)
  const hipError_t e = hipMalloc(&b.cells, bytes);
  if (e == hipSuccess) table.allocated(b.plan.slot, b.cells, bytes);
  return e;
}

// `launch` enqueues the readers of a map on s if its build succeeded; the launch error is taken here, once, behind them,
// and the stream-ordered buffer (if any) is freed behind them whatever happened
template <typename Launch>
hipError_t launch_then_free(hipError_t built, void* async_cells, hipStream_t s, Launch launch)
{
  if (built == hipSuccess) {
    launch();
    built = hipGetLastError();
  }
  if (async_cells) (void)hipFreeAsync(async_cells, s);
  return built;
}
}  // namespace eea
