// GridMap::world2Grid (reference grid.cpp:143-159) on the device, bit-exact with the reference's x86-64 build: the ONE
// definition the collision kernels (collision_kernel.hip) and the range sensor (sense_kernel.hip) take a pose's cell from.
// Both translation units are compiled with -ffp-contract=off.
#pragma once

#include "common.hpp"

namespace eea
{
// static_cast<unsigned>(double) as x86-64 gcc compiles it (cvttsd2si r64, low 32 bits):
// negative and > 2^32 values wrap mod 2^32, out-of-range / NaN give 0.  The GPU's own
// double->u32 conversion saturates, so it is not used.
__device__ __forceinline__ unsigned cast_u32_x86(double v)
{
  if (!(v > -9.2233720368547758e18 && v < 9.2233720368547758e18)) return 0u;
  return static_cast<unsigned>(static_cast<unsigned long long>(static_cast<long long>(v)));
}

// grid.cpp:143-159: column j and row i of a world point, a point exactly on the upper edge taken into the last cell
__device__ __forceinline__ void world_to_grid(const CollisionParams& c, double px, double py, unsigned& j, unsigned& i)
{
  j = cast_u32_x86(floor((px - c.xmin) / c.resolution));
  i = cast_u32_x86(floor((py - c.ymin) / c.resolution));
  if (j == c.xsize) j--;
  if (i == c.ysize) i--;
}
}  // namespace eea
