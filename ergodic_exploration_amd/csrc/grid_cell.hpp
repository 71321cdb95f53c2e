// GridMap::world2Grid (reference grid.cpp:143-159) on the device, bit-exact with the reference's x86-64 build: the ONE
// definition the collision kernels (collision_kernel.hip) and the range sensor (sense_kernel.hip) take a pose's cell from.
// With it the other device pieces the grid queries share: the literal occupancy test and the writer of a clearance answer
// (clearance_kernel.hip, distance_kernel.hip).  Every translation unit that includes this is compiled with -ffp-contract=off.
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

// checkCell's test on GridMap::getCell (collision.cpp:216-243, grid.cpp:177-184) in the reference's literal form: a cell of
// value v is occupied iff !(v / 100.0 < threshold)
__device__ __forceinline__ bool occupied(const CollisionParams& c, int8_t v)
{
  return !(static_cast<double>(v) / 100.0 < c.occupied_threshold);
}

// The answer of one centre (clearance_kernel.hip, distance_kernel.hip) and its one writer: out [.][4] ints (msg, sqrd_obs,
// dx, dy), dmin [.], disp [.][2], each of which may be null
struct ClearanceAnswer
{
  int msg, sq, dx, dy;
  double dmin, d0, d1;
};
__device__ __forceinline__ void write_answer(int* __restrict__ out, double* __restrict__ dmin, double* __restrict__ disp, size_t q,
                                             const ClearanceAnswer& a)
{
  if (out != nullptr) {
    out[4 * q] = a.msg;
    out[4 * q + 1] = a.sq;
    out[4 * q + 2] = a.dx;
    out[4 * q + 3] = a.dy;
  }
  if (dmin != nullptr) dmin[q] = a.dmin;
  if (disp != nullptr) {
    disp[2 * q] = a.d0;
    disp[2 * q + 1] = a.d1;
  }
}
}  // namespace eea
