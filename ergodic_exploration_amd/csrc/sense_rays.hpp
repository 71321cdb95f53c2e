// The ray set of the range sensor (include/ergodic_amd.h, eea_sense_reveal_batch): the ONE definition the reveal kernels
// (sense_kernel.hip) and the information-gain field (gain_kernel.hip) take a ray's steps from.  Integers only: ray q of the 8R
// rays aims at a perimeter cell of [-R, R]^2, step s sits at sgn(m) ((2 s |m| + R) div 2R) per axis -- formed by adding 2|m| per
// step to a remainder that starts at R and wraps at 2R, which is that quotient exactly (2|m| <= 2R: at most one wrap per step).
#pragma once

#include "common.hpp"

namespace eea
{
// what a robot at (i0, j0) can touch: offsets [xlo, xhi] x [ylo, yhi] of [-R, R]^2 that fall on the grid
struct Clip
{
  int xlo, xhi, ylo, yhi;
};
__device__ __forceinline__ Clip clip_of(const CollisionParams& c, unsigned i0, unsigned j0, int R)
{
  Clip w;
  const unsigned uR = static_cast<unsigned>(R), rx = c.xsize - 1u - j0, ry = c.ysize - 1u - i0;
  w.xlo = j0 < uR ? -static_cast<int>(j0) : -R;
  w.xhi = rx < uR ? static_cast<int>(rx) : R;
  w.ylo = i0 < uR ? -static_cast<int>(i0) : -R;
  w.yhi = ry < uR ? static_cast<int>(ry) : R;
  return w;
}

// the cell at offset (dx, dy) from (i0, j0) in a row-major [ysize][xsize] grid
__device__ __forceinline__ size_t cell_index(const CollisionParams& c, unsigned i0, unsigned j0, int dx, int dy)
{
  return (static_cast<size_t>(i0) + static_cast<size_t>(static_cast<long long>(dy))) * c.xsize +
         (static_cast<size_t>(j0) + static_cast<size_t>(static_cast<long long>(dx)));
}

// ray q at step s = 0; step() moves it to the next step's offset (dx, dy).  march()'s recurrence as an object, for a caller
// whose lanes share ONE ray and end it together (gain_kernel.hip); march() below keeps its own loop, statement for statement as
// the reveal kernels were compiled with (their register figures are held to: DESIGN 4.7)
struct Ray
{
  int ax2, ay2, sx, sy, remx, remy, dx, dy;
  __device__ __forceinline__ Ray(int q, int R)
  {
    const int side = q / (2 * R), k = q - side * 2 * R;
    const int tx = side == 0 ? R : side == 1 ? R - k : side == 2 ? -R : -R + k;
    const int ty = side == 0 ? -R + k : side == 1 ? R : side == 2 ? R - k : -R;
    ax2 = 2 * (tx < 0 ? -tx : tx);
    ay2 = 2 * (ty < 0 ? -ty : ty);
    sx = tx > 0 ? 1 : tx < 0 ? -1 : 0;
    sy = ty > 0 ? 1 : ty < 0 ? -1 : 0;
    remx = remy = R;  // (2 s |m| + R) = (2R) (|d|) + rem
    dx = dy = 0;
  }
  __device__ __forceinline__ void step(int R)
  {
    remx += ax2;
    if (remx >= 2 * R) {
      remx -= 2 * R;
      dx += sx;
    }
    remy += ay2;
    if (remy >= 2 * R) {
      remy -= 2 * R;
      dy += sy;
    }
  }
  __device__ __forceinline__ bool in_disc(int R) const { return dx * dx + dy * dy <= R * R; }
};

// ray q of a robot: steps s = 1 .. R until the ray leaves the disc or the grid, or visit(dx, dy) says the cell blocks;
// returns the range s of the blocking cell or -1
template <typename Visit>
__device__ __forceinline__ int march(int q, int R, const Clip& w, Visit visit)
{
  const int side = q / (2 * R), k = q - side * 2 * R;
  const int tx = side == 0 ? R : side == 1 ? R - k : side == 2 ? -R : -R + k;
  const int ty = side == 0 ? -R + k : side == 1 ? R : side == 2 ? R - k : -R;
  const int ax2 = 2 * (tx < 0 ? -tx : tx), ay2 = 2 * (ty < 0 ? -ty : ty);
  const int sx = tx > 0 ? 1 : tx < 0 ? -1 : 0, sy = ty > 0 ? 1 : ty < 0 ? -1 : 0;
  int remx = R, remy = R, dx = 0, dy = 0;  // (2 s |m| + R) = (2R) (|d|) + rem
  for (int s = 1; s <= R; ++s) {
    remx += ax2;
    if (remx >= 2 * R) {
      remx -= 2 * R;
      dx += sx;
    }
    remy += ay2;
    if (remy >= 2 * R) {
      remy -= 2 * R;
      dy += sy;
    }
    if (dx * dx + dy * dy > R * R) break;
    if (dx < w.xlo || dx > w.xhi || dy < w.ylo || dy > w.yhi) break;
    if (visit(dx, dy)) return s;
  }
  return -1;
}
}  // namespace eea
