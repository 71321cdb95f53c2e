// The ray set of the range sensor (include/ergodic_amd.h, eea_sense_reveal_batch): the ONE definition the reveal kernels
// (sense_kernel.hip), the evidence grid's scan (evidence_kernel.hip) and the candidate fields (gain_kernel.hip, mi_kernel.hip)
// take a ray's steps from.  Integers only: ray q of the 8R rays aims at a perimeter cell of [-R, R]^2, step s sits at
// sgn(m) ((2 s |m| + R) div 2R) per axis -- formed by adding 2|m| per step to a remainder that starts at R and wraps at 2R,
// which is that quotient exactly (2|m| <= 2R: at most one wrap per step).
// Behind the rays, what a scan of the fleet is around its staging and its write-out (the reveal stages the truth and copies
// truth -> known, the evidence grid stages what a noisy scan sees and adds evidence): the launch block both carry (ScanParams,
// scan_launch), the robot of a workgroup's turn (robot_cell) and the march on the staged window (march_window).
// The integer code -- Clip, clip_of, cell_index, Ray, march -- compiles on the host: tests/sense_rays_check.cpp drives it.
#pragma once

#include "common.hpp"
#include "grid_cell.hpp"

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
// whose lanes share ONE ray and end it together (the LDS forms of gain_kernel.hip and mi_kernel.hip); march() below keeps its
// own loop, statement for statement as the reveal kernels were compiled with (their register figures are held to: DESIGN
// 4.7).  Both single forms were compiled -- march() over a Ray, and both over one per-axis step function -- and each makes every
// kernel that marches longer (profiles/sensor_family_refactor.txt); tests/sense_rays_check.cpp holds the two to each other
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

// ---- a scan of the fleet: one workgroup of kBlock threads per robot, a thread per ray -----------------------------------
constexpr unsigned kScanMaxBlocks = 1u << 16;  // workgroups per launch; they stride over the robots past that

// what the reveal's and the observe launch read alike; each launch's own parameter block derives from it.  Out: the cell type
// of the grid the scan writes (the reveal: int8_t, `known`; the evidence grid: int32_t, the evidence), which keeps the reveal's
// block in the order its kernels were compiled with
template <typename Out>
struct ScanParams
{
  CollisionParams c;  // the geometry (the radii are not read)
  int R;
  int cutoff;  // a truth cell blocks a ray iff cell >= cutoff (128: no cell does)
  const int8_t* truth;
  Out* out;
  const double* pose;  // [P][3]
  const int* mask;     // [P] or null
  int* ranges;         // [P][8R] or null
  unsigned P;
};

// fills the block and returns the workgroups of the launch; *window_bytes: a robot's (2R + 1)^2 window at one byte per cell
template <typename Out>
inline unsigned scan_launch(const CollisionParams& c, unsigned range_cells, const int8_t* d_truth, Out* d_out, const double* d_pose,
                            const int* d_mask, int* d_ranges, unsigned P, ScanParams<Out>& p, size_t* window_bytes)
{
  p.c = c;
  p.R = static_cast<int>(range_cells);
  p.cutoff = blocking_cutoff(c.occupied_threshold);
  p.truth = d_truth;
  p.out = d_out;
  p.pose = d_pose;
  p.mask = d_mask;
  p.ranges = d_ranges;
  p.P = P;
  const size_t W = 2 * static_cast<size_t>(range_cells) + 1;
  *window_bytes = W * W;
  return P < kScanMaxBlocks ? P : kScanMaxBlocks;
}

#if defined(__HIPCC__)
// the robot of this workgroup's turn: false when the mask leaves it out or its cell is off the grid (mapping.cpp:81-86's
// rule; its row of ranges is then -1).  Uniform over the workgroup
template <typename Out>
__device__ __forceinline__ bool robot_cell(const ScanParams<Out>& p, unsigned b, unsigned& i0, unsigned& j0)
{
  if (p.mask != nullptr && p.mask[b] == 0) return false;
  world_to_grid(p.c, p.pose[3 * static_cast<size_t>(b)], p.pose[3 * static_cast<size_t>(b) + 1], j0, i0);
  if ((i0 <= p.c.ysize - 1u) && (j0 <= p.c.xsize - 1u)) return true;
  if (p.ranges != nullptr) {
    int* const row = p.ranges + static_cast<size_t>(b) * 8u * p.R;
    for (int q = threadIdx.x; q < 8 * p.R; q += kBlock) row[q] = -1;
  }
  return false;
}

// the march phase of robot b on its staged window s_cell [2R + 1][2R + 1] (bit 0 of a byte: the cell blocks a ray): a thread
// per ray sets bit 1 of the cells the ray visits -- every writer of a byte writes the same value, bit 0 is never changed -- and
// stores the ray's range.  Between two barriers of the caller, who marks the robot's own cell (no ray visits offset (0, 0))
template <typename Out>
__device__ __forceinline__ void march_window(const ScanParams<Out>& p, unsigned b, const Clip& w, unsigned char* s_cell)
{
  const int R = p.R, W = 2 * R + 1;
  for (int q = threadIdx.x; q < 8 * R; q += kBlock) {
    const int range = march(q, R, w, [&](int dx, int dy) {
      unsigned char* const cell = s_cell + (dy + R) * W + (dx + R);
      const unsigned char v = *cell;
      if (v < 2) *cell = v | 2;
      return (v & 1) != 0;
    });
    if (p.ranges != nullptr) p.ranges[static_cast<size_t>(b) * 8u * R + q] = range;
  }
}
#endif
}  // namespace eea
