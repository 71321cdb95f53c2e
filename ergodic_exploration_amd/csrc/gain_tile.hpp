// The candidate tiling the information-gain field (gain_kernel.hip) and the mutual-information field (mi_kernel.hip) share: a
// workgroup of 256 threads owns a tile of 32 x 8 candidates of the lattice i0 % stride == 0 && j0 % stride == 0, A LANE IS A
// CANDIDATE, and the union of the tile's sensor windows -- (31 stride + 1 + 2R) x (7 stride + 1 + 2R) cells -- is what the LDS
// forms stage.  The cells of a tile's footprint that are off the lattice are zeroed by the tile, the lattice cells are stored
// by the lanes that own them: no cell has two writers.
// With the tiling: the staging of that window under a per-cell encoder (stage_window: the two fields differ in the byte they
// write per cell and nothing else), and the value grid of a target over a candidate field (candidate_values, values_grid): the
// one body of gain_values_kernel, mi_values_kernel and geodesic_kernel.hip's reachable_values_kernel.
#pragma once

#include <cstdint>

#include "common.hpp"

namespace eea
{
constexpr int kGainBlock = 256, kGainTX = 32, kGainTY = 8;  // a 32-lane LDS group is one row of 32 candidates
constexpr unsigned kGainMaxBlocks = 1u << 16;                // workgroups per launch; they stride over the tiles past that
constexpr size_t kGainLdsMax = 64u * 1024u;                  // what a launch may ask for without opting in
constexpr int kGainChunk = 4;  // steps of a ray whose cells are read before the first is used
static_assert(kGainTX * kGainTY == kGainBlock, "a lane per candidate");

// what both fields' kernels read of a launch; the field's own parameter block derives from it
struct CandidateGrid
{
  CollisionParams c;  // the geometry (the radii are not read)
  int R;
  int cutoff;  // a cell blocks a ray iff cell >= cutoff (128: no cell does)
  unsigned stride;
  const int8_t* known;
  unsigned ncx, ncy;  // candidate columns and rows: ceil(xsize / stride), ceil(ysize / stride)
  unsigned tiles_x;
  unsigned long long tiles;
  int W, H;  // the LDS window (LDS form; 0 x 0: the march runs in global memory)
};

// the grid of a launch and its workgroups; reserved: the LDS bytes the kernel keeps beside the window.  *window_bytes = W * H when
// the window and `reserved` fit the LDS a launch may ask for, 0 otherwise (W = H = 0)
inline unsigned candidate_grid(const CollisionParams& c, unsigned range_cells, unsigned stride, const int8_t* d_known, size_t reserved,
                               CandidateGrid& p, size_t* window_bytes)
{
  p.c = c;
  p.R = static_cast<int>(range_cells);
  p.cutoff = blocking_cutoff(c.occupied_threshold);
  p.stride = stride;
  p.known = d_known;
  p.ncx = (c.xsize - 1u) / stride + 1u;
  p.ncy = (c.ysize - 1u) / stride + 1u;
  p.tiles_x = (p.ncx - 1u) / kGainTX + 1u;
  p.tiles = static_cast<unsigned long long>(p.tiles_x) * ((p.ncy - 1u) / kGainTY + 1u);
  p.W = p.H = 0;
  *window_bytes = 0;
  const unsigned long long W = static_cast<unsigned long long>(kGainTX - 1) * stride + 1u + 2ull * range_cells;
  const unsigned long long H = static_cast<unsigned long long>(kGainTY - 1) * stride + 1u + 2ull * range_cells;
  if (stride <= kGainLdsMax && W * H + reserved <= kGainLdsMax) {
    p.W = static_cast<int>(W);
    p.H = static_cast<int>(H);
    *window_bytes = static_cast<size_t>(W * H);
  }
  return p.tiles < kGainMaxBlocks ? static_cast<unsigned>(p.tiles) : kGainMaxBlocks;
}

// the workgroups of a value-grid launch (candidate_values below): a thread per column, the rows dealt to gridDim.y
inline dim3 values_grid(const CollisionParams& c)
{
  return dim3((c.xsize - 1u) / kGainBlock + 1u, c.ysize < 65535u ? c.ysize : 65535u);
}

#if defined(__HIPCC__)
struct Tile
{
  unsigned long long cx0, cy0;  // first candidate column / row
  bool in;                      // this lane's candidate exists
  unsigned i0, j0;              // ... its cell
};
__device__ __forceinline__ Tile tile_of(const CandidateGrid& p, unsigned long long t)
{
  Tile k;
  k.cx0 = (t % p.tiles_x) * kGainTX;
  k.cy0 = (t / p.tiles_x) * kGainTY;
  const unsigned long long cx = k.cx0 + (threadIdx.x % kGainTX), cy = k.cy0 + (threadIdx.x / kGainTX);
  k.in = cx < p.ncx && cy < p.ncy;
  k.j0 = k.in ? static_cast<unsigned>(cx * p.stride) : 0u;
  k.i0 = k.in ? static_cast<unsigned>(cy * p.stride) : 0u;
  return k;
}

// zeroes the cells of the tile's footprint that are no candidates; the candidates are stored by their lanes
template <typename T>
__device__ __forceinline__ void zero_off_lattice(const CandidateGrid& p, const Tile& k, T* out)
{
  if (p.stride == 1u) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long x0 = k.cx0 * p.stride, y0 = k.cy0 * p.stride;  // (on the grid: the tile has a candidate)
  unsigned long long w = static_cast<unsigned long long>(kGainTX) * p.stride, h = static_cast<unsigned long long>(kGainTY) * p.stride;
  if (w > p.c.xsize - x0) w = p.c.xsize - x0;
  if (h > p.c.ysize - y0) h = p.c.ysize - y0;
  for (unsigned long long ry = wave; ry < h; ry += kGainBlock / 64) {
    const bool lattice_row = static_cast<unsigned>(ry) % p.stride == 0u;
    T* const row = out + (y0 + ry) * p.c.xsize + x0;
    for (unsigned long long rx = lane; rx < w; rx += 64) {
      if (!(lattice_row && static_cast<unsigned>(rx) % p.stride == 0u)) row[rx] = T(0);
    }
  }
}

// stages the union of the tile's sensor windows, s_win [H][W] from R cells in front of the tile's first candidate on, as one byte
// per cell: encode(value) for a cell of the grid, off_grid for the padding.  A wavefront per row, the row read coalesced
template <typename Encode>
__device__ __forceinline__ void stage_window(const CandidateGrid& p, const Tile& k, unsigned char* s_win, int off_grid, Encode encode)
{
  const int R = p.R, W = p.W, H = p.H, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long wx0 = static_cast<long long>(k.cx0 * p.stride) - R, wy0 = static_cast<long long>(k.cy0 * p.stride) - R;
  for (int wy = wave; wy < H; wy += kGainBlock / 64) {
    const long long gy = wy0 + wy;
    const bool row_in = gy >= 0 && gy < static_cast<long long>(p.c.ysize);
    const int8_t* const krow = p.known + (row_in ? static_cast<size_t>(gy) * p.c.xsize : 0);
    unsigned char* const srow = s_win + wy * W;
    for (int wx = lane; wx < W; wx += 64) {
      const long long gx = wx0 + wx;
      int b = off_grid;
      if (row_in && gx >= 0 && gx < static_cast<long long>(p.c.xsize)) b = encode(static_cast<int>(krow[gx]));
      srow[wx] = static_cast<unsigned char>(b);
    }
  }
}

// the value grid of a target over a candidate field (eea_set_target_gain / _mi / _reachable): (real)((double)field + floor) on
// the candidates whose cell does not block -- with GEO: and has geo >= 0 --, 0 elsewhere.  The body of the three value kernels
template <typename R, typename Cell, bool GEO>
__device__ __forceinline__ void candidate_values(const int8_t* __restrict__ known, const Cell* __restrict__ field,
                                                 const int* __restrict__ geo, unsigned xsize, unsigned ysize, unsigned stride,
                                                 int cutoff, double floor, R* __restrict__ out)
{
  const unsigned long long x = static_cast<unsigned long long>(blockIdx.x) * kGainBlock + threadIdx.x;
  if (x >= xsize) return;
  const bool lattice_col = static_cast<unsigned>(x) % stride == 0u;
  for (unsigned y = blockIdx.y; y < ysize; y += gridDim.y) {
    const size_t g = static_cast<size_t>(y) * xsize + x;
    const bool cand = lattice_col && y % stride == 0u && known[g] < cutoff && (!GEO || geo[g] >= 0);
    out[g] = cand ? static_cast<R>(static_cast<double>(field[g]) + floor) : R(0);
  }
}
#endif
}  // namespace eea
