// Information-gain field of a known grid (include/ergodic_amd.h, eea_sense_gain_field / eea_set_target_gain): for every
// candidate cell -- the lattice i0 % stride == 0 && j0 % stride == 0 --, how many unknown cells the 8R rays of the range sensor
// (sense_rays.hpp: the reveal's rays, steps, disc and blocking rule) would cross when cast from there through `known` itself,
// counted per beam, plus one if the cell itself is unknown.  Integers only, no atomics, every element of d_gain written once.
//
//  - a workgroup of 256 threads owns a tile of 32 x 8 candidates (the tiling is gain_tile.hpp's, shared with mi_kernel.hip),
//    A LANE IS A CANDIDATE: the ray geometry (q, s, dx, dy and the remainder recurrence) does not depend on the lane and stays in scalar registers; per step a lane reads one cell at its
//    own base plus a uniform offset, adds `alive & unknown` and clears `alive` on a cell that ends the ray.  A ray ends for the
//    wavefront where it leaves the disc or no lane is alive.  No cross-lane reduction.
//  - LDS form: the union of the tile's windows, (31 stride + 1 + 2R) x (7 stride + 1 + 2R) cells, is staged as one byte per
//    cell -- bit 0 blocks, bit 1 unknown, bit 2 off the grid -- with coalesced row reads (gain_tile.hpp: stage_window, under
//    this field's encoder); the R cells of padding on every side
//    are off-grid bytes, so the march has no bounds test and no LDS write.  Taken when the window fits the 64 KB a launch may
//    ask for without opting in (stride 1: R <= 118; 2: R <= 109; 4: R <= 91; 8: R <= 60).
//  - global form (everything else, up to R = 1024 and any stride): the same tile, every lane marches its own rays through
//    `known` in global memory with march() and the clip of its cell.  Correct, and slow by the chain of dependent byte loads.
//  Both forms zero the cells of their tile's footprint that are off the lattice (stride > 1) and store the lattice cells
//  from the lane that owns them: no cell has two writers.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.hpp"
#include "gain_tile.hpp"
#include "sense_rays.hpp"

namespace eea
{
namespace
{
struct GainParams : CandidateGrid
{
  unsigned* gain;
};

__global__ __launch_bounds__(kGainBlock) void gain_field_lds_kernel(const GainParams p)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char s_win[];  // [H][W]: bit 0 blocks, bit 1 unknown, bit 2 off-grid
  const int R = p.R, W = p.W, tid = threadIdx.x;
  const int st = static_cast<int>(p.stride);  // (small: the window fits 64 KB)
  const int base = ((tid / kGainTX) * st + R) * W + (tid % kGainTX) * st + R;
  for (unsigned long long t = blockIdx.x; t < p.tiles; t += gridDim.x) {
    __syncthreads();  // the tile before has read the window
    const Tile k = tile_of(p, t);
    stage_window(p, k, s_win, 4, [&](int v) { return (v >= p.cutoff ? 1 : 0) | (v < 0 ? 2 : 0); });
    zero_off_lattice(p, k, p.gain);
    __syncthreads();
    const unsigned own = s_win[base];  // (inside the window for every lane, candidate or not)
    const bool cand = k.in && (own & 5u) == 0u;  // a robot cannot stand in a blocking cell
    unsigned count = cand ? (own >> 1) & 1u : 0u;
    if (__builtin_amdgcn_ballot_w64(cand) != 0) {
      for (int q = 0; q < 8 * R; ++q) {
        Ray ray(q, R);  // (the same in every lane: scalar registers)
        unsigned alive = cand ? 1u : 0u;
        // kGainChunk steps at a time: their offsets are formed and their cells read before the first one is used, so a
        // wavefront has that many LDS reads in flight instead of one dependent read per step
        for (int s0 = 1; s0 <= R; s0 += kGainChunk) {
          unsigned v[kGainChunk];
          bool in[kGainChunk];
#pragma unroll
          for (int u = 0; u < kGainChunk; ++u) {
            ray.step(R);
            in[u] = s0 + u <= R && ray.in_disc(R);
            // |dx|, |dy| <= R while s <= R: inside the padded window; a step that does not count reads the lane's own cell
            v[u] = s_win[base + (in[u] ? ray.dy * W + ray.dx : 0)];
          }
#pragma unroll
          for (int u = 0; u < kGainChunk; ++u) {
            alive = in[u] ? alive : 0u;  // (uniform) past the disc or step R the ray has ended for every lane
            count += alive & (v[u] >> 1);  // (alive is 0 / 1: bit 0 of v >> 1 is "unknown")
            alive = (v[u] & 5u) != 0u ? 0u : alive;  // a blocking cell is counted, then ends the ray; so does the grid's edge
          }
          if (__builtin_amdgcn_ballot_w64(alive != 0u) == 0) break;
        }
      }
    }
    if (k.in) p.gain[static_cast<size_t>(k.i0) * p.c.xsize + k.j0] = count;
  }
}

__global__ __launch_bounds__(kGainBlock) void gain_field_global_kernel(const GainParams p)
{
  const int R = p.R;
  for (unsigned long long t = blockIdx.x; t < p.tiles; t += gridDim.x) {
    const Tile k = tile_of(p, t);
    zero_off_lattice(p, k, p.gain);
    if (!k.in) continue;
    const size_t g0 = static_cast<size_t>(k.i0) * p.c.xsize + k.j0;
    const int own = p.known[g0];
    unsigned count = 0u;
    if (own < p.cutoff) {
      count = own < 0 ? 1u : 0u;
      const Clip w = clip_of(p.c, k.i0, k.j0, R);
      for (int q = 0; q < 8 * R; ++q) {
        (void)march(q, R, w, [&](int dx, int dy) {
          const int v = p.known[cell_index(p.c, k.i0, k.j0, dx, dy)];
          count += v < 0 ? 1u : 0u;
          return v >= p.cutoff;
        });
      }
    }
    p.gain[g0] = count;
  }
}

// the value grid of eea_set_target_gain: (real)((double)gain + floor) on the candidates whose cell does not block, 0 elsewhere
// (gain_tile.hpp: candidate_values)
template <typename R>
__global__ __launch_bounds__(kGainBlock) void gain_values_kernel(const int8_t* __restrict__ known, const unsigned* __restrict__ gain,
                                                                 unsigned xsize, unsigned ysize, unsigned stride, int cutoff,
                                                                 double floor, R* __restrict__ out)
{
  candidate_values<R, unsigned, false>(known, gain, nullptr, xsize, ysize, stride, cutoff, floor, out);
}

}  // namespace

hipError_t launch_gain_field(const CollisionParams& c, unsigned range_cells, unsigned stride, const int8_t* d_known, unsigned* d_gain,
                             hipStream_t s)
{
  GainParams p;
  size_t lds = 0;
  const unsigned blocks = candidate_grid(c, range_cells, stride, d_known, 0, p, &lds);
  p.gain = d_gain;
  if (lds != 0) {
    hipLaunchKernelGGL(gain_field_lds_kernel, dim3(blocks), dim3(kGainBlock), lds, s, p);
  } else {
    hipLaunchKernelGGL(gain_field_global_kernel, dim3(blocks), dim3(kGainBlock), 0, s, p);
  }
  return hipGetLastError();
}

template <typename R>
hipError_t launch_gain_values(const CollisionParams& c, unsigned stride, const int8_t* d_known, const unsigned* d_gain, double floor,
                              R* d_values, hipStream_t s)
{
  hipLaunchKernelGGL(gain_values_kernel<R>, values_grid(c), dim3(kGainBlock), 0, s, d_known, d_gain, c.xsize, c.ysize, stride,
                     blocking_cutoff(c.occupied_threshold), floor, d_values);
  return hipGetLastError();
}
template hipError_t launch_gain_values<double>(const CollisionParams&, unsigned, const int8_t*, const unsigned*, double, double*,
                                               hipStream_t);
template hipError_t launch_gain_values<float>(const CollisionParams&, unsigned, const int8_t*, const unsigned*, double, float*,
                                              hipStream_t);
}  // namespace eea
