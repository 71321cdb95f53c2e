// Mutual-information field of a known grid (include/ergodic_amd.h, eea_sense_mi_table / eea_sense_mi_field / eea_set_target_mi):
// for every candidate cell of the lattice i0 % stride == 0 && j0 % stride == 0, the Shannon mutual information between the map
// and an ideal beam, summed over the 8R rays of the range sensor (sense_rays.hpp) cast from there through `known` itself:
//     total = h(own);  per ray: reach = 1, beam = 0;  per step: beam += reach * h(v), reach *= pass(v);  total += beam
// in fp64, every product and sum rounded on its own (built with -ffp-contract=off), the rays and their steps in order.  h and
// pass come from ONE table the host builds (mi_table256 below: the only place a log is evaluated) and the launch carries as a
// kernel argument: 103 {h, pass} pairs by compact class -- 0: unknown (v < 0), 1 + min(v, 100): a known cell, 102: off the grid
// ({0, 0}) --, 1648 bytes, copied into LDS by every workgroup.  No upload, no allocation, no atomics, every element of d_mi
// written once.  A dead ray (reach == +0.0) adds +0.0 per step, which changes no bit of a sum >= 0: the step has no branch.
//
//  - the tiling is the gain field's (gain_tile.hpp): a workgroup of 256 owns 32 x 8 candidates, A LANE IS A CANDIDATE, the ray
//    geometry is wavefront-uniform and stays in scalar registers.
//  - LDS form: the table, then the union of the tile's windows as one class byte per cell (gain_tile.hpp: stage_window, the
//    encoder being class_of), the R cells of padding on every side and whatever else is off the grid being class 102.  A step is a byte read, a 16-byte pair read (ds_read_b128) and
//    beam += reach * h; reach *= pass: no bounds test, no blocking test, no alive flag.  kGainChunk steps are read before the
//    first is used.  A ray ends for the wavefront where it leaves the disc or no lane has reach > 0.  Taken when
//    W H + 1648 <= 64 KB (stride 1: R <= 116; 2: R <= 107; 4: R <= 90; 8: R <= 58) and the classes say all the table has to
//    know -- the blocking cutoff is not among the negative cell values (cutoff >= 0, every sensible threshold, or -128).
//  - global form (everything else, up to R = 1024 and any stride, and a threshold below zero that makes SOME negative cells
//    block): every lane marches its own rays through `known` in global memory with march() and the clip of its cell, the table
//    in LDS; a cell's blocking is taken from its value, not from the table, so the form is exact for every threshold.
//  The candidate's own cell is judged by its value in both forms (a cell above 100 shares class 101 with 100 and may or may not
//  block).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "common.hpp"
#include "gain_tile.hpp"
#include "sense_rays.hpp"

namespace eea
{
// include/ergodic_amd.h, eea_sense_mi_table: h and pass of every int8 value, entry v + 128
void mi_table256(double occupied_threshold, double p_unknown, double* h256, double* pass256)
{
  for (int v = -128; v <= 127; ++v) {
    const double o = v < 0 ? p_unknown : static_cast<double>(v < 100 ? v : 100) / 100.0;
    const bool blocks = !(static_cast<double>(v) / 100.0 < occupied_threshold);
    h256[v + 128] = (o == 0.0 || o == 1.0) ? 0.0 : -o * std::log(o) - (1.0 - o) * std::log(1.0 - o);
    pass256[v + 128] = blocks ? 0.0 : 1.0 - o;
  }
}

namespace
{
constexpr int kMiClasses = 103, kMiOffGrid = 102;
constexpr size_t kMiTableBytes = sizeof(double) * 2 * kMiClasses;  // 1648: a multiple of 16, the window starts behind it
static_assert(kMiTableBytes % 16 == 0, "the pair reads are 16-byte aligned");

struct MiParams : CandidateGrid
{
  double* mi;
  double tab[2 * kMiClasses];  // {h, pass} by class
};

__device__ __forceinline__ int class_of(int v) { return v < 0 ? 0 : (v < 100 ? v : 100) + 1; }

// the launch's table into LDS (the caller synchronises before the first read)
__device__ __forceinline__ void stage_table(const MiParams& p, double* s_tab)
{
  for (int n = threadIdx.x; n < 2 * kMiClasses; n += kGainBlock) s_tab[n] = p.tab[n];
}

__global__ __launch_bounds__(kGainBlock) void mi_field_lds_kernel(const MiParams p)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char s_mem[];  // the table, then [H][W] class bytes
  double2* const s_tab = reinterpret_cast<double2*>(s_mem);
  unsigned char* const s_win = s_mem + kMiTableBytes;
  const int R = p.R, W = p.W, tid = threadIdx.x;
  const int st = static_cast<int>(p.stride);  // (small: the window fits 64 KB)
  const int base = ((tid / kGainTX) * st + R) * W + (tid % kGainTX) * st + R;
  stage_table(p, reinterpret_cast<double*>(s_mem));
  for (unsigned long long t = blockIdx.x; t < p.tiles; t += gridDim.x) {
    __syncthreads();  // the tile before has read the window
    const Tile k = tile_of(p, t);
    stage_window(p, k, s_win, kMiOffGrid, [](int v) { return class_of(v); });
    zero_off_lattice(p, k, p.mi);
    __syncthreads();
    const size_t g0 = static_cast<size_t>(k.i0) * p.c.xsize + k.j0;  // (cell (0, 0) for a lane without a candidate)
    const bool cand = k.in && p.known[g0] < p.cutoff;                // a robot cannot stand in a blocking cell
    double total = cand ? s_tab[s_win[base]].x : 0.0;                // (base: inside the window for every lane)
    if (__builtin_amdgcn_ballot_w64(cand) != 0) {
      for (int q = 0; q < 8 * R; ++q) {
        Ray ray(q, R);  // (the same in every lane: scalar registers)
        double reach = cand ? 1.0 : 0.0, beam = 0.0;
        // kGainChunk steps at a time: their class bytes are read before the first pair is, the pairs before the first is used
        for (int s0 = 1; s0 <= R; s0 += kGainChunk) {
          int cls[kGainChunk];
          double2 hp[kGainChunk];
          bool ended = false;
#pragma unroll
          for (int u = 0; u < kGainChunk; ++u) {
            ray.step(R);
            const bool in = s0 + u <= R && ray.in_disc(R);  // (uniform; the steps in the disc are a prefix of the ray)
            ended = ended || !in;
            // |dx|, |dy| <= R while s <= R: inside the padded window; a step past the ray's end reads the lane's own cell and
            // takes the off-grid pair {0, 0}, which ends the ray for every lane
            const int c = s_win[base + (in ? ray.dy * W + ray.dx : 0)];
            cls[u] = in ? c : kMiOffGrid;
          }
#pragma unroll
          for (int u = 0; u < kGainChunk; ++u) hp[u] = s_tab[cls[u]];
#pragma unroll
          for (int u = 0; u < kGainChunk; ++u) {
            beam = beam + reach * hp[u].x;
            reach = reach * hp[u].y;  // a blocking cell contributes, then ends the ray: its pass is +0.0
          }
          if (ended || __builtin_amdgcn_ballot_w64(reach > 0.0) == 0) break;
        }
        total = total + beam;
      }
    }
    if (k.in) p.mi[g0] = total;
  }
}

__global__ __launch_bounds__(kGainBlock) void mi_field_global_kernel(const MiParams p)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char s_mem[];  // the table
  const double2* const s_tab = reinterpret_cast<const double2*>(s_mem);
  const int R = p.R;
  stage_table(p, reinterpret_cast<double*>(s_mem));
  __syncthreads();
  for (unsigned long long t = blockIdx.x; t < p.tiles; t += gridDim.x) {
    const Tile k = tile_of(p, t);
    zero_off_lattice(p, k, p.mi);
    if (!k.in) continue;
    const size_t g0 = static_cast<size_t>(k.i0) * p.c.xsize + k.j0;
    const int own = p.known[g0];
    double total = 0.0;
    if (own < p.cutoff) {
      total = s_tab[class_of(own)].x;
      const Clip w = clip_of(p.c, k.i0, k.j0, R);
      for (int q = 0; q < 8 * R; ++q) {
        double reach = 1.0, beam = 0.0;
        (void)march(q, R, w, [&](int dx, int dy) {
          const int v = p.known[cell_index(p.c, k.i0, k.j0, dx, dy)];
          const double2 hp = s_tab[class_of(v)];
          const bool blocks = v >= p.cutoff;
          beam = beam + reach * hp.x;
          reach = blocks ? 0.0 : reach * hp.y;
          return blocks;
        });
        total = total + beam;
      }
    }
    p.mi[g0] = total;
  }
}

// the value grid of eea_set_target_mi: (real)(mi + floor) on the candidates whose cell does not block, 0 elsewhere
// (gain_tile.hpp: candidate_values; the cell is a double already)
template <typename R>
__global__ __launch_bounds__(kGainBlock) void mi_values_kernel(const int8_t* __restrict__ known, const double* __restrict__ mi,
                                                               unsigned xsize, unsigned ysize, unsigned stride, int cutoff, double floor,
                                                               R* __restrict__ out)
{
  candidate_values<R, double, false>(known, mi, nullptr, xsize, ysize, stride, cutoff, floor, out);
}
}  // namespace

hipError_t launch_mi_field(const CollisionParams& c, unsigned range_cells, unsigned stride, double p_unknown, const int8_t* d_known,
                           double* d_mi, hipStream_t s)
{
  MiParams p;
  size_t window = 0;
  const unsigned blocks = candidate_grid(c, range_cells, stride, d_known, kMiTableBytes, p, &window);
  p.mi = d_mi;
  double h[256], pass[256];
  mi_table256(c.occupied_threshold, p_unknown, h, pass);
  for (int cl = 0; cl < kMiClasses; ++cl) {
    // class 0: the negative values share h; of pass they share the one of -128, the last of them to block -- every negative
    // value's when the LDS form runs, and in the global form that of those that do not block (which is all it reads)
    const int v = cl == 0 ? -128 : cl - 1;
    p.tab[2 * cl] = cl == kMiOffGrid ? 0.0 : h[v + 128];
    p.tab[2 * cl + 1] = cl == kMiOffGrid ? 0.0 : pass[v + 128];
  }
  // classes are all the LDS form knows of a cell: with a cutoff among the negative values some of class 0 block, some do not
  const bool classes_suffice = p.cutoff >= 0 || p.cutoff == -128;
  if (window != 0 && classes_suffice) {
    hipLaunchKernelGGL(mi_field_lds_kernel, dim3(blocks), dim3(kGainBlock), kMiTableBytes + window, s, p);
  } else {
    hipLaunchKernelGGL(mi_field_global_kernel, dim3(blocks), dim3(kGainBlock), kMiTableBytes, s, p);
  }
  return hipGetLastError();
}

template <typename R>
hipError_t launch_mi_values(const CollisionParams& c, unsigned stride, const int8_t* d_known, const double* d_mi, double floor,
                            R* d_values, hipStream_t s)
{
  hipLaunchKernelGGL(mi_values_kernel<R>, values_grid(c), dim3(kGainBlock), 0, s, d_known, d_mi, c.xsize, c.ysize, stride,
                     blocking_cutoff(c.occupied_threshold), floor, d_values);
  return hipGetLastError();
}
template hipError_t launch_mi_values<double>(const CollisionParams&, unsigned, const int8_t*, const double*, double, double*,
                                             hipStream_t);
template hipError_t launch_mi_values<float>(const CollisionParams&, unsigned, const int8_t*, const double*, double, float*,
                                            hipStream_t);
}  // namespace eea
