// The evidence grid of a simulated fleet (include/ergodic_amd.h, eea_sense_observe_batch / eea_evidence_publish /
// eea_evidence_table): every robot's NOISY scan is fused into a grid of integer log-odds units, and a publication step turns
// the evidence into the int8 occupancy probabilities 1 .. 99 the tick, the census, the gain count and the mutual information
// read.  The sensor is the reveal's (sense_kernel.hip): the rays, the disc and grid tests, the launch block (ScanParams), the
// robot of a workgroup's turn with the mask and the off-grid rule (robot_cell) and the march on the staged window
// (march_window) are sense_rays.hpp's, one definition for both; what a ray meets is not the truth but what the robot's scan
// SEES of it: this file keeps the staging (the noise) and the write-out (the atomic adds).  This is NOT
// the reference's OccupancyMapper (mapping.cpp), whose per-update int8 round trip makes the result depend on the order of
// every beam: it borrows its sensor-model constants and logOdds2Prob (mapping.cpp:51-54, 66-74) and nothing else.
//
//  - order-free: a robot adds +w_occ or -w_free ONCE to every cell its scan touched, with integer atomics; int32 adds commute,
//    so robots, rays, workgroups and calls may come in any order;
//  - counter-based noise: what robot g sees of cell (i, j) in scan `scan` is word j & 3 of Philox4x32-10 (philox.hpp) at the
//    counter (j >> 2, i, g, scan): one outcome per (robot, scan, cell), whichever ray gets there, and one call serves four
//    neighbouring cells of a row;
//  - observe: the reveal's shape -- one workgroup of 256 threads per robot, the clipped (2R + 1)^2 window in LDS as one byte
//    per cell, rows read coalesced (a lane per group of four columns; a wavefront takes a row of 64 groups, or several shorter
//    rows at once: with a wavefront per row a window of 21 columns kept 6 lanes of 64 busy with Philox and the scan cost 1.6
//    times the reveal).  The noise is applied AT STAGING: bit 0 of a window byte is "appears blocking".  The rays
//    march in LDS through the reveal's march_window and set bit 1 of the cells they touch (every writer of a byte writes the
//    same value); the write-out walks the window's rows and issues one atomic add per touched cell.  Global memory sees each
//    window row once on the way in and at most one atomic per cell on the way out.  Only this LDS form is built: R <= 127;
//  - publish: a streaming kernel of the census' form, from the census' pieces (grid_census.hpp: stream_split, count_value,
//    census_commit) -- 16-byte loads of the evidence, a byte store per cell, the table of 2 e_clip + 1 bytes carried in the
//    kernel arguments and staged in LDS, the three counts by wavefront reduction and one integer atomic per workgroup and count.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "common.hpp"
#include "grid_census.hpp"  // Census, count_value, census_commit, stream_split: shared with sense_kernel.hip
#include "philox.hpp"
#include "sense_rays.hpp"  // the rays, and with sense_kernel.hip ScanParams, scan_launch, robot_cell, march_window

namespace eea
{
namespace
{
struct ObserveParams : ScanParams<int32_t>  // out: the evidence
{
  int w_occ, w_free;
  uint32_t thr_miss, thr_false, seed_lo, seed_hi;
  unsigned scan, robot0;
};

__global__ __launch_bounds__(kBlock) void evidence_observe_kernel(const ObserveParams p)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char s_cell[];  // [2R + 1][2R + 1]: bit 0 appears blocking, bit 1 touched
  const int R = p.R, W = 2 * R + 1, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (unsigned b = blockIdx.x; b < p.P; b += gridDim.x) {
    __syncthreads();  // the robot before has read the window
    unsigned i0, j0;
    if (!robot_cell(p, b, i0, j0)) continue;  // (uniform over the workgroup)
    const Clip w = clip_of(p.c, i0, j0, R);
    // columns jlo .. jhi of the grid, in groups of four that share a Philox call: group = column >> 2
    const unsigned jlo = j0 + static_cast<unsigned>(w.xlo), jhi = j0 + static_cast<unsigned>(w.xhi);
    const unsigned glo = jlo >> 2, robot = p.robot0 + b;
    // the window's groups, row after row, dealt to the 256 threads in turn: neighbouring lanes read neighbouring groups of a
    // row (a wavefront covers a row of 64 groups, or several shorter rows), and a thread's next group lies 256 further on
    const unsigned per_row = (jhi >> 2) - glo + 1u;  // <= 65: a row of 2R + 1 <= 255 cells
    const unsigned rows = static_cast<unsigned>(w.yhi - w.ylo) + 1u;
    const unsigned skip_rows = kBlock / per_row, skip_grps = kBlock % per_row;
    unsigned row = static_cast<unsigned>(tid) / per_row, at = static_cast<unsigned>(tid) % per_row;
    while (row < rows) {
      const int dy = w.ylo + static_cast<int>(row);
      const unsigned i = i0 + static_cast<unsigned>(dy), grp = glo + at;
      const int8_t* const trow = p.truth + static_cast<size_t>(i) * p.c.xsize;
      unsigned char* const srow = s_cell + (dy + R) * W + R;
      const Philox r = philox4x32_10(grp, i, robot, p.scan, p.seed_lo, p.seed_hi);
#pragma unroll
      for (unsigned k = 0; k < 4; ++k) {
        const unsigned j = 4u * grp + k;
        if (j < jlo || j > jhi) continue;
        const bool blocks = trow[j] >= p.cutoff;
        const bool seen = blocks ? !(r.v[k] < p.thr_miss) : (r.v[k] < p.thr_false);
        srow[static_cast<int>(j - j0)] = seen ? 1 : 0;
      }
      row += skip_rows;
      at += skip_grps;
      if (at >= per_row) {
        at -= per_row;
        row += 1u;
      }
    }
    __syncthreads();
    if (tid == 0) s_cell[R * W + R] = 2;  // the robot's own cell: touched, never appears blocking (no ray visits offset (0, 0))
    march_window(p, b, w, s_cell);
    __syncthreads();
    for (int dy = w.ylo + wave; dy <= w.yhi; dy += kBlock / 64) {
      int32_t* const erow = p.out + cell_index(p.c, i0, j0, 0, dy);
      const unsigned char* const srow = s_cell + (dy + R) * W + R;
      for (int dx = w.xlo + lane; dx <= w.xhi; dx += 64) {
        const unsigned char v = srow[dx];
        if (v & 2) atomicAdd(erow + dx, (v & 1) ? p.w_occ : -p.w_free);  // (integers: any order of the robots gives the same sums)
      }
    }
  }
}

// ---- publish ---------------------------------------------------------------------------------
constexpr int kTableWords = (2 * kEvidenceMaxClip + 1 + 3) / 4;  // 513

struct PublishParams
{
  const int32_t* evid;
  int8_t* known;
  unsigned long long* counts;  // [3] or null; zeroed on the stream
  size_t n;
  int e_clip, cutoff;
  uint32_t table[kTableWords];  // the 2 e_clip + 1 bytes of evidence_table, zero behind them
};
static_assert(sizeof(PublishParams) <= 4096, "the publish launch carries its table in the kernel arguments");

// one cell: its byte is stored and counted
__device__ __forceinline__ void publish_cell(const PublishParams& p, const int8_t* s_table, size_t at, int e, Census& n)
{
  const int c = e < -p.e_clip ? -p.e_clip : e > p.e_clip ? p.e_clip : e;
  const int v = e == 0 ? -1 : s_table[c + p.e_clip];
  p.known[at] = static_cast<int8_t>(v);
  count_value(n, v, p.cutoff);
}

// 16 bytes (four cells) per load from the evidence's first 16-byte boundary on; the cells in front of it and behind the last
// whole load one by one (at most 3 each: the first threads of the launch take them).  `known` is written in bytes: it may
// start anywhere
__global__ __launch_bounds__(kBlock) void evidence_publish_kernel(const PublishParams p)
{
  __shared__ uint32_t s_words[kTableWords];
  for (int k = threadIdx.x; k < kTableWords; k += kBlock) s_words[k] = p.table[k];
  __syncthreads();
  const int8_t* const s_table = reinterpret_cast<const int8_t*>(s_words);
  const StreamSplit sp = stream_split<4>(reinterpret_cast<uintptr_t>(p.evid), p.n);
  const size_t t = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x, stride = static_cast<size_t>(gridDim.x) * kBlock;
  Census cnt{ 0u, 0u, 0u };
  const int4* const body = reinterpret_cast<const int4*>(p.evid + sp.head);
  for (size_t ch = t; ch < sp.chunks; ch += stride) {
    const int4 v = body[ch];
    const size_t at = sp.head + 4u * ch;
    publish_cell(p, s_table, at, v.x, cnt);
    publish_cell(p, s_table, at + 1, v.y, cnt);
    publish_cell(p, s_table, at + 2, v.z, cnt);
    publish_cell(p, s_table, at + 3, v.w, cnt);
  }
  if (t < sp.head) publish_cell(p, s_table, t, p.evid[t], cnt);
  if (t < p.n - sp.tail0) publish_cell(p, s_table, sp.tail0 + t, p.evid[sp.tail0 + t], cnt);
  if (p.counts == nullptr) return;  // (uniform over the launch)
  census_commit(cnt, p.counts);
}
}  // namespace

void evidence_table(const EvidenceParams& ev, int8_t* table)
{
  for (int e = -ev.e_clip; e <= ev.e_clip; ++e) {
    const double l = static_cast<double>(e) * ev.quantum;
    const double sigma = 1.0 - 1.0 / (1.0 + std::exp(l));  // logOdds2Prob (mapping.cpp:51-54)
    const double v = std::floor(100.0 * sigma + 0.5);       // to nearest, not the reference's truncation
    table[e + ev.e_clip] = static_cast<int8_t>(v < 1.0 ? 1 : v > 99.0 ? 99 : static_cast<int>(v));
  }
}

hipError_t launch_evidence_observe(const CollisionParams& c, const EvidenceParams& ev, unsigned range_cells, unsigned scan,
                                   unsigned robot0, const int8_t* d_truth, int32_t* d_evid, const double* d_pose, const int* d_mask,
                                   unsigned P, int* d_ranges, hipStream_t s)
{
  if (P == 0) return hipSuccess;
  if (range_cells == 0 || range_cells > kEvidenceMaxR) return hipErrorInvalidValue;  // (the entry has refused it: the window is LDS)
  ObserveParams p;
  size_t window = 0;
  const unsigned blocks = scan_launch(c, range_cells, d_truth, d_evid, d_pose, d_mask, d_ranges, P, p, &window);
  p.w_occ = ev.w_occ;
  p.w_free = ev.w_free;
  p.thr_miss = ev.thr_miss;
  p.thr_false = ev.thr_false;
  p.seed_lo = ev.seed_lo;
  p.seed_hi = ev.seed_hi;
  p.scan = scan;
  p.robot0 = robot0;
  hipLaunchKernelGGL(evidence_observe_kernel, dim3(blocks), dim3(kBlock), window, s, p);
  return hipGetLastError();
}

hipError_t launch_evidence_publish(const CollisionParams& c, const EvidenceParams& ev, const int32_t* d_evid, int8_t* d_known,
                                   unsigned long long* d_counts, hipStream_t s)
{
  if (ev.e_clip < 1 || ev.e_clip > kEvidenceMaxClip) return hipErrorInvalidValue;  // (the entry has refused it: the table's size)
  // the table of the last (e_clip, quantum) of this thread: a repeated call evaluates no exp
  struct Cached
  {
    bool valid = false;
    int e_clip = 0;
    double quantum = 0.0;
    uint32_t words[kTableWords];
  };
  static thread_local Cached cache;
  if (!cache.valid || cache.e_clip != ev.e_clip || cache.quantum != ev.quantum) {
    int8_t bytes[4 * kTableWords] = {};
    evidence_table(ev, bytes);
    std::memcpy(cache.words, bytes, sizeof(cache.words));
    cache.e_clip = ev.e_clip;
    cache.quantum = ev.quantum;
    cache.valid = true;
  }
  PublishParams p;
  p.evid = d_evid;
  p.known = d_known;
  p.counts = d_counts;
  p.n = static_cast<size_t>(c.xsize) * c.ysize;
  p.e_clip = ev.e_clip;
  p.cutoff = blocking_cutoff(c.occupied_threshold);
  std::memcpy(p.table, cache.words, sizeof(p.table));
  if (d_counts != nullptr) {
    const hipError_t e = hipMemsetAsync(d_counts, 0, 3 * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
  }
  const size_t want = (p.n / 4u + kBlock - 1) / kBlock + 1;  // (+ 1: the head and tail cells when there is no whole load)
  // every workgroup of a counting launch ends in three atomics on the same three counters: fewer, longer workgroups then
  const size_t most = d_counts != nullptr ? 256u : 2048u;
  const unsigned blocks = static_cast<unsigned>(want < most ? want : most);
  hipLaunchKernelGGL(evidence_publish_kernel, dim3(blocks), dim3(kBlock), 0, s, p);
  return hipGetLastError();
}
}  // namespace eea
