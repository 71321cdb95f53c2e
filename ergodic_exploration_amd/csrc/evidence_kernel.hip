// The evidence grid of a simulated fleet (include/ergodic_amd.h, eea_sense_observe_batch / eea_evidence_publish /
// eea_evidence_table): every robot's NOISY scan is fused into a grid of integer log-odds units, and a publication step turns
// the evidence into the int8 occupancy probabilities 1 .. 99 the tick, the census, the gain count and the mutual information
// read.  The sensor is the reveal's (sense_kernel.hip: the rays, the disc and grid tests, blocks(), the robot's cell, the mask,
// all from sense_rays.hpp / grid_cell.hpp); what a ray meets is not the truth but what the robot's scan SEES of it.  This is NOT
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
//    times the reveal).  The noise is applied AT STAGING: bit 0 of a window byte is "appears blocking".  The rays march in LDS through march() as it is and set bit 1 of the cells
//    they touch (every writer of a byte writes the same value); the write-out walks the window's rows and issues one atomic add
//    per touched cell.  Global memory sees each window row once on the way in and at most one atomic per cell on the way out.
//    Only this LDS form is built: R <= 127;
//  - publish: a streaming kernel of the census' form -- 16-byte loads of the evidence, a byte store per cell, the table of
//    2 e_clip + 1 bytes carried in the kernel arguments and staged in LDS, the three counts by wavefront reduction and one
//    integer atomic per workgroup and count.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "common.hpp"
#include "grid_cell.hpp"
#include "philox.hpp"
#include "sense_rays.hpp"  // Clip, clip_of, cell_index, march: the reveal's, unchanged

namespace eea
{
namespace
{
constexpr int kEvidenceBlock = 256;
constexpr unsigned kEvidenceMaxBlocks = 1u << 16;  // workgroups per launch; they stride over the robots past that

struct ObserveParams
{
  CollisionParams c;  // the geometry (the radii are not read)
  int R;
  int cutoff;  // a truth cell blocks iff cell >= cutoff (128: no cell does)
  int w_occ, w_free;
  uint32_t thr_miss, thr_false, seed_lo, seed_hi;
  unsigned scan, robot0;
  const int8_t* truth;
  int32_t* evid;
  const double* pose;  // [P][3]
  const int* mask;     // [P] or null
  int* ranges;         // [P][8R] or null
  unsigned P;
};

// the robot of this workgroup's turn, as the reveal takes it: false when the mask leaves it out or its cell is off the grid
// (its row of ranges is then -1)
__device__ __forceinline__ bool observer_cell(const ObserveParams& p, unsigned b, unsigned& i0, unsigned& j0)
{
  if (p.mask != nullptr && p.mask[b] == 0) return false;
  world_to_grid(p.c, p.pose[3 * static_cast<size_t>(b)], p.pose[3 * static_cast<size_t>(b) + 1], j0, i0);
  if ((i0 <= p.c.ysize - 1u) && (j0 <= p.c.xsize - 1u)) return true;
  if (p.ranges != nullptr) {
    int* const row = p.ranges + static_cast<size_t>(b) * 8u * p.R;
    for (int q = threadIdx.x; q < 8 * p.R; q += kEvidenceBlock) row[q] = -1;
  }
  return false;
}

__global__ __launch_bounds__(kEvidenceBlock) void evidence_observe_kernel(const ObserveParams p)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char s_cell[];  // [2R + 1][2R + 1]: bit 0 appears blocking, bit 1 touched
  const int R = p.R, W = 2 * R + 1, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (unsigned b = blockIdx.x; b < p.P; b += gridDim.x) {
    __syncthreads();  // the robot before has read the window
    unsigned i0, j0;
    if (!observer_cell(p, b, i0, j0)) continue;  // (uniform over the workgroup)
    const Clip w = clip_of(p.c, i0, j0, R);
    // columns jlo .. jhi of the grid, in groups of four that share a Philox call: group = column >> 2
    const unsigned jlo = j0 + static_cast<unsigned>(w.xlo), jhi = j0 + static_cast<unsigned>(w.xhi);
    const unsigned glo = jlo >> 2, robot = p.robot0 + b;
    // the window's groups, row after row, dealt to the 256 threads in turn: neighbouring lanes read neighbouring groups of a
    // row (a wavefront covers a row of 64 groups, or several shorter rows), and a thread's next group lies 256 further on
    const unsigned per_row = (jhi >> 2) - glo + 1u;  // <= 65: a row of 2R + 1 <= 255 cells
    const unsigned rows = static_cast<unsigned>(w.yhi - w.ylo) + 1u;
    const unsigned skip_rows = kEvidenceBlock / per_row, skip_grps = kEvidenceBlock % per_row;
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
    for (int q = tid; q < 8 * R; q += kEvidenceBlock) {
      const int range = march(q, R, w, [&](int dx, int dy) {
        unsigned char* const cell = s_cell + (dy + R) * W + (dx + R);
        const unsigned char v = *cell;
        if (v < 2) *cell = v | 2;
        return (v & 1) != 0;
      });
      if (p.ranges != nullptr) p.ranges[static_cast<size_t>(b) * 8u * R + q] = range;
    }
    __syncthreads();
    for (int dy = w.ylo + wave; dy <= w.yhi; dy += kEvidenceBlock / 64) {
      int32_t* const erow = p.evid + cell_index(p.c, i0, j0, 0, dy);
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

struct Census
{
  unsigned unknown, below, blocking;
};

// one cell: its byte is stored and counted
__device__ __forceinline__ void publish_cell(const PublishParams& p, const int8_t* s_table, size_t at, int e, Census& n)
{
  const int c = e < -p.e_clip ? -p.e_clip : e > p.e_clip ? p.e_clip : e;
  const int v = e == 0 ? -1 : s_table[c + p.e_clip];
  p.known[at] = static_cast<int8_t>(v);
  n.unknown += v < 0 ? 1u : 0u;
  n.below += (v >= 0 && v < p.cutoff) ? 1u : 0u;
  n.blocking += v >= p.cutoff ? 1u : 0u;
}

// 16 bytes (four cells) per load from the evidence's first 16-byte boundary on; the cells in front of it and behind the last
// whole load one by one (at most 3 each: the first threads of the launch take them).  `known` is written in bytes: it may
// start anywhere
__global__ __launch_bounds__(kEvidenceBlock) void evidence_publish_kernel(const PublishParams p)
{
  __shared__ uint32_t s_words[kTableWords];
  __shared__ unsigned s_part[kEvidenceBlock / 64][3];
  for (int k = threadIdx.x; k < kTableWords; k += kEvidenceBlock) s_words[k] = p.table[k];
  __syncthreads();
  const int8_t* const s_table = reinterpret_cast<const int8_t*>(s_words);
  size_t head = ((16u - (reinterpret_cast<uintptr_t>(p.evid) & 15u)) & 15u) / 4u;
  if (head > p.n) head = p.n;
  const size_t chunks = (p.n - head) / 4u, tail0 = head + chunks * 4u;
  const size_t t = static_cast<size_t>(blockIdx.x) * kEvidenceBlock + threadIdx.x, stride = static_cast<size_t>(gridDim.x) * kEvidenceBlock;
  Census cnt{ 0u, 0u, 0u };
  const int4* const body = reinterpret_cast<const int4*>(p.evid + head);
  for (size_t ch = t; ch < chunks; ch += stride) {
    const int4 v = body[ch];
    const size_t at = head + 4u * ch;
    publish_cell(p, s_table, at, v.x, cnt);
    publish_cell(p, s_table, at + 1, v.y, cnt);
    publish_cell(p, s_table, at + 2, v.z, cnt);
    publish_cell(p, s_table, at + 3, v.w, cnt);
  }
  if (t < head) publish_cell(p, s_table, t, p.evid[t], cnt);
  if (t < p.n - tail0) publish_cell(p, s_table, tail0 + t, p.evid[tail0 + t], cnt);
  if (p.counts == nullptr) return;  // (uniform over the launch)
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    cnt.unknown += __shfl_down(cnt.unknown, d, 64);
    cnt.below += __shfl_down(cnt.below, d, 64);
    cnt.blocking += __shfl_down(cnt.blocking, d, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    s_part[threadIdx.x >> 6][0] = cnt.unknown;
    s_part[threadIdx.x >> 6][1] = cnt.below;
    s_part[threadIdx.x >> 6][2] = cnt.blocking;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    unsigned long long sum = 0;
    for (int wv = 0; wv < kEvidenceBlock / 64; ++wv) sum += s_part[wv][threadIdx.x];
    if (sum != 0) atomicAdd(p.counts + threadIdx.x, sum);  // integers: any order of the workgroups gives the same sums
  }
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
  p.c = c;
  p.R = static_cast<int>(range_cells);
  p.cutoff = blocking_cutoff(c.occupied_threshold);
  p.w_occ = ev.w_occ;
  p.w_free = ev.w_free;
  p.thr_miss = ev.thr_miss;
  p.thr_false = ev.thr_false;
  p.seed_lo = ev.seed_lo;
  p.seed_hi = ev.seed_hi;
  p.scan = scan;
  p.robot0 = robot0;
  p.truth = d_truth;
  p.evid = d_evid;
  p.pose = d_pose;
  p.mask = d_mask;
  p.ranges = d_ranges;
  p.P = P;
  const unsigned blocks = P < kEvidenceMaxBlocks ? P : kEvidenceMaxBlocks;
  const size_t W = 2 * static_cast<size_t>(range_cells) + 1;
  hipLaunchKernelGGL(evidence_observe_kernel, dim3(blocks), dim3(kEvidenceBlock), W * W, s, p);
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
  const size_t want = (p.n / 4u + kEvidenceBlock - 1) / kEvidenceBlock + 1;  // (+ 1: the head and tail cells when there is no whole load)
  // every workgroup of a counting launch ends in three atomics on the same three counters: fewer, longer workgroups then
  const size_t most = d_counts != nullptr ? 256u : 2048u;
  const unsigned blocks = static_cast<unsigned>(want < most ? want : most);
  hipLaunchKernelGGL(evidence_publish_kernel, dim3(blocks), dim3(kEvidenceBlock), 0, s, p);
  return hipGetLastError();
}
}  // namespace eea
