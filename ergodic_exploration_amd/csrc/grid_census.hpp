// The census of a grid of int8 cell values -- how many are unknown (< 0), known below the blocking cutoff, blocking -- and the
// shape of a kernel that streams an array in 16-byte loads: the ONE definition grid_census_kernel (sense_kernel.hip) and
// evidence_publish_kernel (evidence_kernel.hip) take both from.  The split is plain integer code and compiles on the host
// (tests/sense_rays_check.cpp drives it).
#pragma once

#include <cstddef>
#include <cstdint>

#include "common.hpp"

namespace eea
{
// n elements of SIZE bytes from `base` on (a multiple of SIZE): elements [0, head) lie in front of the first 16-byte boundary,
// `chunks` whole 16-byte loads follow, elements [tail0, n) lie behind the last of them.  head and n - tail0 are below
// 16 / SIZE: the first threads of a launch take them one by one
struct StreamSplit
{
  size_t head, chunks, tail0;
};
template <unsigned SIZE>
__host__ __device__ __forceinline__ StreamSplit stream_split(uintptr_t base, size_t n)
{
  static_assert(SIZE == 1u || SIZE == 2u || SIZE == 4u || SIZE == 8u, "elements tile a 16-byte load");
  StreamSplit s;
  s.head = ((16u - (base & 15u)) & 15u) / SIZE;
  if (s.head > n) s.head = n;
  s.chunks = (n - s.head) / (16u / SIZE);
  s.tail0 = s.head + s.chunks * (16u / SIZE);
  return s;
}

struct Census
{
  unsigned unknown, below, blocking;
};
__host__ __device__ __forceinline__ void count_value(Census& n, int v, int cutoff)
{
  n.unknown += v < 0 ? 1u : 0u;
  n.below += (v >= 0 && v < cutoff) ? 1u : 0u;
  n.blocking += v >= cutoff ? 1u : 0u;
}

#if defined(__HIPCC__)
// the counts of a workgroup of kBlock threads into counts [3] (zeroed on the stream): a shuffle reduction per wavefront, 48
// bytes of LDS across the four, one 64-bit atomic per count that is not zero.  Every thread of the workgroup calls it
__device__ __forceinline__ void census_commit(Census cnt, unsigned long long* __restrict__ counts)
{
  __shared__ unsigned s_part[kBlock / kWave][3];
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
    for (int wv = 0; wv < kBlock / kWave; ++wv) sum += s_part[wv][threadIdx.x];
    if (sum != 0) atomicAdd(counts + threadIdx.x, sum);  // integers: any order of the workgroups gives the same sums
  }
}
#endif
}  // namespace eea
