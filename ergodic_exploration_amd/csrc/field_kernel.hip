// Coverage fields (include/ergodic_amd.h, eea_records_field): sum records taken back to the target grid -- the synthesis that
// belongs to the analysis of phik_kernel.hip.  Per record F = CX^T A CY^T on the grid configTarget builds
// (ergodic_control.hpp:387-408): CX[k1][i] = cos((k1 pi / lx) x_i), CY[r][k2] = cos((k2 pi / ly) y_r) are the axis tables the
// phi_k path uses (axis_tables_kernel, the expression of basis.cpp:85), built once per (nx, ny_total, lx, ly) by the engine and
// read here; A[k2 K + k1] = a_m is formed from the record, phi_k and lamda_k per workgroup.  The reference has
// no counterpart: it publishes its target as markers (target.hpp Target::markers) and never forms c_k of its whole history.
//
//  - a workgroup owns (record, tile of <= rt rows, tile of <= 128 columns): it stages its columns of CX and the record's A
//    in LDS, forms W[k1][r] = sum_k2 A[k2 K + k1] CY[r][k2] for its rows once (k2 ascending), then every output element is
//    sum_k1 CX[k1][i] W[k1][r], k1 ascending, one fma per mode: a pure function of the record, the domain, phi_k and (r, i).
//    Neither the tiling (rt, the row range asked for) nor the record's place in the batch enters the arithmetic;
//  - a thread's item is 16 bytes of x (2 doubles / 4 floats) of 4 rows: per mode it reads the columns once for the 4 rows
//    and the 4 W values once for the columns, (VEC + 4) LDS reads for 4 VEC fmas;
//  - stores are 16 bytes where the ADDRESS allows: the rows of an odd-length grid (121, the shipped one) start on every
//    alignment in turn, so the rows of a tile are taken in classes of equal alignment (row, row + period, ..: period =
//    16 bytes / gcd(row length in bytes, 16 bytes) rows); a class's rows share the head (elements before the first 16-byte
//    boundary, stored one by one), the aligned body and the tail (one by one).  No store straddles a boundary, no element
//    has two writers, no atomics;
//  - the cost at fleet size is the output's write traffic (4096 x 121 x 61 x 8 B = 242 MB against 0.6 Gflop at K = 10).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "abi_util.hpp"
#include "common.hpp"

namespace eea
{
namespace
{
constexpr int kFieldXT = 128;     // columns of CX a workgroup stages
constexpr int kFieldRows = 64;    // rows per workgroup at most (rt; the launcher takes fewer when there are few tiles)
constexpr int kFieldMinRows = 16;
constexpr int kFieldRB = 4;       // rows per thread item
constexpr unsigned kFieldMaxBlocks = 1u << 16;  // workgroups per launch; they stride over the tiles past that

template <typename R>
struct FieldParams
{
  const R* rec;     // [n_rec][rec_len]
  const R* phik;    // [K^2]
  const R* lamdak;  // [K^2]
  const R* cx;      // [K][nx]
  const R* cy;      // [ny_total][K]
  R* out;           // [n_rec][nrows][nx]
  int kind, K, rec_len;
  unsigned nx, row0, nrows, rt, xtiles, rtiles;
  unsigned period;  // rows between two rows of equal store alignment
  unsigned obase;   // (out / sizeof(R)) mod VEC
  R area;           // lx * ly
  unsigned long long tiles;  // n_rec * rtiles * xtiles
};

template <typename R>
__device__ __forceinline__ R fma_r(R a, R b, R c);
template <>
__device__ __forceinline__ double fma_r<double>(double a, double b, double c)
{
  return fma(a, b, c);
}
template <>
__device__ __forceinline__ float fma_r<float>(float a, float b, float c)
{
  return fmaf(a, b, c);
}

template <typename R>
__global__ void __launch_bounds__(kBlock) records_field_kernel(FieldParams<R> q)
{
  constexpr int VEC = 16 / static_cast<int>(sizeof(R));
  typedef R vec_t __attribute__((ext_vector_type(VEC)));
  extern __shared__ __attribute__((aligned(16))) unsigned char field_lds[];
  const int K = q.K, K2 = K * K, tid = threadIdx.x;
  const int rt = static_cast<int>(q.rt);
  R* const s_cx = reinterpret_cast<R*>(field_lds);  // [K][kFieldXT]
  R* const s_w = s_cx + K * kFieldXT;               // [K][rt]
  R* const s_a = s_w + K * rt;                      // [K^2]

  for (unsigned long long tile = blockIdx.x; tile < q.tiles; tile += gridDim.x) {
    const unsigned xt = static_cast<unsigned>(tile % q.xtiles);
    const unsigned long long t2 = tile / q.xtiles;
    const unsigned rti = static_cast<unsigned>(t2 % q.rtiles);
    const size_t j = static_cast<size_t>(t2 / q.rtiles);
    const unsigned x0 = xt * kFieldXT, r0 = rti * q.rt;
    const int w = static_cast<int>(q.nx - x0 < static_cast<unsigned>(kFieldXT) ? q.nx - x0 : kFieldXT);
    const int h = static_cast<int>(q.nrows - r0 < q.rt ? q.nrows - r0 : q.rt);
    __syncthreads();  // the tile before has read the LDS images

    // a_m of the record: c_m = rec[m] / rec[K^2], 0 where the count is not positive (the rule of records_metric_kernel)
    const R* const rj = q.rec + j * q.rec_len;
    const R n = rj[K2];
    const bool counted = n > R(0);
    for (int m = tid; m < K2; m += kBlock) {
      const int k2 = m / K, k1 = m - k2 * K;
      const R c = counted ? rj[m] / n : R(0);
      R a;
      if (q.kind == EEA_FIELD_POTENTIAL) {
        a = q.lamdak[m] * (c - q.phik[m]);
      } else {
        // 1 / |cos(k pi x / l)|^2 over [0, l] = w_k / l: w_0 = 1, w_k = 2
        const R wgt = static_cast<R>((k1 > 0 ? 2 : 1) * (k2 > 0 ? 2 : 1));
        a = wgt * (q.kind == EEA_FIELD_DENSITY ? c : q.phik[m] - c) / q.area;
      }
      s_a[m] = a;
    }
    for (int idx = tid; idx < K * w; idx += kBlock) {
      const int k = idx / w, i = idx - k * w;
      s_cx[k * kFieldXT + i] = q.cx[static_cast<size_t>(k) * q.nx + x0 + i];
    }
    __syncthreads();
    for (int idx = tid; idx < K * h; idx += kBlock) {
      const int k1 = idx / h, r = idx - k1 * h;
      const R* const cyr = q.cy + static_cast<size_t>(q.row0 + r0 + r) * K;  // the table is indexed by the GRID row
      R acc = R(0);
      for (int k2 = 0; k2 < K; ++k2) acc = fma_r(s_a[k2 * K + k1], cyr[k2], acc);
      s_w[k1 * rt + r] = acc;
    }
    __syncthreads();

    const size_t rows_before = j * q.nrows + r0;  // output rows in front of the tile's first
    const int P = static_cast<int>(q.period);
    for (int cls = 0; cls < P && cls < h; ++cls) {
      // the rows cls, cls + P, .. of the tile: element x0 of each sits `mis` reals past a 16-byte boundary
      const size_t e_first = (rows_before + cls) * q.nx + x0;
      const int mis = static_cast<int>((q.obase + e_first) & (VEC - 1));
      int head = (VEC - mis) & (VEC - 1);
      head = head < w ? head : w;
      const int nslots = 1 + (w - head + VEC - 1) / VEC;  // slot 0: the head (possibly empty); then 16 bytes each, the last one short
      const int nrows_c = (h - cls + P - 1) / P;
      const int nitems = ((nrows_c + kFieldRB - 1) / kFieldRB) * nslots;
      for (int item = tid; item < nitems; item += kBlock) {
        const int g = item / nslots, s = item - g * nslots;
        const int i0 = s ? head + (s - 1) * VEC : 0;
        const int len = s ? (w - i0 < VEC ? w - i0 : VEC) : head;
        if (len == 0) continue;
        int col[VEC], row[kFieldRB];
#pragma unroll
        for (int v = 0; v < VEC; ++v) col[v] = i0 + v < w ? i0 + v : w - 1;  // past the slot's end: a valid column, not stored
#pragma unroll
        for (int t = 0; t < kFieldRB; ++t) {
          const int r = cls + P * (kFieldRB * g + t);
          row[t] = r < h ? r : h - 1;  // past the tile's end: a valid row, not stored
        }
        R acc[kFieldRB][VEC];
#pragma unroll
        for (int t = 0; t < kFieldRB; ++t)
#pragma unroll
          for (int v = 0; v < VEC; ++v) acc[t][v] = R(0);
        for (int k1 = 0; k1 < K; ++k1) {
          R cv[VEC], wv[kFieldRB];
#pragma unroll
          for (int v = 0; v < VEC; ++v) cv[v] = s_cx[k1 * kFieldXT + col[v]];
#pragma unroll
          for (int t = 0; t < kFieldRB; ++t) wv[t] = s_w[k1 * rt + row[t]];
#pragma unroll
          for (int t = 0; t < kFieldRB; ++t)
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[t][v] = fma_r(cv[v], wv[t], acc[t][v]);
        }
#pragma unroll
        for (int t = 0; t < kFieldRB; ++t) {
          const int r = cls + P * (kFieldRB * g + t);
          if (r >= h) break;
          R* const dst = q.out + (rows_before + r) * q.nx + x0 + i0;
          if (len == VEC) {
            vec_t val;
#pragma unroll
            for (int v = 0; v < VEC; ++v) val[v] = acc[t][v];
            *reinterpret_cast<vec_t*>(dst) = val;
          } else {
#pragma unroll
            for (int v = 0; v < VEC; ++v)
              if (v < len) dst[v] = acc[t][v];
          }
        }
      }
    }
  }
}
}  // namespace

template <typename R>
hipError_t launch_records_field(int kind, unsigned n_rec, const R* d_rec, int K, const R* d_phik, const R* d_lamdak,
                                const R* d_cx, const R* d_cy, unsigned nx, unsigned row0, unsigned nrows, R area, R* d_out,
                                hipStream_t s)
{
  constexpr unsigned VEC = 16 / sizeof(R);
  FieldParams<R> q;
  q.rec = d_rec;
  q.phik = d_phik;
  q.lamdak = d_lamdak;
  q.cx = d_cx;
  q.cy = d_cy;
  q.out = d_out;
  q.kind = kind;
  q.K = K;
  q.rec_len = ck_record_len(K * K);
  q.nx = nx;
  q.row0 = row0;
  q.nrows = nrows;
  q.xtiles = (nx + kFieldXT - 1) / kFieldXT;
  // rows per workgroup: 64, fewer while the launch would leave most of the device without a tile (the arithmetic of an
  // element does not depend on it)
  unsigned rt = kFieldRows;
  while (rt > kFieldMinRows && static_cast<unsigned long long>(n_rec) * q.xtiles * ((nrows + rt - 1) / rt) < 512ull) rt /= 2;
  q.rt = rt;
  q.rtiles = (nrows + rt - 1) / rt;
  q.tiles = static_cast<unsigned long long>(n_rec) * q.rtiles * q.xtiles;
  unsigned g = nx % VEC, period = VEC;  // period = VEC / gcd(nx mod VEC, VEC)
  for (unsigned d = VEC; d >= 1; d /= 2) {
    if (g % d == 0) {
      period = VEC / d;
      break;
    }
  }
  q.period = period;
  q.obase = static_cast<unsigned>((reinterpret_cast<uintptr_t>(d_out) / sizeof(R)) % VEC);
  q.area = area;
  const unsigned blocks = q.tiles < kFieldMaxBlocks ? static_cast<unsigned>(q.tiles) : kFieldMaxBlocks;
  const size_t lds = sizeof(R) * (static_cast<size_t>(K) * kFieldXT + static_cast<size_t>(K) * rt + static_cast<size_t>(K) * K);
  hipLaunchKernelGGL(records_field_kernel<R>, dim3(blocks), dim3(kBlock), lds, s, q);
  return hipGetLastError();
}

template hipError_t launch_records_field<double>(int, unsigned, const double*, int, const double*, const double*, const double*,
                                                 const double*, unsigned, unsigned, unsigned, double, double*, hipStream_t);
template hipError_t launch_records_field<float>(int, unsigned, const float*, int, const float*, const float*, const float*,
                                                const float*, unsigned, unsigned, unsigned, float, float*, hipStream_t);
}  // namespace eea
