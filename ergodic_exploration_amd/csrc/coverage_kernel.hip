// Coverage of a fleet's history (include/ergodic_amd.h, eea_replay_history_records / eea_records_metric): the sum record of
// every robot's WHOLE stored history -- Basis::trajCoeff (reference basis.cpp:109-120) without the 1/N, over the poses of the
// device replay memory (replay_kernel.hip) -- and the ergodic metric eps = sum_k lamda_k (c_k - phi_k)^2 of any sum record.
// The reference only samples its history (buffer.cpp:64-111); it computes eps nowhere (its gradient: ergodic_control.hpp:419-446).
//
// A recompute from the stored map-frame poses, never a running sum: configTarget changes lx, ly and map_pos whenever the map
// grows (ergodic_control.hpp:362-416), and every term cos(k pi (x - map_x) / lx) changes with them.
//
// History kernel, per robot: C = CX CY^T with CX[k][i] = cos(k pi (x_i - map_x) / lx), a K x n by n x K product of two
// cosine tables that never exist in memory:
//  - one WAVEFRONT (= one workgroup) owns a robot, as in replay_sample_kernel; lanes run along the pose index, a pass takes
//    64 consecutive poses: the store row [capacity][3] is read once, 1536 contiguous bytes per pass (theta comes along in the
//    cache lines and is not used); the next pass's poses are requested before this pass's arithmetic;
//  - per pose one cos per axis (sincospi_r: exact argument reduction) and the Chebyshev recurrence cos((k + 1) a) =
//    2 cos a cos(k a) - cos((k - 1) a) the control kernels use, two modes per 16-byte LDS store into a [pose][mode] tile;
//  - the contraction on the matrix cores: v_mfma_f64_16x16x4_f64 (fp32 engines: v_mfma_f32_16x16x4_f32), 4 poses per
//    instruction, K padded to 16-mode tiles (K <= 16: one tile, K = 20: 2 x 2) -- the pad columns of the LDS tile are zeroed
//    once and never written, the rows of poses past the count are zero, groups of 4 poses past the count are not issued;
//  - fixed order: passes in order, within a pass the groups of 4 poses alternate between two accumulators (even / odd
//    group), which are added at the end.  A robot's record is a pure function of its poses, its count and the domain: it does
//    not depend on B, on the robot's index or on the other robots, so a shard of a fleet gives the bits the whole fleet gives;
//  - plain stores only, no atomics: the wavefront owns its record row.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "abi_util.hpp"
#include "common.hpp"

namespace eea
{
namespace
{
constexpr int kCovWave = 64;   // lanes = poses per pass
constexpr int kCovGroups = 16;  // groups of 4 poses (one matrix instruction per tile) per pass

template <typename R>
struct HistoryParams
{
  const R* store;         // [B][capacity][3]
  const unsigned* count;  // [B]
  R* rec;                 // [B][rec_len]
  unsigned capacity;
  int K, rec_len;
  R map_x, map_y, inv_lx, inv_ly;
};

__device__ __forceinline__ void cov_lds_fence()
{
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <typename R>
__device__ __forceinline__ void store_pair(R* dst, R a, R b);
template <>
__device__ __forceinline__ void store_pair<double>(double* dst, double a, double b)
{
  *reinterpret_cast<double2*>(dst) = double2{ a, b };
}
template <>
__device__ __forceinline__ void store_pair<float>(float* dst, float a, float b)
{
  *reinterpret_cast<float2*>(dst) = float2{ a, b };
}

// NT: 16-mode tiles per axis (K <= 16 NT, checked by the launcher)
template <typename R, int NT>
__global__ void __launch_bounds__(kCovWave) history_records_kernel(HistoryParams<R> q)
{
  using M = Mfma<R>;
  using acc_t = typename M::acc_t;
  constexpr int KP = 16 * NT;  // modes per axis after padding
  constexpr int KS = KP + 2;   // row stride of the tiles: even (16-byte stores), and 2 mod 16 spreads the rows over the banks
  __shared__ __attribute__((aligned(16))) R tabx[kCovWave * KS];
  __shared__ __attribute__((aligned(16))) R taby[kCovWave * KS];
  const int lane = threadIdx.x;
  const unsigned b = blockIdx.x;
  const int K = q.K;
  // the pad columns (modes K .. KP - 1 past the last pair the recurrence writes) stay zero for the whole kernel
  for (int i = lane; i < kCovWave * KS; i += kCovWave) {
    tabx[i] = R(0);
    taby[i] = R(0);
  }
  unsigned n = q.count[b];
  n = n < q.capacity ? n : q.capacity;
  const R* const store_b = q.store + 3 * static_cast<size_t>(b) * q.capacity;
  acc_t acc0[NT * NT], acc1[NT * NT];  // even / odd groups of 4 poses
#pragma unroll
  for (int t = 0; t < NT * NT; ++t) acc0[t] = acc1[t] = acc_t{ R(0), R(0), R(0), R(0) };
  const int mk = lane >> 4, mi = lane & 15;  // matrix-instruction operand coordinates of this lane: pose of the group, mode
  const int pairs = (K + 1) / 2;             // 16-byte stores per row
  R* const rowx = tabx + lane * KS;
  R* const rowy = taby + lane * KS;

  R x = R(0), y = R(0);
  if (static_cast<unsigned>(lane) < n) {
    x = store_b[3 * static_cast<size_t>(lane)];
    y = store_b[3 * static_cast<size_t>(lane) + 1];
  }
  for (unsigned base = 0; base < n; base += kCovWave) {
    const bool valid = base + lane < n;
    R sn, cx, cy;
    // the poses as stored, shifted by map_pos as control() shifts the memory columns; nothing is clipped to the domain
    sincospi_r((x - q.map_x) * q.inv_lx, &sn, &cx);
    sincospi_r((y - q.map_y) * q.inv_ly, &sn, &cy);
    const size_t next = static_cast<size_t>(base) + kCovWave + lane;
    if (next < n) {  // the next pass's pose: in flight during this pass's arithmetic
      x = store_b[3 * next];
      y = store_b[3 * next + 1];
    }
    cov_lds_fence();  // the matrix instructions of the pass before have read the tiles
    {
      R ax = valid ? R(1) : R(0), bx = valid ? cx : R(0), ay = ax, by = valid ? cy : R(0);
      const R tx = cx + cx, ty = cy + cy;
      for (int p = 0; p < pairs; ++p) {
        store_pair(rowx + 2 * p, ax, bx);
        store_pair(rowy + 2 * p, ay, by);
        const R nx0 = tx * bx - ax, ny0 = ty * by - ay;
        const R nx1 = tx * nx0 - bx, ny1 = ty * ny0 - by;
        ax = nx0;
        bx = nx1;
        ay = ny0;
        by = ny1;
      }
    }
    cov_lds_fence();
    const unsigned left = n - base;
    const int groups = left >= static_cast<unsigned>(kCovWave) ? kCovGroups : static_cast<int>((left + 3) / 4);  // wavefront-uniform
    for (int m = 0; m < groups; m += 2) {
      {
        const int off = (4 * m + mk) * KS + mi;
#pragma unroll
        for (int t = 0; t < NT * NT; ++t) acc0[t] = M::run(tabx[off + 16 * (t / NT)], taby[off + 16 * (t % NT)], acc0[t]);
      }
      if (m + 1 < groups) {
        const int off = (4 * (m + 1) + mk) * KS + mi;
#pragma unroll
        for (int t = 0; t < NT * NT; ++t) acc1[t] = M::run(tabx[off + 16 * (t / NT)], taby[off + 16 * (t % NT)], acc1[t]);
      }
    }
  }

  // D[k1][k2]: k2 = the lane's column, k1 = the accumulator row of register r; rec[k2 * K + k1], no h_k normalisation
  R* const rec_b = q.rec + static_cast<size_t>(b) * q.rec_len;
#pragma unroll
  for (int t = 0; t < NT * NT; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int k1 = 16 * (t / NT) + M::row(lane, r), k2 = 16 * (t % NT) + mi;
      if (k1 < K && k2 < K) rec_b[k2 * K + k1] = acc0[t][r] + acc1[t][r];
    }
  }
  // element K^2: the robot's count; then the padding, exactly 0
  for (int i = K * K + lane; i < q.rec_len; i += kCovWave) rec_b[i] = (i == K * K) ? static_cast<R>(n) : R(0);
}

// eps of one sum record per wavefront: c_m = rec[m] / rec[K^2] (0 where rec[K^2] <= 0), lane l adds its modes l, l + 64, ..
// in order, then the 64 partial sums meet in a fixed tree
template <typename R>
__global__ void __launch_bounds__(kCovWave) records_metric_kernel(const R* __restrict__ rec, int K2, int rec_len,
                                                                  const R* __restrict__ phik, const R* __restrict__ lamdak,
                                                                  R* __restrict__ metric, R* __restrict__ ck)
{
  const int lane = threadIdx.x;
  const size_t j = blockIdx.x;
  const R* const rj = rec + j * rec_len;
  const R n = rj[K2];
  const bool counted = n > R(0);
  R part = R(0);
  for (int m = lane; m < K2; m += kCovWave) {
    const R c = counted ? rj[m] / n : R(0);
    if (ck != nullptr) ck[j * K2 + m] = c;
    const R d = c - phik[m];
    part += lamdak[m] * d * d;
  }
#pragma unroll
  for (int off = kCovWave / 2; off > 0; off >>= 1) part += __shfl_down(part, off);
  if (lane == 0) metric[j] = part;
}

template <typename R>
hipError_t launch_history(const EngineView& ev, const ReplayView& rv, void* d_rec, hipStream_t s)
{
  HistoryParams<R> q;
  q.store = static_cast<const R*>(rv.d_store);
  q.count = rv.d_count;
  q.rec = static_cast<R*>(d_rec);
  q.capacity = rv.capacity;
  q.K = ev.K;
  q.rec_len = ck_record_len(ev.K * ev.K);
  q.map_x = static_cast<R>(ev.map_x);
  q.map_y = static_cast<R>(ev.map_y);
  q.inv_lx = static_cast<R>(1.0 / ev.lx);
  q.inv_ly = static_cast<R>(1.0 / ev.ly);
  if (ev.K <= 16) {
    hipLaunchKernelGGL((history_records_kernel<R, 1>), dim3(rv.B), dim3(kCovWave), 0, s, q);
  } else {
    hipLaunchKernelGGL((history_records_kernel<R, 2>), dim3(rv.B), dim3(kCovWave), 0, s, q);
  }
  return hipGetLastError();
}

template <typename R>
hipError_t launch_metric(const EngineView& ev, unsigned n_rec, const void* d_rec, void* d_metric, void* d_ck, hipStream_t s)
{
  const int K2 = ev.K * ev.K;
  hipLaunchKernelGGL(records_metric_kernel<R>, dim3(n_rec), dim3(kCovWave), 0, s, static_cast<const R*>(d_rec), K2,
                     ck_record_len(K2), static_cast<const R*>(ev.d_phik), static_cast<const R*>(ev.d_lamdak),
                     static_cast<R*>(d_metric), static_cast<R*>(d_ck));
  return hipGetLastError();
}
}  // namespace
}  // namespace eea

using eea::fail;

extern "C" {

eea_status eea_replay_history_records(eea_engine* e, eea_replay* r, void* d_rec, void* stream)
{
  if (e == nullptr || r == nullptr || d_rec == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  eea::EngineView ev;
  eea::ReplayView rv;
  eea::engine_view(e, &ev);
  eea::replay_view(r, &rv);
  if (rv.real_size != (ev.f32 ? 4u : 8u)) {
    return fail(EEA_ERR_INVALID_ARGUMENT, "the replay memory's real_size is not the engine's");
  }
  if (rv.device != ev.device) return fail(EEA_ERR_INVALID_ARGUMENT, "the replay memory and the engine are on different devices");
  if (!(ev.lx > 0.0) || !(ev.ly > 0.0)) return fail(EEA_ERR_NO_TARGET, "no domain: call eea_config_domain or eea_set_target_grid first");
  if (ev.K > 32) return fail(EEA_ERR_UNSUPPORTED, "history records: K <= 32");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const eea_status st = eea::engine_enter(e, s);  // the device, and behind a rebuild that was only enqueued on another stream
  if (st != EEA_OK) return st;
  EEA_HIP(ev.f32 ? eea::launch_history<float>(ev, rv, d_rec, s) : eea::launch_history<double>(ev, rv, d_rec, s));
  return EEA_OK;
}

eea_status eea_records_metric(eea_engine* e, unsigned n_rec, const void* d_rec, void* d_metric, void* d_ck, void* stream)
{
  if (e == nullptr || d_rec == nullptr || d_metric == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  if (n_rec == 0 || n_rec > 0x7fffffffu) return fail(EEA_ERR_INVALID_ARGUMENT, "n_rec must be in 1 .. 2^31 - 1");
  eea::EngineView ev;
  eea::engine_view(e, &ev);
  if (!ev.have_phik) return fail(EEA_ERR_NO_TARGET, "no phi_k: call eea_config_domain or eea_set_target_grid first");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const eea_status st = eea::engine_enter(e, s);
  if (st != EEA_OK) return st;
  EEA_HIP(ev.f32 ? eea::launch_metric<float>(ev, n_rec, d_rec, d_metric, d_ck, s)
                 : eea::launch_metric<double>(ev, n_rec, d_rec, d_metric, d_ck, s));
  return EEA_OK;
}

}  // extern "C"
