// The replay memory of a FLEET in device memory (include/ergodic_amd.h, eea_replay_*): ReplayBuffer::append and
// ReplayBuffer::sampleMemory (reference buffer.cpp:54-62, 64-111) for B robots as kernels, filling the d_mem_cols / d_n_mem
// buffers eea_control_batch / eea_tick_batch take -- the closed loop of a fleet needs no host round trip between ticks.
//
// Store: robot-major [B][capacity][3] reals + count [B] + dropped [B].  A robot's draws then gather from ONE region of
// n x 24 bytes (neighbouring draws share cache lines, the region of a robot stays in the L2 of the XCD its wavefront runs
// on), eea_replay_read is one contiguous copy, and a wavefront that serves a robot owns everything of that robot -- store
// slot, count, output columns -- so the fused launch has no hand-off between wavefronts at all.  The price is an append of
// B scattered 24-byte stores instead of one contiguous write: 98 KB per tick at 4096 robots against the 9.8 MB of sampled
// columns the same launch writes.
//
// Random stream: counter-based, Philox4x32-10 (Salmon et al., SC'11; the three Random123 known answers are pinned in
// tests/test_replay_memory.py): counter (j, robot0 + b, draw_lo, draw_hi), key (seed_lo, seed_hi); r64 = out[0] | out[1] << 32;
// index = (r64 * n) >> 64.  A draw is a pure function of (seed, draw, global robot id, column): reproducible, and
// independent of how the fleet is sharded.
//
// The POOLED memory (eea_replay_pool_sample, at the end of the kernels below): the columns of a robot drawn from the stored
// poses of ALL robots of the object, optionally without its own -- two launches, an exclusive 64-bit prefix sum of count[B]
// and a sampler of the form of replay_sample_kernel that looks the owner of a pool index up in the offsets.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <limits>
#include <new>
#include <vector>

#include "abi_util.hpp"
#include "philox.hpp"  // philox4x32_10: shared with evidence_kernel.hip

struct eea_replay
{
  int device = 0;
  unsigned B = 0, capacity = 0, batch_size = 0, robot0 = 0;
  uint64_t seed = 0;
  size_t real_size = 8;
  void* d_store = nullptr;                  // [B][capacity][3] reals
  unsigned* d_count = nullptr;              // [B] stored poses
  unsigned long long* d_dropped = nullptr;  // [B] appends refused because the store was full
  unsigned long long* d_pool_off = nullptr;  // [B + 1] pool offsets, rewritten by every eea_replay_pool_sample on its stream
};

namespace eea
{
namespace
{
constexpr unsigned kWave = 64;
constexpr unsigned kRobotsPerBlock = 4;  // one wavefront per robot, 256 threads

template <typename real>
struct Pose
{
  real x, y, th;
};

struct ReplayParams
{
  unsigned B, capacity, batch_size, robot0, mem_stride;
  uint32_t seed_lo, seed_hi, draw_lo, draw_hi;
};

// ReplayBuffer::append for one robot, by the ONE lane that owns the robot in this launch: returns the count after the call
// (`n` is the count before it) and sets `fresh` to the slot it filled.
template <typename real>
__device__ __forceinline__ unsigned append_one(real* store_b, unsigned* count_b, unsigned long long* dropped_b, unsigned n,
                                               unsigned capacity, const Pose<real>& p, unsigned& fresh)
{
  if (n < capacity) {
    store_b[3 * static_cast<size_t>(n) + 0] = p.x;
    store_b[3 * static_cast<size_t>(n) + 1] = p.y;
    store_b[3 * static_cast<size_t>(n) + 2] = p.th;
    *count_b = n + 1;
    fresh = n;
    return n + 1;
  }
  *dropped_b += 1;  // "WARNING: Buffer is full" (buffer.cpp:61): the pose is dropped, this is not a ring
  return n;
}

template <typename real>
__device__ __forceinline__ Pose<real> load_pose(const real* a, size_t i)
{
  return Pose<real>{a[3 * i], a[3 * i + 1], a[3 * i + 2]};
}

constexpr unsigned kNoSlot = 0xffffffffu;

// eea_replay_append: one lane per robot
template <typename real>
__global__ void __launch_bounds__(256) replay_append_kernel(real* store, unsigned* count, unsigned long long* dropped,
                                                            const real* pose, const int* mask, unsigned B, unsigned capacity)
{
  const unsigned b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  if (mask != nullptr && mask[b] == 0) return;
  unsigned fresh = kNoSlot;
  append_one(store + 3 * static_cast<size_t>(b) * capacity, count + b, dropped + b, count[b], capacity, load_pose(pose, b), fresh);
}

// eea_replay_sample (APPEND = false) / eea_replay_append_sample (APPEND = true): one WAVEFRONT per robot, lanes along the
// column index, so that the 24-byte stores of a wavefront into [b][j][3] are one contiguous run.  The wavefront is the only
// one that touches robot b in this launch, and within it ONLY LANE 0 touches count[b], dropped[b] and the appended slot:
//  - lane 0 loads the count once, appends, and hands the count AFTER the append to the other lanes through a register
//    (__shfl): no lane reads count[b] while it is updated, because no other lane reads it at all;
//  - a column that resolves to the slot appended in this launch takes the pose from the registers that hold d_pose[b]
//    (every lane loads it: read-only in this launch), never from the store slot lane 0 is writing.
template <typename real, bool APPEND>
__global__ void __launch_bounds__(kWave* kRobotsPerBlock) replay_sample_kernel(real* store, unsigned* count, unsigned long long* dropped,
                                                                              const real* pose, const int* mask, real* mem_cols,
                                                                              int* n_mem, ReplayParams q)
{
  const unsigned lane = threadIdx.x % kWave;
  const unsigned b = blockIdx.x * kRobotsPerBlock + threadIdx.x / kWave;
  if (b >= q.B) return;  // (the same for all lanes of a wavefront: the __shfl below sees all 64)
  real* const store_b = store + 3 * static_cast<size_t>(b) * q.capacity;
  const bool appends = APPEND && (mask == nullptr || mask[b] != 0);
  Pose<real> p{};
  if (appends) p = load_pose(pose, b);
  unsigned n = 0, fresh = kNoSlot;  // fresh: the slot appended in this launch, if any
  if (lane == 0) {
    n = count[b];
    if (appends) n = append_one(store_b, count + b, dropped + b, n, q.capacity, p, fresh);
    n_mem[b] = static_cast<int>(n <= q.batch_size ? n : q.batch_size);
  }
  n = __shfl(n, 0);
  fresh = __shfl(fresh, 0);
  const bool all = n <= q.batch_size;  // buffer.cpp:75-89: the stored poses in order; :91-108: batch_size draws
  const unsigned cols = all ? n : q.batch_size;
  real* const out_b = mem_cols + 3 * static_cast<size_t>(b) * q.mem_stride;
  for (unsigned j = lane; j < cols; j += kWave) {
    unsigned idx = j;
    if (!all) {
      const Philox r = philox4x32_10(j, q.robot0 + b, q.draw_lo, q.draw_hi, q.seed_lo, q.seed_hi);
      const uint64_t r64 = static_cast<uint64_t>(r.v[0]) | (static_cast<uint64_t>(r.v[1]) << 32);
      idx = static_cast<unsigned>(__umul64hi(r64, static_cast<uint64_t>(n)));  // uniform on [0, n - 1], bias <= n / 2^64
    }
    const Pose<real> c = (APPEND && idx == fresh) ? p : load_pose(store_b, idx);
    out_b[3 * static_cast<size_t>(j) + 0] = c.x;
    out_b[3 * static_cast<size_t>(j) + 1] = c.y;
    out_b[3 * static_cast<size_t>(j) + 2] = c.th;
  }
}

// ---- the pooled memory: eea_replay_pool_sample ------------------------------------------------------------------------------
// The pool is every stored pose of every robot in robot-major order (the order of the store): robot q owns the pool indices
// [off[q], off[q + 1]), off = the exclusive prefix sum of count[], N = off[B].  Two launches ordered by the stream: the
// offsets, then the sampler.  A robot's columns come from OTHER robots' rows, which are complete only when the append launch
// in front has finished: the sampler is ordered behind it by the stream and never fused with it; no wavefront of either
// kernel waits for another workgroup.
constexpr unsigned kScanThreads = 1024;
constexpr unsigned kCoarseMax = 1024;  // entries of the coarse offset table in LDS (8 KB)

// off[0 .. B] = exclusive prefix sum of count[0 .. B), 64-bit.  ONE workgroup: chunks of 1024 counts (coalesced loads), per
// chunk a wavefront scan by shuffles, one LDS hop for the 16 wavefront totals, and the carry of the chunks in front in a
// register every thread keeps (all threads add the same total).  65 536 robots are 64 chunks.
__global__ void __launch_bounds__(kScanThreads) pool_offsets_kernel(const unsigned* count, unsigned long long* off, unsigned B)
{
  __shared__ unsigned long long wave_total[kScanThreads / kWave];
  const unsigned lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  unsigned long long carry = 0;
  for (unsigned first = 0; first < B; first += kScanThreads) {  // (uniform trip count: every thread meets every barrier)
    const unsigned i = first + threadIdx.x;
    const unsigned long long own = i < B ? count[i] : 0u;
    unsigned long long incl = own;
#pragma unroll
    for (unsigned d = 1; d < kWave; d *= 2) {
      const unsigned long long up = __shfl_up(incl, d);
      if (lane >= d) incl += up;
    }
    if (lane == kWave - 1) wave_total[wave] = incl;
    __syncthreads();
    unsigned long long before = 0, chunk = 0;
#pragma unroll
    for (unsigned w = 0; w < kScanThreads / kWave; ++w) {  // 16 LDS reads, the same address in every lane: broadcasts
      const unsigned long long t = wave_total[w];
      if (w < wave) before += t;
      chunk += t;
    }
    if (i < B) off[i] = carry + before + incl - own;
    carry += chunk;
    __syncthreads();  // wave_total is rewritten by the next chunk
  }
  if (threadIdx.x == 0) off[B] = carry;
}

struct PoolParams
{
  unsigned B, capacity, robot0, mem_stride, n_cols, stride, n_coarse;  // stride (a power of two) x n_coarse >= B
  int exclude_self, accumulate;
  uint32_t key_lo, key_hi, draw_lo, draw_hi;
};

// One WAVEFRONT per robot, lanes along the column index, as replay_sample_kernel.  off[] is read-only here (the launch in
// front wrote it), so every lane reads off[b], off[b + 1], off[B] itself; the one word this launch reads AND writes is
// n_mem[b] (accumulate), and ONLY LANE 0 touches it: it loads the base once, hands it to the other lanes in a register
// (__shfl) and stores the new value once.
// Owner of a pool index g < N: the last q with off[q] <= g (so off[q] <= g < off[q + 1]: a robot without poses, whose
// offset equals the next one, is never the last).  Two levels: every `stride`-th offset of off[0 .. B) staged in LDS by the
// workgroup (n_coarse <= 1024 entries; B <= 1024: the whole table), a binary search there, and the last log2(stride) steps
// in off[] itself, which a fleet's wavefronts keep hot in L2.
template <typename real>
__global__ void __launch_bounds__(kWave* kRobotsPerBlock) pool_sample_kernel(const real* store, const unsigned long long* off,
                                                                            real* mem_cols, int* n_mem, PoolParams q)
{
  __shared__ unsigned long long coarse[kCoarseMax];
  for (unsigned i = threadIdx.x; i < q.n_coarse; i += kWave * kRobotsPerBlock) coarse[i] = off[static_cast<size_t>(i) * q.stride];
  __syncthreads();
  const unsigned lane = threadIdx.x % kWave;
  const unsigned b = blockIdx.x * kRobotsPerBlock + threadIdx.x / kWave;
  if (b >= q.B) return;  // (behind the barrier; the same for all lanes of a wavefront: the __shfl below sees all 64)
  const unsigned long long off_b = off[b];
  const unsigned long long own = q.exclude_self ? off[b + 1] - off_b : 0ull;  // the robot's own poses, when they are left out
  const unsigned long long n_pool = off[q.B] - own;
  const bool all = n_pool <= q.n_cols;  // buffer.cpp:75-89: all poses in pool order; :91-108: n_cols draws
  unsigned cols = all ? static_cast<unsigned>(n_pool) : q.n_cols;
  unsigned base = 0;
  if (q.accumulate) {
    if (lane == 0) {
      const int have = n_mem[b];
      base = have > 0 ? static_cast<unsigned>(have) : 0u;
    }
    base = __shfl(base, 0);
    const unsigned room = base < q.mem_stride ? q.mem_stride - base : 0u;
    if (cols > room) cols = room;  // a clipped robot keeps the FIRST columns of its sequence: column j depends on j alone
  }
  if (lane == 0) n_mem[b] = static_cast<int>(base + cols);
  real* const out_b = mem_cols + 3 * (static_cast<size_t>(b) * q.mem_stride + base);
  for (unsigned j = lane; j < cols; j += kWave) {
    unsigned long long g = j;
    if (!all) {
      const Philox r = philox4x32_10(j, q.robot0 + b, q.draw_lo, q.draw_hi, q.key_lo, q.key_hi);
      const uint64_t r64 = static_cast<uint64_t>(r.v[0]) | (static_cast<uint64_t>(r.v[1]) << 32);
      g = __umul64hi(r64, n_pool);  // uniform on [0, n_pool - 1], bias <= n_pool / 2^64
    }
    if (g >= off_b) g += own;  // (own == 0 unless the robot's poses are left out: then its segment is skipped)
    unsigned lo = 0, hi = q.n_coarse;  // coarse[lo] <= g, (hi == n_coarse or coarse[hi] > g); coarse[0] == 0
    while (hi - lo > 1) {
      const unsigned mid = (lo + hi) / 2;
      if (coarse[mid] <= g) lo = mid; else hi = mid;
    }
    lo *= q.stride;
    hi = lo + q.stride < q.B ? lo + q.stride : q.B;  // off[lo] <= g < off[hi] (off[B] = N > g)
    while (hi - lo > 1) {
      const unsigned mid = (lo + hi) / 2;
      if (off[mid] <= g) lo = mid; else hi = mid;
    }
    const size_t slot = static_cast<size_t>(lo) * q.capacity + static_cast<size_t>(g - off[lo]);
    const Pose<real> c = load_pose(store, slot);
    out_b[3 * static_cast<size_t>(j) + 0] = c.x;
    out_b[3 * static_cast<size_t>(j) + 1] = c.y;
    out_b[3 * static_cast<size_t>(j) + 2] = c.th;
  }
}

template <typename real>
hipError_t launch_pool(const eea_replay* r, uint64_t draw, unsigned n_cols, int exclude_self, int accumulate, void* d_mem_cols,
                       int* d_n_mem, unsigned mem_stride, hipStream_t s)
{
  hipLaunchKernelGGL(pool_offsets_kernel, dim3(1), dim3(kScanThreads), 0, s, r->d_count, r->d_pool_off, r->B);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return err;
  unsigned stride = 1;
  while ((r->B + stride - 1) / stride > kCoarseMax) stride *= 2;  // B < 2^31: no overflow
  const PoolParams q{r->B,
                     r->capacity,
                     r->robot0,
                     mem_stride,
                     n_cols,
                     stride,
                     (r->B + stride - 1) / stride,
                     exclude_self != 0 ? 1 : 0,
                     accumulate != 0 ? 1 : 0,
                     static_cast<uint32_t>(r->seed),
                     static_cast<uint32_t>(r->seed >> 32) ^ 0x9E3779B9u,  // apart from the own-memory draws at the same (draw, robot, j)
                     static_cast<uint32_t>(draw),
                     static_cast<uint32_t>(draw >> 32)};
  hipLaunchKernelGGL(pool_sample_kernel<real>, dim3((r->B + kRobotsPerBlock - 1) / kRobotsPerBlock), dim3(kWave * kRobotsPerBlock),
                     0, s, static_cast<const real*>(r->d_store), r->d_pool_off, static_cast<real*>(d_mem_cols), d_n_mem, q);
  return hipGetLastError();
}

template <typename real>
hipError_t launch_append(const eea_replay* r, const void* d_pose, const int* d_mask, hipStream_t s)
{
  hipLaunchKernelGGL(replay_append_kernel<real>, dim3((r->B + 255) / 256), dim3(256), 0, s, static_cast<real*>(r->d_store),
                     r->d_count, r->d_dropped, static_cast<const real*>(d_pose), d_mask, r->B, r->capacity);
  return hipGetLastError();
}

template <typename real, bool APPEND>
hipError_t launch_sample(const eea_replay* r, const void* d_pose, const int* d_mask, uint64_t draw, void* d_mem_cols,
                         int* d_n_mem, unsigned mem_stride, hipStream_t s)
{
  const ReplayParams q{r->B,
                       r->capacity,
                       r->batch_size,
                       r->robot0,
                       mem_stride,
                       static_cast<uint32_t>(r->seed),
                       static_cast<uint32_t>(r->seed >> 32),
                       static_cast<uint32_t>(draw),
                       static_cast<uint32_t>(draw >> 32)};
  hipLaunchKernelGGL((replay_sample_kernel<real, APPEND>), dim3((r->B + kRobotsPerBlock - 1) / kRobotsPerBlock),
                     dim3(kWave * kRobotsPerBlock), 0, s, static_cast<real*>(r->d_store), r->d_count, r->d_dropped,
                     static_cast<const real*>(d_pose), d_mask, static_cast<real*>(d_mem_cols), d_n_mem, q);
  return hipGetLastError();
}

eea_status check_sample_args(const eea_replay* r, const void* d_mem_cols, const int* d_n_mem, unsigned mem_stride)
{
  if (r == nullptr || d_mem_cols == nullptr || d_n_mem == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  if (mem_stride < r->batch_size) {
    return fail(EEA_ERR_INVALID_ARGUMENT, "mem_stride must be at least the batch size of the replay memory");
  }
  return EEA_OK;
}
}  // namespace

void replay_view(const eea_replay* r, ReplayView* v)
{
  v->device = r->device;
  v->B = r->B;
  v->capacity = r->capacity;
  v->real_size = r->real_size;
  v->d_store = r->d_store;
  v->d_count = r->d_count;
}
}  // namespace eea

using eea::fail;

extern "C" {

eea_status eea_replay_create(int device, unsigned B, unsigned capacity, unsigned batch_size, uint64_t seed, unsigned robot0,
                             size_t real_size, eea_replay** out)
{
  if (out == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  *out = nullptr;
  if (B == 0 || capacity == 0 || batch_size == 0) {
    return fail(EEA_ERR_INVALID_ARGUMENT, "robots, capacity and batch size of a replay memory must be at least 1");
  }
  if (real_size != 8 && real_size != 4) return fail(EEA_ERR_INVALID_ARGUMENT, "real_size must be 8 (fp64) or 4 (fp32)");
  // [B][capacity][3] reals: the byte count must fit size_t (and the launch grid an int)
  const size_t max = std::numeric_limits<size_t>::max();
  const size_t per_robot = static_cast<size_t>(capacity) * 3 * real_size;  // < 2^32 * 24: fits 64 bits
  if (per_robot > max / B || B > 0x7fffffffu) return fail(EEA_ERR_HIP, "replay memory: robots x capacity overflows the store size");
  const size_t bytes = per_robot * B;
  eea_replay* r = new (std::nothrow) eea_replay();
  if (r == nullptr) return fail(EEA_ERR_HIP, "replay memory: out of host memory");
  r->device = device;
  r->B = B;
  r->capacity = capacity;
  r->batch_size = batch_size;
  r->seed = seed;
  r->robot0 = robot0;
  r->real_size = real_size;
  hipError_t err = hipSetDevice(device);
  if (err == hipSuccess) err = hipMalloc(&r->d_store, bytes);
  if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&r->d_count), sizeof(unsigned) * B);
  if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&r->d_dropped), sizeof(unsigned long long) * B);
  if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&r->d_pool_off), sizeof(unsigned long long) * (static_cast<size_t>(B) + 1));
  if (err == hipSuccess) err = hipMemset(r->d_count, 0, sizeof(unsigned) * B);
  if (err == hipSuccess) err = hipMemset(r->d_dropped, 0, sizeof(unsigned long long) * B);
  if (err != hipSuccess) {
    (void)hipGetLastError();  // (an allocation failure is sticky for the next hipGetLastError otherwise)
    const std::string msg = std::string("replay memory of ") + std::to_string(bytes) + " bytes: " + hipGetErrorString(err);
    eea_replay_destroy(r);
    return fail(EEA_ERR_HIP, msg);
  }
  *out = r;
  return EEA_OK;
}

void eea_replay_destroy(eea_replay* r)
{
  if (r == nullptr) return;
  if (r->d_store != nullptr || r->d_count != nullptr || r->d_dropped != nullptr || r->d_pool_off != nullptr) {
    if (hipSetDevice(r->device) == hipSuccess) {
      if (r->d_store != nullptr) (void)hipFree(r->d_store);  // waits for its users
      if (r->d_count != nullptr) (void)hipFree(r->d_count);
      if (r->d_dropped != nullptr) (void)hipFree(r->d_dropped);
      if (r->d_pool_off != nullptr) (void)hipFree(r->d_pool_off);
    }
  }
  delete r;
}

eea_status eea_replay_append(eea_replay* r, const void* d_pose, const int* d_mask, void* stream)
{
  if (r == nullptr || d_pose == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  EEA_HIP(hipSetDevice(r->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  EEA_HIP(r->real_size == 8 ? eea::launch_append<double>(r, d_pose, d_mask, s) : eea::launch_append<float>(r, d_pose, d_mask, s));
  return EEA_OK;
}

eea_status eea_replay_sample(eea_replay* r, uint64_t draw, void* d_mem_cols, int* d_n_mem, unsigned mem_stride, void* stream)
{
  const eea_status st = eea::check_sample_args(r, d_mem_cols, d_n_mem, mem_stride);
  if (st != EEA_OK) return st;
  EEA_HIP(hipSetDevice(r->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  EEA_HIP(r->real_size == 8 ? (eea::launch_sample<double, false>(r, nullptr, nullptr, draw, d_mem_cols, d_n_mem, mem_stride, s))
                            : (eea::launch_sample<float, false>(r, nullptr, nullptr, draw, d_mem_cols, d_n_mem, mem_stride, s)));
  return EEA_OK;
}

eea_status eea_replay_append_sample(eea_replay* r, const void* d_pose, const int* d_mask, uint64_t draw, void* d_mem_cols,
                                    int* d_n_mem, unsigned mem_stride, void* stream)
{
  const eea_status st = eea::check_sample_args(r, d_mem_cols, d_n_mem, mem_stride);
  if (st != EEA_OK) return st;
  if (d_pose == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  EEA_HIP(hipSetDevice(r->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  EEA_HIP(r->real_size == 8 ? (eea::launch_sample<double, true>(r, d_pose, d_mask, draw, d_mem_cols, d_n_mem, mem_stride, s))
                            : (eea::launch_sample<float, true>(r, d_pose, d_mask, draw, d_mem_cols, d_n_mem, mem_stride, s)));
  return EEA_OK;
}

eea_status eea_replay_pool_sample(eea_replay* r, uint64_t draw, unsigned n_cols, int exclude_self, int accumulate,
                                  void* d_mem_cols, int* d_n_mem, unsigned mem_stride, void* stream)
{
  if (r == nullptr || d_mem_cols == nullptr || d_n_mem == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  if (n_cols == 0) return fail(EEA_ERR_INVALID_ARGUMENT, "pooled sample: n_cols must be at least 1");
  if (mem_stride == 0) return fail(EEA_ERR_INVALID_ARGUMENT, "pooled sample: mem_stride must be at least 1");
  if (accumulate == 0 && mem_stride < n_cols) {
    return fail(EEA_ERR_INVALID_ARGUMENT, "pooled sample: mem_stride must be at least n_cols unless the columns are accumulated");
  }
  EEA_HIP(hipSetDevice(r->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  EEA_HIP(r->real_size == 8
            ? eea::launch_pool<double>(r, draw, n_cols, exclude_self, accumulate, d_mem_cols, d_n_mem, mem_stride, s)
            : eea::launch_pool<float>(r, draw, n_cols, exclude_self, accumulate, d_mem_cols, d_n_mem, mem_stride, s));
  return EEA_OK;
}

eea_status eea_replay_counts(eea_replay* r, unsigned* h_count, unsigned long long* h_dropped)
{
  if (r == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  EEA_HIP(hipSetDevice(r->device));
  EEA_HIP(hipDeviceSynchronize());
  if (h_count != nullptr) EEA_HIP(hipMemcpy(h_count, r->d_count, sizeof(unsigned) * r->B, hipMemcpyDeviceToHost));
  if (h_dropped != nullptr) {
    std::vector<unsigned long long> d(r->B);
    EEA_HIP(hipMemcpy(d.data(), r->d_dropped, sizeof(unsigned long long) * r->B, hipMemcpyDeviceToHost));
    unsigned long long sum = 0;
    for (unsigned long long v : d) sum += v;
    *h_dropped = sum;
  }
  return EEA_OK;
}

eea_status eea_replay_read(eea_replay* r, unsigned b, unsigned first, unsigned n, void* h_cols)
{
  if (r == nullptr || (n > 0 && h_cols == nullptr)) return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  if (b >= r->B) return fail(EEA_ERR_INVALID_ARGUMENT, "replay memory: no such robot");
  EEA_HIP(hipSetDevice(r->device));
  EEA_HIP(hipDeviceSynchronize());
  unsigned count = 0;
  EEA_HIP(hipMemcpy(&count, r->d_count + b, sizeof(unsigned), hipMemcpyDeviceToHost));
  if (first > count || n > count - first) return fail(EEA_ERR_INVALID_ARGUMENT, "replay memory: poses past the robot's count");
  if (n == 0) return EEA_OK;
  const char* src = static_cast<const char*>(r->d_store) + (static_cast<size_t>(b) * r->capacity + first) * 3 * r->real_size;
  EEA_HIP(hipMemcpy(h_cols, src, static_cast<size_t>(n) * 3 * r->real_size, hipMemcpyDeviceToHost));
  return EEA_OK;
}

eea_status eea_replay_reset(eea_replay* r, void* stream)
{
  if (r == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  EEA_HIP(hipSetDevice(r->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  EEA_HIP(hipMemsetAsync(r->d_count, 0, sizeof(unsigned) * r->B, s));
  EEA_HIP(hipMemsetAsync(r->d_dropped, 0, sizeof(unsigned long long) * r->B, s));
  return EEA_OK;
}

}  // extern "C"
