// FleetReplayMemory: the replay memory of a fleet of robots in DEVICE memory (eea_replay_* of include/ergodic_amd.h) -- one
// ReplayBuffer (buffer.hpp; reference buffer.cpp) per robot, append and sampleMemory as kernels that fill the d_mem_cols /
// d_n_mem buffers eea_control_batch / eea_tick_batch take.  With it the loop of a fleet,
//     appendSample(d_pose, tick, d_mem_cols, d_n_mem, stream); eea_tick_batch(..); eea_integrate_twist_batch(..);
// stays on one stream without a host round trip between ticks.  ReplayBuffer itself serves the single-robot path, where the
// host holds the poses anyway.  The random stream is counter-based (Philox4x32-10 over (seed, tick, global robot id,
// column): ergodic_amd.h), so a shard of a fleet passes the global id of its first robot and draws what the whole fleet
// would have drawn for its robots.
#pragma once

#include <cstdint>
#include <vector>

#include <ergodic_exploration/device.hpp>

namespace ergodic_exploration
{
class FleetReplayMemory
{
public:
  // buffer_size / batch_size: the constructor arguments of ReplayBuffer, per robot; real_size: 8 (fp64 engines) or 4
  FleetReplayMemory(unsigned int n_robots, unsigned int buffer_size, unsigned int batch_size, std::uint64_t seed = 5489u,
                    unsigned int first_robot = 0, std::size_t real_size = sizeof(double))
    : n_(n_robots), batch_size_(batch_size), real_size_(real_size)
  {
    throw_on_error(eea_replay_create(device_ordinal(), n_robots, buffer_size, batch_size, seed, first_robot, real_size, &r_));
  }
  ~FleetReplayMemory() { eea_replay_destroy(r_); }
  FleetReplayMemory(const FleetReplayMemory&) = delete;
  FleetReplayMemory& operator=(const FleetReplayMemory&) = delete;

  // ReplayBuffer::append of d_pose [n][3] for the robots with d_mask[b] != 0 (nullptr: all); a full store drops and counts
  void append(const void* d_pose, const int* d_mask = nullptr, void* stream = nullptr)
  {
    throw_on_error(eea_replay_append(r_, d_pose, d_mask, stream));
  }
  // the columns sampleMemory() prepends: d_mem_cols [n][mem_stride][3], d_n_mem [n]; tick: the caller's tick counter
  void sample(std::uint64_t tick, void* d_mem_cols, int* d_n_mem, unsigned int mem_stride, void* stream = nullptr)
  {
    throw_on_error(eea_replay_sample(r_, tick, d_mem_cols, d_n_mem, mem_stride, stream));
  }
  // append, then sample from the memory that includes the new pose (exploration.hpp:209 then :232), in one launch
  void appendSample(const void* d_pose, std::uint64_t tick, void* d_mem_cols, int* d_n_mem, unsigned int mem_stride,
                    const int* d_mask = nullptr, void* stream = nullptr)
  {
    throw_on_error(eea_replay_append_sample(r_, d_pose, d_mask, tick, d_mem_cols, d_n_mem, mem_stride, stream));
  }
  // up to n_cols columns per robot from the POOLED history of all robots of this object (exclude_self: without the robot's
  // own poses); accumulate: behind the d_n_mem[b] columns the row already holds -- appendSample(..), then
  // samplePool(.., accumulate = true, ..) on the same buffers and stream puts the fleet's past behind the robot's own
  void samplePool(std::uint64_t tick, unsigned int n_cols, void* d_mem_cols, int* d_n_mem, unsigned int mem_stride,
                  bool exclude_self = false, bool accumulate = false, void* stream = nullptr)
  {
    throw_on_error(eea_replay_pool_sample(r_, tick, n_cols, exclude_self ? 1 : 0, accumulate ? 1 : 0, d_mem_cols, d_n_mem,
                                          mem_stride, stream));
  }
  // poses stored per robot (ReplayBuffer::size); waits for the device
  std::vector<unsigned int> sizes() const
  {
    std::vector<unsigned int> n(n_);
    throw_on_error(eea_replay_counts(r_, n.data(), nullptr));
    return n;
  }
  // appends refused by full stores ("WARNING: Buffer is full"), all robots; waits for the device
  unsigned long long dropped() const
  {
    unsigned long long d = 0;
    throw_on_error(eea_replay_counts(r_, nullptr, &d));
    return d;
  }
  // poses first .. first + n - 1 of one robot, n x 3 reals of realSize() bytes into h_cols; waits for the device
  void read(unsigned int robot, unsigned int first, unsigned int n, void* h_cols) const
  {
    throw_on_error(eea_replay_read(r_, robot, first, n, h_cols));
  }
  void reset(void* stream = nullptr) { throw_on_error(eea_replay_reset(r_, stream)); }
  // d_rec [n][eea_ck_record_len(e)]: the sum record of every robot's WHOLE stored history in the engine's current domain
  // (Basis::trajCoeff without the 1/N; element K^2 = the robot's count); eea_ck_records_sum over the rows is the fleet's
  void historyRecords(eea_engine* e, void* d_rec, void* stream = nullptr)
  {
    throw_on_error(eea_replay_history_records(e, r_, d_rec, stream));
  }

  unsigned int robots() const { return n_; }
  unsigned int batchSize() const { return batch_size_; }  // the least mem_stride sample() takes
  std::size_t realSize() const { return real_size_; }
  eea_replay* handle() const { return r_; }

private:
  unsigned int n_, batch_size_;
  std::size_t real_size_;
  eea_replay* r_ = nullptr;
};

// the ergodic metric sum_k lamda_k (c_k - phi_k)^2 of n_rec sum records (history records, a fleet record, the consensus
// records of control passes): d_metric [n_rec], d_ck [n_rec][K^2] optional
inline void recordsMetric(eea_engine* e, unsigned int n_rec, const void* d_rec, void* d_metric, void* d_ck = nullptr,
                          void* stream = nullptr)
{
  throw_on_error(eea_records_metric(e, n_rec, d_rec, d_metric, d_ck, stream));
}

// the same records as maps on the target grid: d_field [n_rec][nrows][nx] = the band-limited visit density, the deficit
// against the target or the potential control() descends (kind: EEA_FIELD_*), rows row0 .. row0 + nrows - 1 of an
// nx x ny_total grid in the Fourier frame (eea_records_field)
inline void recordsField(eea_engine* e, int kind, unsigned int n_rec, const void* d_rec, unsigned int nx,
                         unsigned int ny_total, unsigned int row0, unsigned int nrows, void* d_field, void* stream = nullptr)
{
  throw_on_error(eea_records_field(e, kind, n_rec, d_rec, nx, ny_total, row0, nrows, d_field, stream));
}
}  // namespace ergodic_exploration
