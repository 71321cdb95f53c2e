// DistanceField: the exact Euclidean distance transform of a GridMap's occupied cells on the device, and poses / a
// trajectory looked up in it (eea_distance_field / eea_distance_query_batch / eea_distance_traj_min).  No reference class:
// the reference README lists a distance field under "Future Improvements".  Beside Collision, whose ring search has gaps,
// sees nothing inside the bounding radius and nothing beyond the search radius; constructed from the same parameters.  The
// object owns the two device planes (squared cell distance, nearest occupied cell) of the map it was last updated with.
#pragma once

#include <cstring>
#include <stdexcept>
#include <vector>

#include <ergodic_exploration/collision.hpp>
#include <ergodic_exploration/device.hpp>
#include <ergodic_exploration/grid.hpp>

namespace ergodic_exploration
{
// state of a looked-up pose: Collision's three, and off the grid (which is not free space)
enum class DistanceMsg
{
  crash = EEA_COLLISION_CRASH,
  obstacle = EEA_COLLISION_OBSTACLE,
  none = EEA_COLLISION_NONE,
  off_grid = EEA_COLLISION_OFF_GRID
};

class DistanceField
{
public:
  DistanceField(double boundary_radius, double search_radius, double obstacle_threshold, double occupied_threshold)
    : collision_(boundary_radius, search_radius, obstacle_threshold, occupied_threshold)
  {
  }
  DistanceField(const DistanceField&) = delete;
  DistanceField& operator=(const DistanceField&) = delete;
  ~DistanceField() { release(); }

  // builds the field of this map (again after the map's cells changed: a GridMap's device copy is made once per object)
  void update(const GridMap& grid)
  {
    const eea_collision_cfg cfg = collision_.deviceConfig(grid);
    const size_t cells = static_cast<size_t>(cfg.xsize) * cfg.ysize;
    const int8_t* const d_grid = device_cells(grid);
    if (cells > capacity_) {
      release();
      hip_check(hipSetDevice(device_ordinal()));
      hip_check(hipMalloc(reinterpret_cast<void**>(&d_sq_), cells * sizeof(int)));
      hip_check(hipMalloc(reinterpret_cast<void**>(&d_nearest_), cells * sizeof(int)));
      capacity_ = cells;
    }
    built_ = false;
    throw_on_error(eea_distance_field(device_ordinal(), &cfg, d_grid, d_sq_, d_nearest_, nullptr));
    cfg_ = cfg;
    built_ = true;
  }

  // poses 3 x P through the field: msg [P], dmin [P], disp 2 x P, cells [P] = (sqrd_obs, dx, dy) per pose -- under a crash too
  struct Answer
  {
    std::vector<DistanceMsg> msg;
    std::vector<double> dmin;
    mat disp;
    std::vector<eea_clearance> cells;
  };
  Answer query(const mat& poses) const
  {
    need_field();
    Answer out;
    const unsigned P = static_cast<unsigned>(poses.n_cols());
    if (P == 0) return out;
    const size_t pose_bytes = sizeof(double) * 3 * P, dmin_bytes = sizeof(double) * P, disp_bytes = sizeof(double) * 2 * P;
    const PinnedScratch sc = pinned_scratch(pose_bytes + dmin_bytes + disp_bytes + sizeof(eea_clearance) * P);
    std::memcpy(sc.host, poses.memptr(), pose_bytes);
    char* const dev = static_cast<char*>(sc.dev);
    throw_on_error(eea_distance_query_batch(device_ordinal(), &cfg_, d_sq_, d_nearest_, reinterpret_cast<const double*>(dev), P,
                                            reinterpret_cast<eea_clearance*>(dev + pose_bytes + dmin_bytes + disp_bytes),
                                            reinterpret_cast<double*>(dev + pose_bytes),
                                            reinterpret_cast<double*>(dev + pose_bytes + dmin_bytes), nullptr));
    hip_check(hipStreamSynchronize(nullptr));
    const char* const host = static_cast<const char*>(sc.host);
    const double* const dmin = reinterpret_cast<const double*>(host + pose_bytes);
    const eea_clearance* const cells = reinterpret_cast<const eea_clearance*>(host + pose_bytes + dmin_bytes + disp_bytes);
    out.dmin.assign(dmin, dmin + P);
    out.cells.assign(cells, cells + P);
    out.disp = mat(2, P);
    std::memcpy(out.disp.memptr(), host + pose_bytes + dmin_bytes, disp_bytes);
    out.msg.reserve(P);
    for (unsigned q = 0; q < P; ++q) out.msg.push_back(static_cast<DistanceMsg>(cells[q].msg));
    return out;
  }

  // the worst step of a trajectory 3 x T (T >= 1): off the grid before on it, then the smallest distance, then the earliest
  struct WorstStep
  {
    DistanceMsg msg;
    eea_clearance cell;
    int step;
    double dmin;
  };
  WorstStep worstStep(const mat& traj) const
  {
    need_field();
    const unsigned T = static_cast<unsigned>(traj.n_cols());
    const size_t traj_bytes = sizeof(double) * 3 * T;
    const PinnedScratch sc = pinned_scratch(traj_bytes + sizeof(double) + sizeof(eea_clearance) + sizeof(int));
    std::memcpy(sc.host, traj.memptr(), traj_bytes);
    char* const dev = static_cast<char*>(sc.dev);
    throw_on_error(eea_distance_traj_min(device_ordinal(), &cfg_, d_sq_, d_nearest_, reinterpret_cast<const double*>(dev), 1, T,
                                         reinterpret_cast<eea_clearance*>(dev + traj_bytes + sizeof(double)),
                                         reinterpret_cast<int*>(dev + traj_bytes + sizeof(double) + sizeof(eea_clearance)),
                                         reinterpret_cast<double*>(dev + traj_bytes), nullptr));
    hip_check(hipStreamSynchronize(nullptr));
    const char* const host = static_cast<const char*>(sc.host);
    WorstStep w;
    std::memcpy(&w.dmin, host + traj_bytes, sizeof(double));
    std::memcpy(&w.cell, host + traj_bytes + sizeof(double), sizeof(eea_clearance));
    std::memcpy(&w.step, host + traj_bytes + sizeof(double) + sizeof(eea_clearance), sizeof(int));
    w.msg = static_cast<DistanceMsg>(w.cell.msg);
    return w;
  }

  // the planes of the last update, [ysize][xsize] row-major device memory
  const int* squaredDistances() const { return d_sq_; }
  const int* nearestCells() const { return d_nearest_; }

private:
  void need_field() const
  {
    if (!built_) throw std::logic_error("DistanceField: update() has not built a field");
  }
  void release()
  {
    if (d_sq_) (void)hipFree(d_sq_);
    if (d_nearest_) (void)hipFree(d_nearest_);
    d_sq_ = d_nearest_ = nullptr;
    capacity_ = 0;
    built_ = false;
  }
  Collision collision_;
  eea_collision_cfg cfg_{};
  int* d_sq_ = nullptr;
  int* d_nearest_ = nullptr;
  size_t capacity_ = 0;
  bool built_ = false;
};
}  // namespace ergodic_exploration
