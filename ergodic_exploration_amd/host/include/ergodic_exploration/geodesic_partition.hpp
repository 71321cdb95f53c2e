// GeodesicPartition: the geodesic field of a GridMap from the fleet's poses with, per cell, the robot that reaches it most
// cheaply (the geodesic Voronoi partition of free space); per robot the area of its region, its goal -- the best cell of its
// own region under a score of a gain or mutual-information field minus the cost of getting there -- and the path from the
// robot to that goal (eea_geodesic_partition / eea_partition_goals / eea_partition_path_batch).  No reference class.
// Constructed from Collision's parameters, built like GeodesicField.  The object owns the two device planes, the workspace, the
// state words, the poses of its last update and the goals of its last goals() call.
#pragma once

#include <cstring>
#include <stdexcept>
#include <vector>

#include <ergodic_exploration/collision.hpp>
#include <ergodic_exploration/device.hpp>
#include <ergodic_exploration/distance_field.hpp>
#include <ergodic_exploration/grid.hpp>

namespace ergodic_exploration
{
class GeodesicPartition
{
public:
  GeodesicPartition(double boundary_radius, double search_radius, double obstacle_threshold, double occupied_threshold)
    : collision_(boundary_radius, search_radius, obstacle_threshold, occupied_threshold)
  {
  }
  GeodesicPartition(const GeodesicPartition&) = delete;
  GeodesicPartition& operator=(const GeodesicPartition&) = delete;
  ~GeodesicPartition() { release(); }

  // builds both planes of this map from the cells of the robots' poses (3 x P; robot q has label q); waits for it.  distance,
  // clear_sq, flags: as GeodesicField::update.  The map must outlive the goals() calls that follow: they read its device cells
  void update(const GridMap& grid, const mat& poses, const DistanceField* distance = nullptr, int clear_sq = 0, unsigned flags = 0)
  {
    const eea_collision_cfg cfg = collision_.deviceConfig(grid);
    const size_t cells = static_cast<size_t>(cfg.xsize) * cfg.ysize;
    const unsigned P = static_cast<unsigned>(poses.n_cols());
    size_t ws_bytes = 0;
    throw_on_error(eea_partition_ws_bytes(&cfg, &ws_bytes));
    const int8_t* const d_grid = device_cells(grid);
    built_ = have_goals_ = false;
    hip_check(hipSetDevice(device_ordinal()));
    if (cells > capacity_ || ws_bytes > ws_capacity_) {
      release_planes();
      hip_check(hipMalloc(reinterpret_cast<void**>(&d_geo_), cells * sizeof(int)));
      hip_check(hipMalloc(reinterpret_cast<void**>(&d_owner_), cells * sizeof(int)));
      hip_check(hipMalloc(&d_ws_, ws_bytes));  // (an allocation's start: 8-byte aligned)
      hip_check(hipMalloc(reinterpret_cast<void**>(&d_state_), 4 * sizeof(unsigned)));
      capacity_ = cells;
      ws_capacity_ = ws_bytes;
    }
    if (P > robots_capacity_) {
      release_robots();
      hip_check(hipMalloc(reinterpret_cast<void**>(&d_pose_), sizeof(double) * 3 * P));
      hip_check(hipMalloc(reinterpret_cast<void**>(&d_goal_score_), sizeof(double) * P));
      hip_check(hipMalloc(reinterpret_cast<void**>(&d_goal_cell_), sizeof(int) * P));
      hip_check(hipMalloc(reinterpret_cast<void**>(&d_area_), sizeof(unsigned) * P));
      robots_capacity_ = P;
    }
    if (P != 0) hip_check(hipMemcpy(d_pose_, poses.memptr(), sizeof(double) * 3 * P, hipMemcpyHostToDevice));
    throw_on_error(eea_geodesic_partition(device_ordinal(), &cfg, d_grid, distance ? distance->squaredDistances() : nullptr, clear_sq,
                                          flags, d_pose_, P, nullptr, 0, 0, d_geo_, d_owner_, d_ws_, d_state_, nullptr));
    hip_check(hipMemcpy(state_, d_state_, sizeof(state_), hipMemcpyDeviceToHost));
    cfg_ = cfg;
    d_grid_ = d_grid;
    P_ = P;
    built_ = true;
  }

  // of the last update: rounds that changed something, accepted sources, robots
  unsigned rounds() const { return state_[1]; }
  unsigned sources() const { return state_[2]; }
  unsigned robots() const { return P_; }

  // the planes of the last update, [ysize][xsize] row-major device memory: the robot that owns the cell (-1: nobody reaches
  // it) and the cost from that robot (GeodesicField's for the same sources)
  const int* owners() const { return d_owner_; }
  const int* costs() const { return d_geo_; }

  struct Goals
  {
    std::vector<int> cell;       // [P] row-major index of the robot's goal, -1: no candidate in its region
    std::vector<double> score;   // [P] its score, 0.0 without a goal
    std::vector<unsigned> area;  // [P] cells the robot owns
  };
  // per robot the candidate of its own region with the greatest w_field * field - w_cost * cost, the lowest index on a tie.
  // kind 0: d_field is the uint32 device field of sense_gain_field, 1: the double field of sense_mi_field, for the map of the
  // last update; candidates lie on the stride lattice, on cells of that map that do not block, with field > 0.  Waits
  Goals goals(int kind, const void* d_field, unsigned stride, double w_field, double w_cost)
  {
    need_field();
    Goals out;
    have_goals_ = false;
    if (P_ == 0) return out;
    throw_on_error(eea_partition_goals(device_ordinal(), &cfg_, kind, d_field, stride, d_grid_, d_geo_, d_owner_, P_, w_field, w_cost,
                                       d_goal_cell_, d_goal_score_, d_area_, nullptr));
    out.cell.resize(P_);
    out.score.resize(P_);
    out.area.resize(P_);
    hip_check(hipMemcpy(out.cell.data(), d_goal_cell_, sizeof(int) * P_, hipMemcpyDeviceToHost));
    hip_check(hipMemcpy(out.score.data(), d_goal_score_, sizeof(double) * P_, hipMemcpyDeviceToHost));
    hip_check(hipMemcpy(out.area.data(), d_area_, sizeof(unsigned) * P_, hipMemcpyDeviceToHost));
    have_goals_ = true;
    return out;
  }

  // area [P] alone: the cells each robot owns.  A goals call with both weights 0 whose field is the cost plane itself (any
  // plane of the grid's size serves: an area does not depend on it); the goals of the last goals() call are forgotten
  std::vector<unsigned> area()
  {
    std::vector<unsigned> out = goals(0, d_geo_, 1, 0.0, 0.0).area;
    have_goals_ = false;
    return out;
  }

  // every robot's way from its own cell to its goal of the last goals() call, inside its own region: way-points 3 x (P *
  // n_steps), robot q's in columns q * n_steps ..; len [P] = the moves written, -1 for a robot without a goal or off the grid
  // (its columns hold its pose)
  struct Walk
  {
    mat path;
    std::vector<int> len;
  };
  Walk paths(unsigned n_steps) const
  {
    need_field();
    if (!have_goals_) throw std::logic_error("GeodesicPartition: goals() has not chosen goals");
    Walk out;
    const size_t path_bytes = sizeof(double) * 3 * P_ * n_steps;
    const PinnedScratch sc = pinned_scratch(path_bytes + sizeof(int) * P_);
    char* const dev = static_cast<char*>(sc.dev);
    throw_on_error(eea_partition_path_batch(device_ordinal(), &cfg_, d_geo_, d_owner_, d_pose_, P_, d_goal_cell_, n_steps,
                                            reinterpret_cast<double*>(dev), reinterpret_cast<int*>(dev + path_bytes), nullptr));
    hip_check(hipStreamSynchronize(nullptr));
    const char* const host = static_cast<const char*>(sc.host);
    out.path = mat(3, static_cast<size_t>(P_) * n_steps);
    std::memcpy(out.path.memptr(), host, path_bytes);
    const int* const len = reinterpret_cast<const int*>(host + path_bytes);
    out.len.assign(len, len + P_);
    return out;
  }

private:
  void need_field() const
  {
    if (!built_) throw std::logic_error("GeodesicPartition: update() has not built a partition");
  }
  void release_planes()
  {
    if (d_geo_) (void)hipFree(d_geo_);
    if (d_owner_) (void)hipFree(d_owner_);
    if (d_ws_) (void)hipFree(d_ws_);
    if (d_state_) (void)hipFree(d_state_);
    d_geo_ = d_owner_ = nullptr;
    d_ws_ = nullptr;
    d_state_ = nullptr;
    capacity_ = ws_capacity_ = 0;
  }
  void release_robots()
  {
    if (d_pose_) (void)hipFree(d_pose_);
    if (d_goal_score_) (void)hipFree(d_goal_score_);
    if (d_goal_cell_) (void)hipFree(d_goal_cell_);
    if (d_area_) (void)hipFree(d_area_);
    d_pose_ = d_goal_score_ = nullptr;
    d_goal_cell_ = nullptr;
    d_area_ = nullptr;
    robots_capacity_ = 0;
  }
  void release()
  {
    release_planes();
    release_robots();
    built_ = have_goals_ = false;
  }
  Collision collision_;
  eea_collision_cfg cfg_{};
  const int8_t* d_grid_ = nullptr;
  int *d_geo_ = nullptr, *d_owner_ = nullptr, *d_goal_cell_ = nullptr;
  void* d_ws_ = nullptr;
  unsigned *d_state_ = nullptr, *d_area_ = nullptr;
  double *d_pose_ = nullptr, *d_goal_score_ = nullptr;
  unsigned state_[4] = { 0, 0, 0, 0 };
  unsigned P_ = 0;
  size_t capacity_ = 0, ws_capacity_ = 0, robots_capacity_ = 0;
  bool built_ = false, have_goals_ = false;
};
}  // namespace ergodic_exploration
