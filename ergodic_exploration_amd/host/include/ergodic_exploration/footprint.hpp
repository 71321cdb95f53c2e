// Footprint: the robot's base as a convex polygon, checked against a GridMap's occupied cells on the device
// (eea_footprint_radii / eea_footprint_check_batch / eea_footprint_traj_first / eea_footprint_validate_control_batch; the
// dynamic window for such a base: DynamicWindow::control's overloads that take a Footprint).  No reference class: the reference README lists
// a polygon base under "Future Improvements".  Beside Collision, which treats the robot as a disc and reads no heading.  A pose
// collides iff an occupied in-grid cell has its centre in the closed polygon placed at the pose; a DistanceField of the same
// map and the same occupied threshold, when given, decides most poses with one lookup and never changes an answer.
#pragma once

#include <cstring>
#include <stdexcept>
#include <utility>
#include <vector>

#include <ergodic_exploration/device.hpp>
#include <ergodic_exploration/distance_field.hpp>
#include <ergodic_exploration/grid.hpp>

namespace ergodic_exploration
{
class Footprint
{
public:
  // vertices (x, y) in the body frame, metres, counter-clockwise and strictly convex, the body origin strictly inside: else
  // std::invalid_argument.  No padding: a margin is a larger polygon.  occupied_threshold: Collision's, in [0, 100]
  explicit Footprint(const std::vector<std::pair<double, double>>& vertices, double occupied_threshold = 0.8)
    : occupied_threshold_(occupied_threshold)
  {
    if (occupied_threshold_ > 100.0 || occupied_threshold_ < 0.0) {
      throw std::invalid_argument("Occupied threshold must be between 0 and 100");
    }
    fp_ = eea_footprint{};
    fp_.n = static_cast<unsigned>(vertices.size());
    for (size_t k = 0; k < vertices.size() && k < EEA_FOOTPRINT_MAX_VERTICES; ++k) {
      fp_.x[k] = vertices[k].first;
      fp_.y[k] = vertices[k].second;
    }
    throw_on_error(eea_footprint_radii(&fp_, &r_in_, &r_out_));
  }

  // radii of the inscribed and the circumscribed circle about the body origin
  double inscribedRadius() const { return r_in_; }
  double circumscribedRadius() const { return r_out_; }

  // true if the base at the pose covers the centre of an occupied cell
  bool check(const GridMap& grid, const vec& pose, const DistanceField* field = nullptr) const
  {
    mat p(3, 1);
    p.set_col(0, pose);
    return check(grid, p, field).at(0);
  }

  // batched form: poses 3 x P
  std::vector<bool> check(const GridMap& grid, const mat& poses, const DistanceField* field = nullptr) const
  {
    const unsigned P = static_cast<unsigned>(poses.n_cols());
    if (P == 0) return {};
    const int8_t* const d_grid = device_cells(grid);
    const size_t pose_bytes = sizeof(double) * 3 * P;
    const PinnedScratch sc = pinned_scratch(pose_bytes + sizeof(int) * P);
    std::memcpy(sc.host, poses.memptr(), pose_bytes);
    const eea_collision_cfg cfg = deviceConfig(grid);
    throw_on_error(eea_footprint_check_batch(device_ordinal(), &cfg, &fp_, d_grid, field ? field->squaredDistances() : nullptr,
                                             static_cast<const double*>(sc.dev), P,
                                             reinterpret_cast<int*>(static_cast<char*>(sc.dev) + pose_bytes), nullptr));
    hip_check(hipStreamSynchronize(nullptr));
    const int* const hit = reinterpret_cast<const int*>(static_cast<const char*>(sc.host) + pose_bytes);
    return std::vector<bool>(hit, hit + P);
  }

  // the first colliding step of a trajectory 3 x T (T >= 1), -1 when none collides
  int firstStep(const GridMap& grid, const mat& traj, const DistanceField* field = nullptr) const
  {
    const unsigned T = static_cast<unsigned>(traj.n_cols());
    const int8_t* const d_grid = device_cells(grid);
    const size_t traj_bytes = sizeof(double) * 3 * T;
    const PinnedScratch sc = pinned_scratch(traj_bytes + sizeof(int));
    std::memcpy(sc.host, traj.memptr(), traj_bytes);
    const eea_collision_cfg cfg = deviceConfig(grid);
    throw_on_error(eea_footprint_traj_first(device_ordinal(), &cfg, &fp_, d_grid, field ? field->squaredDistances() : nullptr,
                                            static_cast<const double*>(sc.dev), 1, T,
                                            reinterpret_cast<int*>(static_cast<char*>(sc.dev) + traj_bytes), nullptr));
    hip_check(hipStreamSynchronize(nullptr));
    int step;
    std::memcpy(&step, static_cast<const char*>(sc.host) + traj_bytes, sizeof(int));
    return step;
  }

  // validate_control (numerics.hpp:312-330) for this base: true when no step of the rollout of the twist u from x0 collides
  bool validateControl(const GridMap& grid, const vec& x0, const vec& u, double dt, double horizon,
                       const DistanceField* field = nullptr) const
  {
    const int8_t* const d_grid = device_cells(grid);
    const PinnedScratch sc = pinned_scratch(sizeof(double) * 7);  // x0 | u | valid
    double* const h = static_cast<double*>(sc.host);
    double* const d_buf = static_cast<double*>(sc.dev);
    for (int c = 0; c < 3; ++c) {
      h[c] = x0(c);
      h[3 + c] = u(c);
    }
    const eea_collision_cfg cfg = deviceConfig(grid);
    throw_on_error(eea_footprint_validate_control_batch(device_ordinal(), &cfg, &fp_, d_grid, field ? field->squaredDistances() : nullptr,
                                                        d_buf, d_buf + 3, dt, horizon, 1, reinterpret_cast<int*>(d_buf + 6), nullptr));
    hip_check(hipStreamSynchronize(nullptr));
    int valid = 0;
    std::memcpy(&valid, &h[6], sizeof(int));
    return valid != 0;
  }

  const eea_footprint& deviceFootprint() const { return fp_; }

  // the geometry and the occupied threshold; the calls read no radius
  eea_collision_cfg deviceConfig(const GridMap& grid) const
  {
    eea_collision_cfg c{};
    c.xmin = grid.xmin();
    c.ymin = grid.ymin();
    c.resolution = grid.resolution();
    c.xsize = grid.xsize();
    c.ysize = grid.ysize();
    c.occupied_threshold = occupied_threshold_;
    return c;
  }

private:
  eea_footprint fp_;
  double occupied_threshold_;
  double r_in_ = 0.0, r_out_ = 0.0;
};
}  // namespace ergodic_exploration
