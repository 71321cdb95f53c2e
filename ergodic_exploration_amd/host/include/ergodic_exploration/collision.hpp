// Collision: Bresenham ring search around the robot cell (reference collision.hpp /
// collision.cpp).  The search itself runs in the batched device kernels
// (eea_collision_check_batch / eea_validate_control_batch / eea_clearance_batch); this class owns the parameters.  The
// device copy of a map's cells lives with the GridMap (device_cells), call arguments in a per-thread
// scratch buffer: a call costs two small copies and one launch, no allocation.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstring>
#include <memory>
#include <stdexcept>
#include <tuple>
#include <vector>

#include <ergodic_exploration/device.hpp>
#include <ergodic_exploration/grid.hpp>

namespace ergodic_exploration
{
// state of the search (reference collision.hpp:55-60); the values of EEA_COLLISION_*
enum class CollisionMsg
{
  crash = EEA_COLLISION_CRASH,
  obstacle = EEA_COLLISION_OBSTACLE,
  none = EEA_COLLISION_NONE
};

class Collision
{
public:
  Collision(double boundary_radius, double search_radius, double obstacle_threshold, double occupied_threshold)
    : boundary_radius_(boundary_radius)
    , search_radius_(search_radius)
    , obstacle_threshold_(obstacle_threshold)
    , occupied_threshold_(occupied_threshold)
  {
    if (search_radius_ < boundary_radius_) {
      throw std::invalid_argument("Search radius must be at least the same size as the boundary radius");
    }
    if (occupied_threshold_ > 100.0 || occupied_threshold_ < 0.0) {
      throw std::invalid_argument("Occupied threshold must be between 0 and 100");
    }
  }

  // true if the pose is in collision
  bool collisionCheck(const GridMap& grid, const vec& pose) const
  {
    mat p(3, 1);
    p.set_col(0, pose);
    return collisionCheck(grid, p).at(0);
  }

  // batched form: poses 3 x P
  std::vector<bool> collisionCheck(const GridMap& grid, const mat& poses) const
  {
    const unsigned P = static_cast<unsigned>(poses.n_cols());
    if (P == 0) return {};
    const int8_t* const d_grid = device_cells(grid);
    const size_t pose_bytes = sizeof(double) * 3 * P;
    const PinnedScratch sc = pinned_scratch(pose_bytes + sizeof(int) * P);
    std::memcpy(sc.host, poses.memptr(), pose_bytes);
    const eea_collision_cfg cfg = config(grid);
    throw_on_error(eea_collision_check_batch(device_ordinal(), &cfg, d_grid, static_cast<const double*>(sc.dev), P,
                                             reinterpret_cast<int*>(static_cast<char*>(sc.dev) + pose_bytes), nullptr));
    hip_check(hipStreamSynchronize(nullptr));
    const int* const hit = reinterpret_cast<const int*>(static_cast<const char*>(sc.host) + pose_bytes);
    return std::vector<bool>(hit, hit + P);
  }

  // collision state and distance to the closest obstacle cell the ring search sees (reference collision.cpp:65-93):
  // crash: 0.0, none: the largest double
  std::tuple<CollisionMsg, double> minDistance(const GridMap& grid, const vec& pose) const
  {
    mat p(3, 1);
    p.set_col(0, pose);
    const Clearance c = clearance(grid, p);
    return std::make_tuple(c.msg.at(0), c.dmin.at(0));
  }

  // ... and the displacement from the robot's cell to that cell (reference collision.cpp:95-124): crash: zeros, none: the
  // largest double twice
  std::tuple<CollisionMsg, vec> minDirection(const GridMap& grid, const vec& pose) const
  {
    mat p(3, 1);
    p.set_col(0, pose);
    const Clearance c = clearance(grid, p);
    return std::make_tuple(c.msg.at(0), c.disp.col(0));
  }

  // batched form of both: poses 3 x P; msg [P], dmin [P], disp 2 x P, cells [P] = the search's (sqrd_obs, dx, dy) per pose
  struct Clearance
  {
    std::vector<CollisionMsg> msg;
    std::vector<double> dmin;
    mat disp;
    std::vector<eea_clearance> cells;
  };
  Clearance clearance(const GridMap& grid, const mat& poses) const
  {
    Clearance out;
    const unsigned P = static_cast<unsigned>(poses.n_cols());
    if (P == 0) return out;
    const int8_t* const d_grid = device_cells(grid);
    const size_t pose_bytes = sizeof(double) * 3 * P, dmin_bytes = sizeof(double) * P, disp_bytes = sizeof(double) * 2 * P;
    const PinnedScratch sc = pinned_scratch(pose_bytes + dmin_bytes + disp_bytes + sizeof(eea_clearance) * P);
    std::memcpy(sc.host, poses.memptr(), pose_bytes);
    const eea_collision_cfg cfg = config(grid);
    char* const dev = static_cast<char*>(sc.dev);
    throw_on_error(eea_clearance_batch(device_ordinal(), &cfg, d_grid, reinterpret_cast<const double*>(dev), P,
                                       reinterpret_cast<eea_clearance*>(dev + pose_bytes + dmin_bytes + disp_bytes),
                                       reinterpret_cast<double*>(dev + pose_bytes), reinterpret_cast<double*>(dev + pose_bytes + dmin_bytes),
                                       nullptr));
    hip_check(hipStreamSynchronize(nullptr));
    const char* const host = static_cast<const char*>(sc.host);
    const double* const dmin = reinterpret_cast<const double*>(host + pose_bytes);
    const eea_clearance* const cells = reinterpret_cast<const eea_clearance*>(host + pose_bytes + dmin_bytes + disp_bytes);
    out.dmin.assign(dmin, dmin + P);
    out.cells.assign(cells, cells + P);
    out.disp = mat(2, P);
    std::memcpy(out.disp.memptr(), host + pose_bytes + dmin_bytes, disp_bytes);
    out.msg.reserve(P);
    for (unsigned q = 0; q < P; ++q) out.msg.push_back(static_cast<CollisionMsg>(cells[q].msg));
    return out;
  }

  // validate_control (reference numerics.hpp:312-330) for P (state, twist) pairs: true = collision free
  std::vector<bool> validateControl(const GridMap& grid, const mat& x0, const mat& u, double dt, double horizon) const
  {
    const unsigned P = static_cast<unsigned>(x0.n_cols());
    if (P == 0) return {};
    const int8_t* const d_grid = device_cells(grid);
    const size_t pose_bytes = sizeof(double) * 3 * P;
    const PinnedScratch sc = pinned_scratch(2 * pose_bytes + sizeof(int) * P);
    std::memcpy(sc.host, x0.memptr(), pose_bytes);
    std::memcpy(static_cast<char*>(sc.host) + pose_bytes, u.memptr(), pose_bytes);
    const eea_collision_cfg cfg = config(grid);
    char* const dev = static_cast<char*>(sc.dev);
    throw_on_error(eea_validate_control_batch(device_ordinal(), &cfg, d_grid, reinterpret_cast<const double*>(dev),
                                              reinterpret_cast<const double*>(dev + pose_bytes), dt, horizon, P,
                                              reinterpret_cast<int*>(dev + 2 * pose_bytes), nullptr));
    hip_check(hipStreamSynchronize(nullptr));
    const int* const ok = reinterpret_cast<const int*>(static_cast<const char*>(sc.host) + 2 * pose_bytes);
    return std::vector<bool>(ok, ok + P);
  }

  double totalPadding() const { return boundary_radius_ + obstacle_threshold_; }
  // geometry + thresholds in the C-ABI layout
  eea_collision_cfg deviceConfig(const GridMap& grid) const { return config(grid); }

private:
  eea_collision_cfg config(const GridMap& grid) const
  {
    eea_collision_cfg c;
    c.xmin = grid.xmin();
    c.ymin = grid.ymin();
    c.resolution = grid.resolution();
    c.xsize = grid.xsize();
    c.ysize = grid.ysize();
    c.boundary_radius = boundary_radius_;
    c.search_radius = search_radius_;
    c.obstacle_threshold = obstacle_threshold_;
    c.occupied_threshold = occupied_threshold_;
    return c;
  }
  double boundary_radius_, search_radius_, obstacle_threshold_, occupied_threshold_;
};

// numerics.hpp:312-330 of the reference for a single (state, twist)
inline bool validate_control(const Collision& collision, const GridMap& grid, const vec& x0, const vec& u, double dt,
                             double horizon)
{
  mat X(3, 1), U(3, 1);
  X.set_col(0, x0);
  U.set_col(0, u);
  return collision.validateControl(grid, X, U, dt, horizon).at(0);
}
}  // namespace ergodic_exploration
