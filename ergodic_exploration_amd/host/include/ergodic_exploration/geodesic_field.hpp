// GeodesicField: the shortest-path (5-7 chamfer) cost through the traversable cells of a GridMap from a set of source poses,
// on the device, and poses looked up in it: reachable or not, the cost, and the path down the field as way-points
// (eea_geodesic_field / eea_geodesic_path_batch).  No reference class: every distance of the reference is straight-line.
// Constructed from Collision's parameters, in the manner of DistanceField, whose plane inflates the obstacles by the robot's
// radius when one is given.  The object owns the device field, the workspace and the state words of its last update.
#pragma once

#include <cmath>
#include <cstring>
#include <stdexcept>
#include <vector>

#include <ergodic_exploration/collision.hpp>
#include <ergodic_exploration/device.hpp>
#include <ergodic_exploration/distance_field.hpp>
#include <ergodic_exploration/grid.hpp>

namespace ergodic_exploration
{
class GeodesicField
{
public:
  GeodesicField(double boundary_radius, double search_radius, double obstacle_threshold, double occupied_threshold)
    : collision_(boundary_radius, search_radius, obstacle_threshold, occupied_threshold)
  {
  }
  GeodesicField(const GeodesicField&) = delete;
  GeodesicField& operator=(const GeodesicField&) = delete;
  ~GeodesicField() { release(); }

  // builds the field of this map from the cells of the poses `sources` (3 x P); waits for it.  distance (optional): the
  // DistanceField updated with the same map -- cells within clear_sq (a squared cell radius) of an occupied one are not
  // traversable; flags: EEA_GEODESIC_UNKNOWN_BLOCKS
  void update(const GridMap& grid, const mat& sources, const DistanceField* distance = nullptr, int clear_sq = 0, unsigned flags = 0)
  {
    const eea_collision_cfg cfg = collision_.deviceConfig(grid);
    const size_t cells = static_cast<size_t>(cfg.xsize) * cfg.ysize;
    size_t ws_bytes = 0;
    throw_on_error(eea_geodesic_ws_bytes(&cfg, &ws_bytes));
    const int8_t* const d_grid = device_cells(grid);
    if (cells > capacity_ || ws_bytes > ws_capacity_) {
      release();
      hip_check(hipSetDevice(device_ordinal()));
      hip_check(hipMalloc(reinterpret_cast<void**>(&d_geo_), cells * sizeof(int)));
      hip_check(hipMalloc(&d_ws_, ws_bytes));
      hip_check(hipMalloc(reinterpret_cast<void**>(&d_state_), 4 * sizeof(unsigned)));
      capacity_ = cells;
      ws_capacity_ = ws_bytes;
    }
    built_ = false;
    const unsigned P = static_cast<unsigned>(sources.n_cols());
    const size_t pose_bytes = sizeof(double) * 3 * P;
    const PinnedScratch sc = pinned_scratch(pose_bytes ? pose_bytes : 1);
    if (P != 0) std::memcpy(sc.host, sources.memptr(), pose_bytes);
    throw_on_error(eea_geodesic_field(device_ordinal(), &cfg, d_grid, distance ? distance->squaredDistances() : nullptr, clear_sq,
                                      flags, static_cast<const double*>(sc.dev), P, nullptr, 0, 0, d_geo_, d_ws_, d_state_, nullptr));
    hip_check(hipMemcpy(state_, d_state_, sizeof(state_), hipMemcpyDeviceToHost));
    geo_.resize(cells);  // (the call above has waited: cost() looks poses up on the host)
    hip_check(hipMemcpy(geo_.data(), d_geo_, cells * sizeof(int), hipMemcpyDeviceToHost));
    cfg_ = cfg;
    built_ = true;
  }

  // of the last update: rounds that changed something, accepted sources
  unsigned rounds() const { return state_[1]; }
  unsigned sources() const { return state_[2]; }

  // cost [P] of the poses 3 x P: the field at the pose's cell, -1 when it is off the grid or cannot be reached
  std::vector<int> cost(const mat& poses) const
  {
    const Walk w = walk(poses, 1);
    std::vector<int> out(w.len.size());
    // a one-step walk on the device tells a pose on the field from one off it; the cost is the field's at the pose's cell
    for (size_t q = 0; q < out.size(); ++q) {
      out[q] = -1;
      if (w.len[q] < 0) continue;
      unsigned i = 0, j = 0;
      if (cell_of(poses(0, q), poses(1, q), i, j)) out[q] = geo_[static_cast<size_t>(i) * cfg_.xsize + j];
    }
    return out;
  }
  std::vector<bool> reachable(const mat& poses) const
  {
    const Walk w = walk(poses, 1);
    std::vector<bool> out(w.len.size());
    for (size_t q = 0; q < out.size(); ++q) out[q] = w.len[q] >= 0;
    return out;
  }

  // the path of every pose down the field: way-points 3 x (P * n_steps), pose q's in columns q * n_steps ..; len [P] = the
  // moves written, -1 for a pose off the grid or unreachable (its columns hold the pose)
  struct Walk
  {
    mat path;
    std::vector<int> len;
  };
  Walk path(const mat& poses, unsigned n_steps) const { return walk(poses, n_steps); }

  // the field of the last update, [ysize][xsize] row-major device memory
  const int* costs() const { return d_geo_; }

private:
  Walk walk(const mat& poses, unsigned n_steps) const
  {
    if (!built_) throw std::logic_error("GeodesicField: update() has not built a field");
    Walk out;
    const unsigned P = static_cast<unsigned>(poses.n_cols());
    if (P == 0) return out;
    const size_t pose_bytes = sizeof(double) * 3 * P, path_bytes = sizeof(double) * 3 * P * n_steps;
    const PinnedScratch sc = pinned_scratch(pose_bytes + path_bytes + sizeof(int) * P);
    std::memcpy(sc.host, poses.memptr(), pose_bytes);
    char* const dev = static_cast<char*>(sc.dev);
    throw_on_error(eea_geodesic_path_batch(device_ordinal(), &cfg_, d_geo_, reinterpret_cast<const double*>(dev), P, n_steps,
                                           reinterpret_cast<double*>(dev + pose_bytes),
                                           reinterpret_cast<int*>(dev + pose_bytes + path_bytes), nullptr));
    hip_check(hipStreamSynchronize(nullptr));
    const char* const host = static_cast<const char*>(sc.host);
    out.path = mat(3, static_cast<size_t>(P) * n_steps);
    std::memcpy(out.path.memptr(), host + pose_bytes, path_bytes);
    const int* const len = reinterpret_cast<const int*>(host + pose_bytes + path_bytes);
    out.len.assign(len, len + P);
    return out;
  }
  // GridMap::world2Grid + gridBounds of the map of the last update
  bool cell_of(double x, double y, unsigned& i, unsigned& j) const
  {
    j = static_cast<unsigned>(std::floor((x - cfg_.xmin) / cfg_.resolution));
    i = static_cast<unsigned>(std::floor((y - cfg_.ymin) / cfg_.resolution));
    if (j == cfg_.xsize) j--;
    if (i == cfg_.ysize) i--;
    return i <= cfg_.ysize - 1u && j <= cfg_.xsize - 1u;
  }
  void release()
  {
    if (d_geo_) (void)hipFree(d_geo_);
    if (d_ws_) (void)hipFree(d_ws_);
    if (d_state_) (void)hipFree(d_state_);
    d_geo_ = nullptr;
    d_ws_ = nullptr;
    d_state_ = nullptr;
    capacity_ = ws_capacity_ = 0;
    built_ = false;
  }
  Collision collision_;
  eea_collision_cfg cfg_{};
  int* d_geo_ = nullptr;
  void* d_ws_ = nullptr;
  unsigned* d_state_ = nullptr;
  unsigned state_[4] = { 0, 0, 0, 0 };
  std::vector<int> geo_;
  size_t capacity_ = 0, ws_capacity_ = 0;
  bool built_ = false;
};
}  // namespace ergodic_exploration
