// GoalPaths: every robot's shortest (5-7 chamfer) way to its OWN goal cell through the traversable cells of a GridMap, on the
// device, each inside a bounded window around the robot and its goal (eea_geodesic_goto_batch).  No reference class.  For goals
// that no call of the same tick chose: last tick's, an operator's way-point, a rendezvous cell.  Constructed from Collision's
// parameters, in the manner of GeodesicField.  The object owns one device block: the poses, the goals and the outputs of its
// last go().
#pragma once

#include <stdexcept>
#include <vector>

#include <ergodic_exploration/collision.hpp>
#include <ergodic_exploration/device.hpp>
#include <ergodic_exploration/distance_field.hpp>
#include <ergodic_exploration/grid.hpp>

namespace ergodic_exploration
{
class GoalPaths
{
public:
  GoalPaths(double boundary_radius, double search_radius, double obstacle_threshold, double occupied_threshold)
    : collision_(boundary_radius, search_radius, obstacle_threshold, occupied_threshold)
  {
  }
  GoalPaths(const GoalPaths&) = delete;
  GoalPaths& operator=(const GoalPaths&) = delete;
  ~GoalPaths() { release(); }

  struct Paths
  {
    std::vector<int> cost;    // [P] the cost of the way to the goal, -1: none
    std::vector<int> status;  // [P] EEA_GOTO_OK / _NO_ROBOT / _NO_GOAL / _WINDOW / _CUT_OFF
    std::vector<int> len;     // [P] the moves written into path, -1: none
    mat path;                 // 3 x (P * n_steps): robot q's way-points in columns q * n_steps ..; its pose without a way
    unsigned ok = 0, window = 0, cut_off = 0, refused = 0;  // robots by status; refused: no robot cell or no goal
  };
  // the way of every robot of poses (3 x P) to its goal cell goals[q] (a row-major index of grid), inside the box of the two
  // cells grown by margin cells and clipped to the map; a robot whose window is past EEA_GOTO_MAX_CELLS or holds no way gets
  // status WINDOW / CUT_OFF, and the caller falls back to a GeodesicField.  distance, clear_sq, flags: as GeodesicField::update.
  // Waits
  Paths go(const GridMap& grid, const mat& poses, const std::vector<int>& goals, unsigned margin, unsigned n_steps,
           const DistanceField* distance = nullptr, int clear_sq = 0, unsigned flags = 0)
  {
    const unsigned P = static_cast<unsigned>(poses.n_cols());
    if (goals.size() != P) throw std::invalid_argument("GoalPaths: one goal per robot");
    const eea_collision_cfg cfg = collision_.deviceConfig(grid);
    Paths out;
    if (P == 0) return out;
    const size_t pose_bytes = sizeof(double) * 3 * P, path_bytes = sizeof(double) * 3 * P * n_steps;
    // one block: the poses, the path, the goals and the three int outputs, the counts
    const size_t need = pose_bytes + path_bytes + sizeof(int) * 4 * P + sizeof(unsigned) * 4;
    hip_check(hipSetDevice(device_ordinal()));
    if (need > capacity_) {
      release();
      hip_check(hipMalloc(&d_block_, need));
      capacity_ = need;
    }
    double* const d_pose = static_cast<double*>(d_block_);
    double* const d_path = d_pose + 3 * static_cast<size_t>(P);
    int* const d_goal = reinterpret_cast<int*>(reinterpret_cast<char*>(d_path) + path_bytes);
    int* const d_out = d_goal + P;
    unsigned* const d_state = reinterpret_cast<unsigned*>(d_out + 3 * static_cast<size_t>(P));
    hip_check(hipMemcpy(d_pose, poses.memptr(), pose_bytes, hipMemcpyHostToDevice));
    hip_check(hipMemcpy(d_goal, goals.data(), sizeof(int) * P, hipMemcpyHostToDevice));
    throw_on_error(eea_geodesic_goto_batch(device_ordinal(), &cfg, device_cells(grid), distance ? distance->squaredDistances() : nullptr,
                                           clear_sq, flags, d_pose, d_goal, nullptr, P, margin, n_steps, d_out, d_out + P,
                                           n_steps != 0 ? d_path : nullptr, d_out + 2 * static_cast<size_t>(P), d_state, nullptr));
    std::vector<int>* const outs[3] = { &out.cost, &out.status, &out.len };
    for (unsigned k = 0; k < 3; ++k) {
      outs[k]->resize(P);
      hip_check(hipMemcpy(outs[k]->data(), d_out + k * static_cast<size_t>(P), sizeof(int) * P, hipMemcpyDeviceToHost));
    }
    out.path = mat(3, static_cast<size_t>(P) * n_steps);
    if (path_bytes != 0) hip_check(hipMemcpy(out.path.memptr(), d_path, path_bytes, hipMemcpyDeviceToHost));
    unsigned state[4] = { 0, 0, 0, 0 };
    hip_check(hipMemcpy(state, d_state, sizeof(state), hipMemcpyDeviceToHost));
    out.ok = state[0];
    out.window = state[1];
    out.cut_off = state[2];
    out.refused = state[3];
    return out;
  }

private:
  void release()
  {
    if (d_block_) (void)hipFree(d_block_);
    d_block_ = nullptr;
    capacity_ = 0;
  }
  Collision collision_;
  void* d_block_ = nullptr;  // go(): its poses, goals and outputs
  size_t capacity_ = 0;
};
}  // namespace ergodic_exploration
