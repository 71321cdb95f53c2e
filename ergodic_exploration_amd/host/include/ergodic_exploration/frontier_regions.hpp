// FrontierRegions: the frontier cells of a GridMap -- free cells with an unknown axis neighbour -- grouped into their
// 8-connected regions, each with a label, a rank, a size, a centroid, a bounding box and, given a GeodesicPartition of the same
// map, the member that is cheapest to reach with the robot that owns it; and per robot the region it should go for
// (eea_frontier_regions / eea_frontier_goals).  No reference class.  Constructed from Collision's parameters, like
// GeodesicPartition.  The object owns the two device planes, the records, the workspace, the state words and the goals of its
// last goals() call.  auction() gives every robot -- of any fleet, not only the partition's -- a region by distance and capacity
// (eea_frontier_auction) and owns one more block: its workspace, poses and outputs.
#pragma once

#include <stdexcept>
#include <vector>

#include <ergodic_exploration/collision.hpp>
#include <ergodic_exploration/device.hpp>
#include <ergodic_exploration/geodesic_partition.hpp>
#include <ergodic_exploration/grid.hpp>

namespace ergodic_exploration
{
class FrontierRegions
{
public:
  // max_regions: the records kept (regions are ranked by their least cell index; those past max_regions keep their rank in
  // regionAt and have no record)
  FrontierRegions(double boundary_radius, double search_radius, double obstacle_threshold, double occupied_threshold,
                  unsigned max_regions = 4096)
    : collision_(boundary_radius, search_radius, obstacle_threshold, occupied_threshold), max_regions_(max_regions)
  {
  }
  FrontierRegions(const FrontierRegions&) = delete;
  FrontierRegions& operator=(const FrontierRegions&) = delete;
  ~FrontierRegions() { release(); }

  // labels the frontier of this map; with a partition (built from the same map, it must outlive the goals() calls that
  // follow) only reachable cells are members and every record gets its entry.  Waits
  void update(const GridMap& grid, const GeodesicPartition* partition = nullptr)
  {
    const eea_collision_cfg cfg = collision_.deviceConfig(grid);
    const size_t cells = static_cast<size_t>(cfg.xsize) * cfg.ysize;
    size_t ws_bytes = 0;
    throw_on_error(eea_frontier_ws_bytes(&cfg, &ws_bytes));
    const int8_t* const d_grid = device_cells(grid);
    built_ = false;
    hip_check(hipSetDevice(device_ordinal()));
    if (cells > capacity_ || ws_bytes > ws_capacity_) {
      release_planes();
      hip_check(hipMalloc(reinterpret_cast<void**>(&d_root_), cells * sizeof(int)));
      hip_check(hipMalloc(reinterpret_cast<void**>(&d_region_), cells * sizeof(int)));
      hip_check(hipMalloc(&d_ws_, ws_bytes));  // (an allocation's start: 8-byte aligned)
      hip_check(hipMalloc(reinterpret_cast<void**>(&d_state_), 4 * sizeof(unsigned)));
      if (max_regions_ != 0) hip_check(hipMalloc(reinterpret_cast<void**>(&d_regions_), sizeof(eea_frontier_region) * max_regions_));
      capacity_ = cells;
      ws_capacity_ = ws_bytes;
    }
    throw_on_error(eea_frontier_regions(device_ordinal(), &cfg, EEA_FRONTIER_OF_GRID, d_grid, partition ? partition->costs() : nullptr,
                                        partition ? partition->owners() : nullptr, max_regions_, d_root_, d_region_, d_regions_, d_ws_,
                                        d_state_, nullptr));
    hip_check(hipMemcpy(state_, d_state_, sizeof(state_), hipMemcpyDeviceToHost));
    records_.resize(state_[1]);
    if (state_[1] != 0) {
      hip_check(hipMemcpy(records_.data(), d_regions_, sizeof(eea_frontier_region) * state_[1], hipMemcpyDeviceToHost));
    }
    xsize_ = cfg.xsize;
    cells_ = cells;
    robots_ = partition ? partition->robots() : 0;
    built_ = true;
  }

  // of the last update: the regions found, the member cells, and the records of the first min(count, max_regions) regions
  unsigned count() const { return state_[0]; }
  unsigned members() const { return state_[2]; }
  const std::vector<eea_frontier_region>& regions() const { return records_; }

  // the planes of the last update, [ysize][xsize] row-major device memory: the least cell index of the cell's region and the
  // region's rank, -1 for a cell that is no member
  const int* roots() const { return d_root_; }
  const int* ranks() const { return d_region_; }
  // one cell of them (row i, column j); each call copies one int from the device
  int rootAt(unsigned i, unsigned j) const { return cell_of(d_root_, i, j); }
  int regionAt(unsigned i, unsigned j) const { return cell_of(d_region_, i, j); }

  struct Goals
  {
    std::vector<int> cell;      // [P] row-major index of the robot's goal (its region's entry cell), -1: none
    std::vector<int> region;    // [P] the rank of the region it goes for, -1: none
    std::vector<double> score;  // [P] its score, 0.0 without a goal
  };
  // per robot of the partition of the last update the region whose entry it owns, of at least min_size cells, with the
  // greatest w_size * size - w_cost * entry cost, the lowest rank on a tie.  Waits
  Goals goals(unsigned min_size, double w_size, double w_cost)
  {
    if (!built_) throw std::logic_error("FrontierRegions: update() has not labelled a map");
    Goals out;
    const unsigned P = robots_;
    if (P == 0) return out;
    if (max_regions_ == 0) throw std::logic_error("FrontierRegions: goals() needs records (max_regions > 0)");
    if (P > robots_capacity_) {
      release_robots();
      hip_check(hipSetDevice(device_ordinal()));
      hip_check(hipMalloc(reinterpret_cast<void**>(&d_goal_score_), sizeof(double) * P));
      hip_check(hipMalloc(reinterpret_cast<void**>(&d_goal_cell_), sizeof(int) * P));
      hip_check(hipMalloc(reinterpret_cast<void**>(&d_goal_region_), sizeof(int) * P));
      robots_capacity_ = P;
    }
    throw_on_error(eea_frontier_goals(device_ordinal(), d_regions_, d_state_, max_regions_, P, min_size, w_size, w_cost, d_goal_cell_,
                                      d_goal_region_, d_goal_score_, nullptr));
    out.cell.resize(P);
    out.region.resize(P);
    out.score.resize(P);
    hip_check(hipMemcpy(out.cell.data(), d_goal_cell_, sizeof(int) * P, hipMemcpyDeviceToHost));
    hip_check(hipMemcpy(out.region.data(), d_goal_region_, sizeof(int) * P, hipMemcpyDeviceToHost));
    hip_check(hipMemcpy(out.score.data(), d_goal_score_, sizeof(double) * P, hipMemcpyDeviceToHost));
    return out;
  }
  // the goal cells of the last goals() call on the device, [robots]: what eea_partition_path_batch takes as d_goal_cell
  const int* goalCells() const { return d_goal_cell_; }

  struct Assignment
  {
    std::vector<int> region;  // [P] the rank of the region the robot goes for, -1: none
    std::vector<int> cell;    // [P] row-major index of its goal, the member of that region its walk ends on, -1: none
    std::vector<int> cost;    // [P] the cost of the way there, -1: none
    std::vector<int> len;     // [P] the moves written into path, -1: none
    mat path;                 // 3 x (P * n_steps): robot q's way-points in columns q * n_steps ..; its pose without a goal
    bool final = false;       // every field of the call was built to the end
    unsigned assigned = 0, rounds = 0;  // robots with a goal; auction rounds that were not idle
  };
  // a region of the last update for every robot of poses (3 x P; any robots, not only a partition's), by distance and capacity
  // (eea_frontier_auction): n_auction rounds in which every robot without a region bids for the nearest region with room left
  // and a region takes the nearest bidders -- 1, or ceil(size / cells_per_robot) of them over the whole call.  grid is the map
  // of the last update; distance, clear_sq, flags: as GeodesicField::update.  Waits
  Assignment auction(const GridMap& grid, const mat& poses, unsigned n_auction, unsigned min_size, unsigned cells_per_robot,
                     unsigned n_steps, unsigned flags = 0, const DistanceField* distance = nullptr, int clear_sq = 0)
  {
    if (!built_) throw std::logic_error("FrontierRegions: update() has not labelled a map");
    const eea_collision_cfg cfg = collision_.deviceConfig(grid);
    if (static_cast<size_t>(cfg.xsize) * cfg.ysize != cells_ || cfg.xsize != xsize_) {
      throw std::logic_error("FrontierRegions: auction() needs the map of the last update");
    }
    Assignment out;
    const unsigned P = static_cast<unsigned>(poses.n_cols());
    if (P == 0) return out;
    size_t ws_bytes = 0;
    throw_on_error(eea_frontier_auction_ws_bytes(&cfg, P, max_regions_, &ws_bytes));
    const size_t path_bytes = sizeof(double) * 3 * P * n_steps;
    // one block: the workspace (an allocation's start: 8-byte aligned), the poses, the path, the four int outputs, the state
    const size_t ws_room = (ws_bytes + 7) / 8 * 8;
    const size_t need = ws_room + sizeof(double) * 3 * P + path_bytes + sizeof(int) * 4 * P + sizeof(unsigned) * 4;
    hip_check(hipSetDevice(device_ordinal()));
    if (need > auction_capacity_) {
      release_auction();
      hip_check(hipMalloc(&d_auction_, need));
      auction_capacity_ = need;
    }
    char* const base = static_cast<char*>(d_auction_);
    double* const d_pose = reinterpret_cast<double*>(base + ws_room);
    double* const d_path = d_pose + 3 * static_cast<size_t>(P);
    int* const d_out = reinterpret_cast<int*>(reinterpret_cast<char*>(d_path) + path_bytes);
    unsigned* const d_state = reinterpret_cast<unsigned*>(d_out + 4 * static_cast<size_t>(P));
    hip_check(hipMemcpy(d_pose, poses.memptr(), sizeof(double) * 3 * P, hipMemcpyHostToDevice));
    throw_on_error(eea_frontier_auction(device_ordinal(), &cfg, device_cells(grid), distance ? distance->squaredDistances() : nullptr,
                                        clear_sq, flags, d_region_, d_regions_, d_state_, max_regions_, d_pose, P, n_auction, min_size,
                                        cells_per_robot, 0, n_steps, d_out, d_out + P, d_out + 2 * static_cast<size_t>(P),
                                        n_steps != 0 ? d_path : nullptr, d_out + 3 * static_cast<size_t>(P), d_auction_, d_state, nullptr));
    std::vector<int>* const outs[4] = { &out.region, &out.cell, &out.cost, &out.len };
    for (unsigned k = 0; k < 4; ++k) {
      outs[k]->resize(P);
      hip_check(hipMemcpy(outs[k]->data(), d_out + k * static_cast<size_t>(P), sizeof(int) * P, hipMemcpyDeviceToHost));
    }
    out.path = mat(3, static_cast<size_t>(P) * n_steps);
    if (path_bytes != 0) hip_check(hipMemcpy(out.path.memptr(), d_path, path_bytes, hipMemcpyDeviceToHost));
    unsigned state[4] = { 0, 0, 0, 0 };
    hip_check(hipMemcpy(state, d_state, sizeof(state), hipMemcpyDeviceToHost));
    out.final = state[0] != 0;
    out.assigned = state[2];
    out.rounds = state[3];
    return out;
  }

private:
  int cell_of(const int* plane, unsigned i, unsigned j) const
  {
    if (!built_) throw std::logic_error("FrontierRegions: update() has not labelled a map");
    const size_t at = static_cast<size_t>(i) * xsize_ + j;
    if (j >= xsize_ || at >= cells_) throw std::out_of_range("FrontierRegions: cell outside the grid");
    int v = -1;
    hip_check(hipMemcpy(&v, plane + at, sizeof(int), hipMemcpyDeviceToHost));
    return v;
  }
  void release_planes()
  {
    if (d_root_) (void)hipFree(d_root_);
    if (d_region_) (void)hipFree(d_region_);
    if (d_ws_) (void)hipFree(d_ws_);
    if (d_state_) (void)hipFree(d_state_);
    if (d_regions_) (void)hipFree(d_regions_);
    d_root_ = d_region_ = nullptr;
    d_ws_ = nullptr;
    d_state_ = nullptr;
    d_regions_ = nullptr;
    capacity_ = ws_capacity_ = 0;
  }
  void release_robots()
  {
    if (d_goal_score_) (void)hipFree(d_goal_score_);
    if (d_goal_cell_) (void)hipFree(d_goal_cell_);
    if (d_goal_region_) (void)hipFree(d_goal_region_);
    d_goal_score_ = nullptr;
    d_goal_cell_ = d_goal_region_ = nullptr;
    robots_capacity_ = 0;
  }
  void release_auction()
  {
    if (d_auction_) (void)hipFree(d_auction_);
    d_auction_ = nullptr;
    auction_capacity_ = 0;
  }
  void release()
  {
    release_planes();
    release_robots();
    release_auction();
    built_ = false;
  }
  Collision collision_;
  unsigned max_regions_;
  int *d_root_ = nullptr, *d_region_ = nullptr, *d_goal_cell_ = nullptr, *d_goal_region_ = nullptr;
  eea_frontier_region* d_regions_ = nullptr;
  void* d_ws_ = nullptr;
  void* d_auction_ = nullptr;  // auction(): its workspace, poses and outputs
  size_t auction_capacity_ = 0;
  unsigned* d_state_ = nullptr;
  double* d_goal_score_ = nullptr;
  unsigned state_[4] = { 0, 0, 0, 0 };
  std::vector<eea_frontier_region> records_;
  unsigned xsize_ = 0, robots_ = 0;
  size_t cells_ = 0, capacity_ = 0, ws_capacity_ = 0, robots_capacity_ = 0;
  bool built_ = false;
};
}  // namespace ergodic_exploration
