// The range sensor of a simulated fleet (eea_sense_reveal_batch / eea_grid_census of include/ergodic_amd.h): every robot
// casts 8 * range_cells rays through a ground-truth occupancy grid in DEVICE memory and the cells the rays cross become known.
// With it the loop of a fleet that explores a map it has not seen,
//     senseReveal(cfg, R, d_truth, d_known, d_pose, n, ..); gridCensus(cfg, d_known, d_counts, ..);
//     appendSample(..); eea_tick_batch(.. d_grid = d_known ..); eea_integrate_twist_batch(..);
// stays on one stream; the known grid becomes the target through eea_set_target_occupancy (entropy(), numerics.hpp:164-179).
// This is the simulated counterpart of a 360 degree range finder (reference README.md:74-76), not OccupancyMapper (mapping.hpp).
#pragma once

#include <cstdint>

#include <ergodic_exploration/device.hpp>

namespace ergodic_exploration
{
// rays per robot: 8 * range_cells (the row length of d_ranges)
inline unsigned int senseRayCount(unsigned int range_cells) { return eea_sense_ray_count(range_cells); }

// d_known [ysize][xsize] is updated in place from d_truth along the rays of the n_robots poses d_pose [n][3]; d_ranges
// [n][8 * range_cells] (optional): the step at which a ray met a blocking cell, or -1; d_mask [n] (optional): robots with 0
// are left out.  cfg: the grid's geometry and occupied_threshold (the radii are not read)
inline void senseReveal(const eea_collision_cfg& cfg, unsigned int range_cells, const std::int8_t* d_truth, std::int8_t* d_known,
                        const double* d_pose, unsigned int n_robots, int* d_ranges = nullptr, const int* d_mask = nullptr,
                        void* stream = nullptr)
{
  throw_on_error(eea_sense_reveal_batch(device_ordinal(), &cfg, range_cells, d_truth, d_known, d_pose, d_mask, n_robots,
                                        d_ranges, stream));
}

// d_counts [3] = unknown cells (< 0), known cells below the occupied threshold, blocking cells of d_grid: the progress of
// an exploring fleet without reading the grid back
inline void gridCensus(const eea_collision_cfg& cfg, const std::int8_t* d_grid, unsigned long long* d_counts,
                       void* stream = nullptr)
{
  throw_on_error(eea_grid_census(device_ordinal(), &cfg, d_grid, d_counts, stream));
}
}  // namespace ergodic_exploration
