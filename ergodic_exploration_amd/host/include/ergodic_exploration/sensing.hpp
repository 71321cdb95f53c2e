// The range sensor of a simulated fleet (eea_sense_reveal_batch / eea_grid_census of include/ergodic_amd.h): every robot
// casts 8 * range_cells rays through a ground-truth occupancy grid in DEVICE memory and the cells the rays cross become known.
// With it the loop of a fleet that explores a map it has not seen,
//     senseReveal(cfg, R, d_truth, d_known, d_pose, n, ..); gridCensus(cfg, d_known, d_counts, ..);
//     appendSample(..); eea_tick_batch(.. d_grid = d_known ..); eea_integrate_twist_batch(..);
// stays on one stream.  The known grid becomes the target in one of three ways:
//   the entropy surrogate -- eea_set_target_occupancy (entropy(), numerics.hpp:164-179: every unknown cell 0.7, every known one
//     1e-3; it waits for its stream);
//   the gain count -- setTargetGain(engine, cfg, R, stride, d_known, floor, lx, ly, ..): the unknown cells a scan from each cell
//     would cross (senseGainField), zero where nothing is left to see, no host wait;
//   the mutual information -- setTargetMi(engine, cfg, R, stride, p_unknown, d_known, floor, lx, ly, ..): the information that
//     scan is EXPECTED to yield (senseMiField), which reads the occupancy probabilities 1 .. 99 and discounts a cell by the
//     chance that a beam gets as far; zero once the map is known, no host wait.
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

// d_gain [ysize][xsize] (every element overwritten) = for every candidate cell -- both indices multiples of stride, the cell
// itself not blocking -- the unknown cells the sensor's 8 * range_cells rays would cross from there through d_known, counted
// per beam, + 1 for an unknown own cell; 0 elsewhere.  Integers; asynchronous
inline void senseGainField(const eea_collision_cfg& cfg, unsigned int range_cells, unsigned int stride, const std::int8_t* d_known,
                           unsigned int* d_gain, void* stream = nullptr)
{
  throw_on_error(eea_sense_gain_field(device_ordinal(), &cfg, range_cells, stride, d_known, d_gain, stream));
}

// that field + floor on the candidates -> the engine's phi_k on the domain (lx, ly), all on `stream` and without a host wait
// on a repeated call; d_gain (optional) receives the integer field.  floor > 0 keeps the target finite (uniform over the free
// candidates) once nothing is left to see
inline void setTargetGain(eea_engine* engine, const eea_collision_cfg& cfg, unsigned int range_cells, unsigned int stride,
                          const std::int8_t* d_known, double floor, double lx, double ly, unsigned int* d_gain = nullptr,
                          void* stream = nullptr)
{
  throw_on_error(eea_set_target_gain(engine, &cfg, range_cells, stride, d_known, floor, lx, ly, d_gain, stream));
}

// h256 / pass256 [256], entry v + 128: the entropy h(v) and the pass probability pass(v) of the int8 cell value v at cfg's
// occupied_threshold, an unknown cell being occupied with probability p_unknown -- the doubles the two calls below use.  Host only
inline void senseMiTable(const eea_collision_cfg& cfg, double p_unknown, double* h256, double* pass256)
{
  throw_on_error(eea_sense_mi_table(&cfg, p_unknown, h256, pass256));
}

// d_mi [ysize][xsize] (every element overwritten) = for every candidate cell -- both indices multiples of stride, the cell
// itself not blocking -- the Shannon mutual information between the map and the sensor's 8 * range_cells ideal beams cast from
// there through d_known: h(own) + sum over rays and steps of (prod of pass before the step) * h(step); +0.0 elsewhere.  fp64, a
// fixed order: the same bits on every call; asynchronous
inline void senseMiField(const eea_collision_cfg& cfg, unsigned int range_cells, unsigned int stride, double p_unknown,
                         const std::int8_t* d_known, double* d_mi, void* stream = nullptr)
{
  throw_on_error(eea_sense_mi_field(device_ordinal(), &cfg, range_cells, stride, p_unknown, d_known, d_mi, stream));
}

// that field + floor on the candidates -> the engine's phi_k on the domain (lx, ly), all on `stream` and without a host wait
// on a repeated call; d_mi (optional) receives the field.  floor > 0 keeps the target finite once the map is known
inline void setTargetMi(eea_engine* engine, const eea_collision_cfg& cfg, unsigned int range_cells, unsigned int stride,
                        double p_unknown, const std::int8_t* d_known, double floor, double lx, double ly, double* d_mi = nullptr,
                        void* stream = nullptr)
{
  throw_on_error(eea_set_target_mi(engine, &cfg, range_cells, stride, p_unknown, d_known, floor, lx, ly, d_mi, stream));
}
}  // namespace ergodic_exploration
