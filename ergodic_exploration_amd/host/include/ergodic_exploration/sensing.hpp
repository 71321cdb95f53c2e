// The range sensor of a simulated fleet (eea_sense_reveal_batch / eea_grid_census of include/ergodic_amd.h): every robot
// casts 8 * range_cells rays through a ground-truth occupancy grid in DEVICE memory and the cells the rays cross become known.
// With it the loop of a fleet that explores a map it has not seen,
//     senseReveal(cfg, R, d_truth, d_known, d_pose, n, ..); gridCensus(cfg, d_known, d_counts, ..);
//     appendSample(..); eea_tick_batch(.. d_grid = d_known ..); eea_integrate_twist_batch(..);
// stays on one stream.  With a NOISY sensor the first step is two: every scan is fused into an evidence grid of integer
// log-odds units and the known grid is published from it as occupancy probabilities 1 .. 99 (-1 where nothing was seen),
//     senseObserve(cfg, model, R, scan, d_truth, d_evid, d_pose, n, ..); evidencePublish(cfg, model, d_evid, d_known, d_counts, ..);
// (eea_sense_observe_batch / eea_evidence_publish; d_evid is int32 [ysize][xsize], zeroed once; the counts come with the
// publication).  The adds commute and the noise is counter-based: the grid does not depend on the order of robots, rays or calls.
// The known grid becomes the target in one of three ways:
//   the entropy surrogate -- eea_set_target_occupancy (entropy(), numerics.hpp:164-179: every unknown cell 0.7, every known one
//     1e-3; it waits for its stream);
//   the gain count -- setTargetGain(engine, cfg, R, stride, d_known, floor, lx, ly, ..): the unknown cells a scan from each cell
//     would cross (senseGainField), zero where nothing is left to see, no host wait;
//   the mutual information -- setTargetMi(engine, cfg, R, stride, p_unknown, d_known, floor, lx, ly, ..): the information that
//     scan is EXPECTED to yield (senseMiField), which reads the occupancy probabilities 1 .. 99 and discounts a cell by the
//     chance that a beam gets as far; zero once the map is known, no host wait.
// This is the simulated counterpart of a 360 degree range finder (reference README.md:74-76), not OccupancyMapper (mapping.hpp).
#pragma once

#include <cmath>
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

// The sensor model of the evidence grid: an eea_evidence_cfg, from the probabilities an inverse sensor model is usually given as
struct EvidenceModel
{
  eea_evidence_cfg cfg{};

  // p_occ / p_free: the occupancy probability one hit / one miss publishes on a cell nothing else is known of (the reference's
  // prob_occ_ 0.90 and prob_free_ 0.35, mapping.cpp:66-74); a miss is units_free evidence units, which fixes the quantum
  // -logit(p_free) / units_free, and a hit the nearest whole number of them.  (0.90, 0.35, 7) gives 25 and 7 units of
  // 0.0884341726294605: one hit publishes 90, one miss 35.  Noise-free (thr_miss = thr_false = 0) and seed 0: set cfg's fields.
  // Host only; what the library refuses (p outside (0, 1), p_free >= 0.5, units or e_clip out of range) it refuses at the call
  static EvidenceModel fromProbabilities(double p_occ, double p_free, int units_free, int e_clip)
  {
    EvidenceModel m;
    m.cfg.quantum = -std::log(p_free / (1.0 - p_free)) / static_cast<double>(units_free);
    m.cfg.w_free = units_free;
    m.cfg.w_occ = static_cast<int>(std::lround(std::log(p_occ / (1.0 - p_occ)) / m.cfg.quantum));
    m.cfg.e_clip = e_clip;
    return m;
  }
};

// one noisy scan (number `scan`) of the n_robots poses d_pose [n][3] -- robot b is robot0 + b of the fleet -- through d_truth,
// fused into d_evid (int32 [ysize][xsize], in place): + w_occ on every touched cell that appears blocking, - w_free on every
// other touched cell, once per robot and cell.  d_ranges [n][8 * range_cells] (optional): the step at which a ray met a cell that
// appeared blocking, or -1; d_mask [n] (optional): robots with 0 are left out.  range_cells <= 127.  Asynchronous
inline void senseObserve(const eea_collision_cfg& cfg, const EvidenceModel& model, unsigned int range_cells, unsigned int scan,
                         const std::int8_t* d_truth, std::int32_t* d_evid, const double* d_pose, unsigned int n_robots,
                         unsigned int robot0 = 0, int* d_ranges = nullptr, const int* d_mask = nullptr, void* stream = nullptr)
{
  throw_on_error(eea_sense_observe_batch(device_ordinal(), &cfg, &model.cfg, range_cells, scan, robot0, d_truth, d_evid, d_pose,
                                         d_mask, n_robots, d_ranges, stream));
}

// d_known [ysize][xsize] (every element overwritten) = -1 where d_evid is 0, else the occupancy probability 1 .. 99 of the
// evidence clamped to +- e_clip; d_counts [3] (optional): gridCensus of d_known, in the same launches.  Asynchronous
inline void evidencePublish(const eea_collision_cfg& cfg, const EvidenceModel& model, const std::int32_t* d_evid,
                            std::int8_t* d_known, unsigned long long* d_counts = nullptr, void* stream = nullptr)
{
  throw_on_error(eea_evidence_publish(device_ordinal(), &cfg, &model.cfg, d_evid, d_known, d_counts, stream));
}

// table [2 e_clip + 1]: entry e + e_clip is the probability evidencePublish writes for e units.  Host only
inline void evidenceTable(const EvidenceModel& model, std::int8_t* table)
{
  throw_on_error(eea_evidence_table(&model.cfg, table));
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
