// What the two translation units behind the C ABI share (engine.cpp: the entries that take an eea_engine; grid_entries.cpp:
// the ones that take a device or a layer): owning device memory, the checks of an eea_collision_cfg / eea_footprint /
// eea_dwa_cfg with their refusal texts, the parameter blocks made from them, and the two layers.  All inline; internal to
// libergodic_amd.so.
#pragma once

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>

#include "abi_util.hpp"
#include "common.hpp"
#include "footprint_planes.hpp"

namespace eea
{
// Device memory that goes with its owner: a member of the engine (freed by `delete e`, after eea_destroy has stopped
// everything that reads it), of a layer (freed by `delete l`, after its destroy has selected the layer's device) or a local
// of one call.  Never of static storage duration: a free during static destruction would run after the HIP runtime has gone.
struct DevBuf
{
  void* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.detach(); }
  DevBuf& operator=(DevBuf&& o) noexcept
  {
    if (this != &o) {
      release();
      cap = o.cap;
      p = o.detach();
    }
    return *this;
  }
  ~DevBuf() { release(); }
  hipError_t reserve(size_t bytes)
  {
    if (bytes <= cap) return hipSuccess;
    release();
    const hipError_t e = hipMalloc(&p, bytes);
    if (e == hipSuccess) cap = bytes;
    return e;
  }
  void release()
  {
    if (p) (void)hipFree(p);
    detach();
  }
  // the pointer, no longer owned (buffers retired behind an event: sum_workspace)
  void* detach()
  {
    void* const q = p;
    p = nullptr;
    cap = 0;
    return q;
  }
};

// device pointers cross the C ABI and sit in DevBuf untyped: as<R>(p) is p as reals of the call's precision
template <typename R>
inline R* as(void* p)
{
  return static_cast<R*>(p);
}
template <typename R>
inline const R* as(const void* p)
{
  return static_cast<const R*>(p);
}

// steps = (unsigned)|horizon / dt|: validate_control's (numerics.hpp:317) and the dynamic window's (dynamic_window.cpp:68)
inline unsigned horizon_steps(double horizon, double dt) { return static_cast<unsigned>(std::abs(horizon / dt)); }

// DynamicWindow::DynamicWindow (dynamic_window.cpp:71-90) from the C configuration
inline eea_status make_dwa_params(const eea_dwa_cfg* dcfg, eea::DwaParams& d)
{
  if (dcfg == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null DWA configuration");
  d.dt = dcfg->dt;
  d.acc_dt = dcfg->acc_dt;
  d.acc_lim[0] = dcfg->acc_lim_x;
  d.acc_lim[1] = dcfg->acc_lim_y;
  d.acc_lim[2] = dcfg->acc_lim_th;
  d.vmax[0] = dcfg->max_vel_x;
  d.vmax[1] = dcfg->max_vel_y;
  d.vmax[2] = dcfg->max_rot_vel;
  d.vmin[0] = dcfg->min_vel_x;
  d.vmin[1] = dcfg->min_vel_y;
  d.vmin[2] = dcfg->min_rot_vel;
  // a sample count of 0 is raised to 1 (DynamicWindow::DynamicWindow, dynamic_window.cpp:71-90)
  d.ns[0] = dcfg->vx_samples ? dcfg->vx_samples : 1;
  d.ns[1] = dcfg->vy_samples ? dcfg->vy_samples : 1;
  d.ns[2] = dcfg->vth_samples ? dcfg->vth_samples : 1;
  d.steps = horizon_steps(dcfg->horizon, dcfg->dt);
  if (static_cast<size_t>(d.ns[0]) * d.ns[1] * d.ns[2] > 8192) return fail(EEA_ERR_UNSUPPORTED, "more than 8192 DWA samples");
  return EEA_OK;
}

// The trajectory objective (dynamic_window.cpp:258-286) reads column round((n_ref - 1) t / tf) of the reference at every
// rollout step, tf = n_ref dt_ref; the reference's xt_ref.col(j) (:277) is bounds-checked and throws.  The kernel's own
// expression with t accumulated by repeated += dt, on the host: the call is refused when a step would read outside
// [0, n_ref - 1] (for robot r that is robot r + 1's trajectory, or memory behind the buffer) or when tf is not positive
// (dt_ref = 0: the index is NaN).
inline eea_status check_reference_index(const eea::DwaParams& d, unsigned n_ref, double dt_ref)
{
  const double tf = static_cast<double>(n_ref) * dt_ref;
  if (!(tf > 0.0)) return fail(EEA_ERR_INVALID_ARGUMENT, "the reference trajectory needs n_ref * dt_ref > 0");
  const double last = static_cast<double>(n_ref - 1);
  double t = 0.0;
  for (unsigned st = 0; st < d.steps; ++st) {
    const double jj = std::round(last * t / tf);
    if (!(jj >= 0.0 && jj <= last)) {
      return fail(EEA_ERR_INVALID_ARGUMENT, "the DWA rollout runs past the reference trajectory (step " + std::to_string(st) +
                                                " reads column " + std::to_string(jj) + " of " + std::to_string(n_ref) + ")");
    }
    t += d.dt;
  }
  return EEA_OK;
}

// What every entry that runs the dynamic window asks of it, behind the entry's own null checks: one reference -- a twist per
// robot (d_vref) or a trajectory per robot (d_xt_ref: n_ref columns every dt_ref) --, a trajectory that has columns, the
// window's parameters, and a rollout that stays on the trajectory
inline eea_status dwa_window_refusal(const eea_dwa_cfg* dcfg, const double* d_vref, const double* d_xt_ref, unsigned n_ref,
                                     double dt_ref, eea::DwaParams& d)
{
  if ((d_vref == nullptr) == (d_xt_ref == nullptr)) return fail(EEA_ERR_INVALID_ARGUMENT, "give either d_vref or d_xt_ref");
  if (d_xt_ref != nullptr && n_ref == 0) return fail(EEA_ERR_INVALID_ARGUMENT, "empty reference trajectory");
  const eea_status st = make_dwa_params(dcfg, d);
  if (st != EEA_OK || d_xt_ref == nullptr) return st;
  return check_reference_index(d, n_ref, dt_ref);
}

// The checks of an eea_collision_cfg, one refusal each.  Every entry makes the ones it needs, in its own order, before it
// selects a device, and then takes its parameters (collision_params / grid_params).
inline eea_status cfg_given(const eea_collision_cfg* cfg)
{
  return cfg != nullptr ? EEA_OK : fail(EEA_ERR_INVALID_ARGUMENT, "null collision config");
}
// Collision::Collision (collision.cpp:46-63)
inline eea_status cfg_radii_ordered(const eea_collision_cfg* cfg)
{
  if (!(cfg->search_radius < cfg->boundary_radius)) return EEA_OK;
  return fail(EEA_ERR_INVALID_ARGUMENT, "Search radius must be at least the same size as the boundary radius");
}
inline eea_status cfg_threshold_in_range(const eea_collision_cfg* cfg)
{
  if (!(cfg->occupied_threshold > 100.0 || cfg->occupied_threshold < 0.0)) return EEA_OK;
  return fail(EEA_ERR_INVALID_ARGUMENT, "Occupied threshold must be between 0 and 100");
}
// (with a size of 0 the reference's gridBounds, grid.cpp:96-100, lets every cell index through)
inline eea_status cfg_has_cells(const eea_collision_cfg* cfg)
{
  if (cfg->xsize != 0 && cfg->ysize != 0) return EEA_OK;
  return fail(EEA_ERR_INVALID_ARGUMENT, "the grid's xsize and ysize must be positive");
}
inline eea_status cfg_has_resolution(const eea_collision_cfg* cfg)
{
  return cfg->resolution > 0.0 ? EEA_OK : fail(EEA_ERR_INVALID_ARGUMENT, "the grid's resolution must be positive");
}
// what collisionCheck, validate_control, the dynamic window and a fleet layer ask first: Collision::Collision's own checks
inline eea_status collision_cfg_refusal(const eea_collision_cfg* cfg)
{
  eea_status st = cfg_given(cfg);
  if (st == EEA_OK) st = cfg_radii_ordered(cfg);
  if (st == EEA_OK) st = cfg_threshold_in_range(cfg);
  return st;
}
// what the clearance and the distance calls ask first: those around a grid the kernels can index
inline eea_status grid_query_cfg_refusal(const eea_collision_cfg* cfg)
{
  eea_status st = cfg_given(cfg);
  if (st == EEA_OK) st = cfg_has_resolution(cfg);
  if (st == EEA_OK) st = cfg_radii_ordered(cfg);
  if (st == EEA_OK) st = cfg_threshold_in_range(cfg);
  if (st == EEA_OK) st = cfg_has_cells(cfg);
  return st;
}
// what the sensor, the gain field and (behind its own arguments) a fleet layer ask of the grid
inline eea_status grid_cfg_refusal(const eea_collision_cfg* cfg)
{
  const eea_status st = cfg_has_cells(cfg);
  return st == EEA_OK ? cfg_has_resolution(cfg) : st;
}

// the geometry and the threshold of a configuration, the radii 0 (the sensor and the gain field do not read them)
inline eea::CollisionParams grid_params(const eea_collision_cfg* cfg)
{
  return eea::CollisionParams{ cfg->xmin, cfg->ymin, cfg->resolution, cfg->xsize, cfg->ysize, 0, 0, 0, cfg->occupied_threshold };
}
// ... with CollisionConfig's radii in cells (collision.cpp:130-133)
inline eea::CollisionParams collision_params(const eea_collision_cfg* cfg)
{
  eea::CollisionParams c = grid_params(cfg);
  c.r_bnd = static_cast<int>(std::floor(cfg->boundary_radius / cfg->resolution));
  c.r_col = static_cast<int>(std::floor((cfg->boundary_radius + cfg->obstacle_threshold) / cfg->resolution));
  c.r_max = static_cast<int>(std::floor(cfg->search_radius / cfg->resolution));
  return c;
}

// the footprint's own refusals (footprint_planes.hpp), before any device
inline eea_status footprint_refusal(const eea_footprint* fp, eea::FootprintPlanes& planes)
{
  if (fp == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null footprint");
  // (n is checked before a vertex is read: the arrays hold EEA_FOOTPRINT_MAX_VERTICES)
  const eea::FootprintFault fault = eea::footprint_planes(fp->n, fp->x, fp->y, planes);
  return fault == eea::FootprintFault::none ? EEA_OK : fail(EEA_ERR_INVALID_ARGUMENT, eea::footprint_fault_text(fault));
}

// the footprint on the grid of cfg (both given), in the header's order, and what the kernels read of the footprint; r_out:
// the circumscribed radius (may be null)
inline eea_status footprint_on_grid_refusal(const eea_collision_cfg* cfg, const eea_footprint* fp, eea::FootprintArgs& args,
                                            double* r_out = nullptr)
{
  eea::FootprintPlanes planes;
  eea_status st = footprint_refusal(fp, planes);
  if (st == EEA_OK) st = grid_cfg_refusal(cfg);
  if (st != EEA_OK) return st;
  if (static_cast<unsigned long long>(cfg->xsize) * cfg->ysize > (1ull << 31)) {
    return fail(EEA_ERR_UNSUPPORTED, "xsize * ysize above 2^31");
  }
  if (!eea::footprint_supported(planes, cfg->resolution)) {
    return fail(EEA_ERR_UNSUPPORTED, "the footprint's circumscribed radius is above 1024 cells");
  }
  const eea::FootprintThresholds t = eea::footprint_thresholds(planes.r_in, planes.r_out, cfg->resolution);
  args = eea::FootprintArgs{};
  args.n = planes.n;
  args.sq_hit = t.sq_hit;
  args.sq_free = t.sq_free;
  args.box = t.box;
  args.v_min = eea::blocking_cutoff(cfg->occupied_threshold);
  std::memcpy(args.nx, planes.nx, sizeof(args.nx));
  std::memcpy(args.ny, planes.ny, sizeof(args.ny));
  std::memcpy(args.h, planes.h, sizeof(args.h));
  if (r_out != nullptr) *r_out = planes.r_out;
  return EEA_OK;
}

// the checks the footprint's device calls share
inline eea_status footprint_call_refusal(const eea_collision_cfg* cfg, const eea_footprint* fp, const void* d_grid, const void* d_in,
                                         const void* d_out, eea::FootprintArgs& args)
{
  if (cfg == nullptr || fp == nullptr || d_grid == nullptr || d_in == nullptr || d_out == nullptr) {
    return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  }
  return footprint_on_grid_refusal(cfg, fp, args);
}

// the argument checks eea_sense_gain_field and eea_set_target_gain share (after their null checks), before any HIP call
inline eea_status gain_refusal(const eea_collision_cfg* cfg, unsigned range_cells, unsigned stride)
{
  const eea_status st = grid_cfg_refusal(cfg);
  if (st != EEA_OK) return st;
  if (range_cells == 0) return fail(EEA_ERR_INVALID_ARGUMENT, "range_cells must be positive");
  if (stride == 0) return fail(EEA_ERR_INVALID_ARGUMENT, "stride must be positive");
  if (range_cells > 1024u) return fail(EEA_ERR_UNSUPPORTED, "range_cells above 1024");
  return EEA_OK;
}

// what the three geodesic entries ask of the configuration, before the device is selected: the distance calls' checks, then
// the limits that keep 7 * cells inside an int
inline eea_status geodesic_cfg_refusal(const eea_collision_cfg* cfg)
{
  const eea_status st = grid_query_cfg_refusal(cfg);
  if (st != EEA_OK) return st;
  if (cfg->xsize > eea::kDistanceMaxSide || cfg->ysize > eea::kDistanceMaxSide) {
    return fail(EEA_ERR_UNSUPPORTED, "the geodesic field takes grids of up to EEA_DISTANCE_MAX_SIDE cells per side");
  }
  if (static_cast<unsigned long long>(cfg->xsize) * cfg->ysize > eea::kGeodesicMaxCells) {
    return fail(EEA_ERR_UNSUPPORTED, "the geodesic field takes grids of up to 2^26 cells");
  }
  return EEA_OK;
}

// the argument checks of eea_set_target_reachable before the target's own (target_from_field): eea_set_target_gain's without a
// range, and the field it is handed
inline eea_status reachable_refusal(const eea_collision_cfg* cfg, int kind, const void* d_field, unsigned stride, const void* d_known,
                                    const void* d_geo)
{
  if (cfg == nullptr || d_known == nullptr || d_field == nullptr || d_geo == nullptr) {
    return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  }
  const eea_status st = grid_cfg_refusal(cfg);
  if (st != EEA_OK) return st;
  if (stride == 0) return fail(EEA_ERR_INVALID_ARGUMENT, "stride must be positive");
  if (kind != 0 && kind != 1) return fail(EEA_ERR_INVALID_ARGUMENT, "kind must be 0 (gain field) or 1 (mutual-information field)");
  return EEA_OK;
}

// what the mutual-information entries ask of the probability of an unknown cell: inside (0, 1)
inline eea_status p_unknown_refusal(double p_unknown)
{
  if (p_unknown > 0.0 && p_unknown < 1.0) return EEA_OK;  // (NaN and the infinities fail both)
  return fail(EEA_ERR_INVALID_ARGUMENT, "p_unknown must lie inside (0, 1)");
}

// what the evidence entries ask of an eea_evidence_cfg (given), before any HIP call; `ev`: what the kernels read of it
inline eea_status evidence_cfg_refusal(const eea_evidence_cfg* ecfg, eea::EvidenceParams& ev)
{
  if (ecfg->w_occ < 1 || ecfg->w_occ > 32767 || ecfg->w_free < 1 || ecfg->w_free > 32767) {
    return fail(EEA_ERR_INVALID_ARGUMENT, "w_occ and w_free must lie in 1 .. 32767");
  }
  if (ecfg->e_clip < 1 || ecfg->e_clip > eea::kEvidenceMaxClip) return fail(EEA_ERR_INVALID_ARGUMENT, "e_clip must lie in 1 .. 1024");
  if (!(std::isfinite(ecfg->quantum) && ecfg->quantum > 0.0)) return fail(EEA_ERR_INVALID_ARGUMENT, "quantum must be finite and positive");
  ev = eea::EvidenceParams{ ecfg->w_occ, ecfg->w_free, ecfg->e_clip, ecfg->quantum, ecfg->thr_miss, ecfg->thr_false, ecfg->seed_lo,
                            ecfg->seed_hi };
  return EEA_OK;
}

// the message of a refusal, with the entry's name in front
inline eea_status named(const char* entry, eea_status st)
{
  if (st != EEA_OK) eea::g_last_error = std::string(entry) + ": " + eea::g_last_error;
  return st;
}

// guard words on either side of a body layer's maps, written at creation and verified by eea_body_layer_read: a stamp
// outside the maps is seen by the tests
constexpr size_t kBodyGuard = 64;
constexpr int kBodyGuardWord = 0x5a5a5a5a;
}  // namespace eea

// The layers own their device memory: `delete l` frees it, and eea_*_layer_destroy selects the layer's device first.
// ---- fleet layer: robots as obstacles to one another --------------------------------------------
struct eea_fleet_layer
{
  int device = 0, body = 0, n_spans = 0;
  eea::CollisionParams c{};
  eea::FleetView v{};            // (count / cell point at d_count / d_cell; row_start / spans are the shared span table's)
  eea::DevBuf d_count, d_cell;   // ints
};

// ---- body layer: polygon robots as obstacles to one another (body_layer_kernel.hip) ----------------
struct eea_body_layer
{
  int device = 0;
  unsigned flags = 0;
  eea_footprint fp{};
  eea::CollisionParams c{};  // the grid's geometry and threshold (grid_params)
  eea::FootprintArgs f{};
  eea::BodyView v{};         // (cover / near / snap point into maps() / d_snap)
  eea::DevBuf d_block;       // ints: kBodyGuard guard words, the maps, kBodyGuard guard words
  eea::DevBuf d_snap;        // doubles
  // cover [ysize][xsize], then near [near_h][near_w]: one clear
  int* maps() const { return static_cast<int*>(d_block.p) + eea::kBodyGuard; }
};
