// C ABI (include/ergodic_amd.h) of the entries that take a device or a layer and no engine: collision, clearance and distance
// queries, the geodesic field and its paths, the geodesic partition with its goals and paths, the frontier regions and their goals, the frontier auction, the goal paths, the footprint and its planning entries, the range sensor, the census, the evidence grid, the gain and mutual-information fields, and the two layers with their
// batch entries.  Argument checking (entry_util.hpp) and kernel dispatch; every refusal comes before the device is selected.
#include "../../include/ergodic_amd.h"

#include <cstdint>
#include <new>
#include <string>

#include "entry_util.hpp"

using namespace eea;

// ---- what eea_geodesic_field and eea_geodesic_partition share (a template has no C linkage: ahead of the entries) ----
namespace
{
// the refusals of a build in their order, before the device is selected, and what the kernels read of the arguments;
// any_null: one of the entry's own buffers is missing; misaligned, no_source: the entry's own messages
eea_status geodesic_build_args(const eea_collision_cfg* cfg, bool any_null, int clear_sq, unsigned flags, const void* d_ws,
                               unsigned ws_align, const char* misaligned, const double* d_pose, unsigned P, const int* d_cells,
                               unsigned n_cells, const char* no_source, eea::GeodesicArgs& a)
{
  const eea_status st = geodesic_cfg_refusal(cfg);
  if (st != EEA_OK) return st;
  if (any_null) return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  if ((flags & ~static_cast<unsigned>(EEA_GEODESIC_UNKNOWN_BLOCKS | EEA_GEODESIC_CONTINUE)) != 0u) {
    return fail(EEA_ERR_INVALID_ARGUMENT, "unknown flag bits");
  }
  if (clear_sq < 0) return fail(EEA_ERR_INVALID_ARGUMENT, "clear_sq must be >= 0");
  if (reinterpret_cast<uintptr_t>(d_ws) % ws_align != 0u) return fail(EEA_ERR_INVALID_ARGUMENT, misaligned);
  a.clear_sq = clear_sq;
  a.unknown_blocks = (flags & EEA_GEODESIC_UNKNOWN_BLOCKS) != 0u;
  a.keep_field = (flags & EEA_GEODESIC_CONTINUE) != 0u;
  a.P = d_pose != nullptr ? P : 0u;
  a.n_cells = d_cells != nullptr ? n_cells : 0u;
  if (a.P == 0u && a.n_cells == 0u && !a.keep_field) return fail(EEA_ERR_INVALID_ARGUMENT, no_source);
  return EEA_OK;
}

// the rounds behind a begin; launch_rounds(first, count) enqueues rounds first .. first + count - 1 with what follows them.
// A budget is enqueued whole.  The waiting form (max_rounds == 0) looks at d_state[0] behind every batch of rounds: a round
// that is not the last lowers a cell, and a cell takes finitely many values, so the cap below is never met by a build that
// converges as it must; no_fixed_point: the entry's message if it is
template <typename LaunchRounds>
eea_status geodesic_run_rounds(const eea::CollisionParams& c, unsigned max_rounds, const unsigned* d_state, hipStream_t s,
                               const char* no_fixed_point, LaunchRounds launch_rounds)
{
  if (max_rounds != 0u) {
    EEA_HIP(launch_rounds(0u, max_rounds));
    return EEA_OK;
  }
  const unsigned long long cap = static_cast<unsigned long long>(c.xsize) * c.ysize + eea::kGeodesicBatch;
  for (unsigned long long first = 0; first < cap; first += eea::kGeodesicBatch) {
    unsigned final_field = 0u;
    EEA_HIP(launch_rounds(static_cast<unsigned>(first), eea::kGeodesicBatch));
    EEA_HIP(hipMemcpyAsync(&final_field, d_state, sizeof(unsigned), hipMemcpyDeviceToHost, s));
    EEA_HIP(hipStreamSynchronize(s));
    if (final_field != 0u) return EEA_OK;
  }
  return fail(EEA_ERR_HIP, no_fixed_point);
}
}  // namespace

extern "C" {

// ---- collision lookups ---------------------------------------------------------------------
eea_status eea_collision_check_batch(int device, const eea_collision_cfg* cfg, const int8_t* d_grid,
                                     const double* d_pose, unsigned P, int* d_hit, void* stream)
{
  const eea_status st = collision_cfg_refusal(cfg);
  if (st != EEA_OK) return st;
  if (d_grid == nullptr || d_pose == nullptr || d_hit == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  const eea::CollisionParams c = collision_params(cfg);
  EEA_HIP(hipSetDevice(device));
  EEA_HIP(eea::launch_collision_check(c, d_grid, d_pose, P, d_hit, static_cast<hipStream_t>(stream)));
  return EEA_OK;
}

eea_status eea_validate_control_batch(int device, const eea_collision_cfg* cfg, const int8_t* d_grid,
                                      const double* d_x0, const double* d_u, double dt,
                                      double horizon, unsigned P, int* d_valid, void* stream)
{
  const eea_status st = collision_cfg_refusal(cfg);
  if (st != EEA_OK) return st;
  if (d_grid == nullptr || d_x0 == nullptr || d_u == nullptr || d_valid == nullptr) {
    return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  }
  const eea::CollisionParams c = collision_params(cfg);
  const unsigned steps = horizon_steps(horizon, dt);
  EEA_HIP(hipSetDevice(device));
  EEA_HIP(eea::launch_validate_control(c, d_grid, d_x0, d_u, dt, steps, P, d_valid,
                                       static_cast<hipStream_t>(stream)));
  return EEA_OK;
}

eea_status eea_integrate_twist_batch(int device, const double* d_x0, const double* d_u, double dt, unsigned P, double* d_out,
                                     int normalize_heading, void* stream)
{
  if (d_x0 == nullptr || d_u == nullptr || d_out == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  EEA_HIP(hipSetDevice(device));
  EEA_HIP(eea::launch_integrate_twist(d_x0, d_u, dt, P, d_out, normalize_heading != 0, static_cast<hipStream_t>(stream)));
  return EEA_OK;
}

// ---- clearance queries: Collision::minDistance / minDirection (collision.cpp:65-124) -----------
static_assert(sizeof(eea_clearance) == 4 * sizeof(int), "the kernels write an eea_clearance as four ints");

// the checks of the configuration both clearance calls share, before the device is selected: ... and the key bound
static eea_status clearance_cfg_refusal(const eea_collision_cfg* cfg)
{
  const eea_status st = grid_query_cfg_refusal(cfg);
  if (st != EEA_OK) return st;
  if (static_cast<unsigned long long>(cfg->xsize) * cfg->ysize > (1ull << 31)) {
    return fail(EEA_ERR_UNSUPPORTED, "xsize * ysize above 2^31");
  }
  if (!eea::clearance_supported(collision_params(cfg))) {
    return fail(EEA_ERR_UNSUPPORTED, "the search radius is too large in cells: the clearance key (|d|^2, visit index) does not fit 32 bits");
  }
  return EEA_OK;
}

eea_status eea_clearance_batch(int device, const eea_collision_cfg* cfg, const int8_t* d_grid, const double* d_pose, unsigned P,
                               eea_clearance* d_out, double* d_dmin, double* d_disp, void* stream)
{
  const eea_status st = clearance_cfg_refusal(cfg);
  if (st != EEA_OK) return st;
  if (d_grid == nullptr || d_pose == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  if (d_out == nullptr && d_dmin == nullptr && d_disp == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "no output");
  if (P == 0) return EEA_OK;
  const eea::CollisionParams c = collision_params(cfg);
  EEA_HIP(hipSetDevice(device));
  EEA_HIP(eea::launch_clearance(c, cfg->boundary_radius, d_grid, d_pose, P, reinterpret_cast<int*>(d_out), d_dmin, d_disp,
                                static_cast<hipStream_t>(stream)));
  return EEA_OK;
}

eea_status eea_clearance_field(int device, const eea_collision_cfg* cfg, const int8_t* d_grid, eea_clearance* d_field,
                               double* d_dmin, void* stream)
{
  const eea_status st = clearance_cfg_refusal(cfg);
  if (st != EEA_OK) return st;
  if (d_grid == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  if (d_field == nullptr && d_dmin == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "no output");
  const eea::CollisionParams c = collision_params(cfg);
  EEA_HIP(hipSetDevice(device));
  EEA_HIP(eea::launch_clearance(c, cfg->boundary_radius, d_grid, nullptr, static_cast<size_t>(c.xsize) * c.ysize,
                                reinterpret_cast<int*>(d_field), d_dmin, nullptr, static_cast<hipStream_t>(stream)));
  return EEA_OK;
}

// ---- distance field: the exact Euclidean distance transform of the occupied cells (distance_kernel.hip) ----
// the checks of the configuration the three distance calls share, before the device is selected
static eea_status distance_cfg_refusal(const eea_collision_cfg* cfg)
{
  const eea_status st = grid_query_cfg_refusal(cfg);
  if (st != EEA_OK) return st;
  if (cfg->xsize > eea::kDistanceMaxSide || cfg->ysize > eea::kDistanceMaxSide) {
    return fail(EEA_ERR_UNSUPPORTED, "the distance field takes grids of up to EEA_DISTANCE_MAX_SIDE cells per side");
  }
  return EEA_OK;
}

eea_status eea_distance_field(int device, const eea_collision_cfg* cfg, const int8_t* d_grid, int* d_sq, int* d_nearest, void* stream)
{
  const eea_status st = distance_cfg_refusal(cfg);
  if (st != EEA_OK) return st;
  const eea::CollisionParams c = collision_params(cfg);
  if (d_grid == nullptr || d_sq == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  EEA_HIP(hipSetDevice(device));
  EEA_HIP(eea::launch_distance_field(c, d_grid, d_sq, d_nearest, static_cast<hipStream_t>(stream)));
  return EEA_OK;
}

eea_status eea_distance_query_batch(int device, const eea_collision_cfg* cfg, const int* d_sq, const int* d_nearest,
                                    const double* d_pose, unsigned P, eea_clearance* d_out, double* d_dmin, double* d_disp,
                                    void* stream)
{
  const eea_status st = distance_cfg_refusal(cfg);
  if (st != EEA_OK) return st;
  const eea::CollisionParams c = collision_params(cfg);
  if (d_sq == nullptr || d_pose == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  if (d_out == nullptr && d_dmin == nullptr && d_disp == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "no output");
  if (d_nearest == nullptr && (d_out != nullptr || d_disp != nullptr)) {
    return fail(EEA_ERR_INVALID_ARGUMENT, "d_out and d_disp need the field's d_nearest");
  }
  if (P == 0) return EEA_OK;
  EEA_HIP(hipSetDevice(device));
  EEA_HIP(eea::launch_distance_query(c, cfg->boundary_radius, d_sq, d_nearest, d_pose, P, reinterpret_cast<int*>(d_out), d_dmin,
                                     d_disp, static_cast<hipStream_t>(stream)));
  return EEA_OK;
}

eea_status eea_distance_traj_min(int device, const eea_collision_cfg* cfg, const int* d_sq, const int* d_nearest,
                                 const double* d_traj, unsigned B, unsigned T, eea_clearance* d_out, int* d_step, double* d_dmin,
                                 void* stream)
{
  const eea_status st = distance_cfg_refusal(cfg);
  if (st != EEA_OK) return st;
  const eea::CollisionParams c = collision_params(cfg);
  if (d_sq == nullptr || d_traj == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  if (d_out == nullptr && d_step == nullptr && d_dmin == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "no output");
  if (d_nearest == nullptr && d_out != nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "d_out needs the field's d_nearest");
  if (T == 0 || T > 0x7fffffffu) return fail(EEA_ERR_INVALID_ARGUMENT, "T must be between 1 and 2^31 - 1");
  if (B == 0) return EEA_OK;
  EEA_HIP(hipSetDevice(device));
  EEA_HIP(eea::launch_distance_traj_min(c, cfg->boundary_radius, d_sq, d_nearest, d_traj, B, T, reinterpret_cast<int*>(d_out),
                                        d_step, d_dmin, static_cast<hipStream_t>(stream)));
  return EEA_OK;
}

// ---- geodesic field: 5-7 chamfer shortest paths through traversable cells (geodesic_kernel.hip) ----
eea_status eea_geodesic_ws_bytes(const eea_collision_cfg* cfg, size_t* bytes)
{
  const eea_status st = geodesic_cfg_refusal(cfg);
  if (st != EEA_OK) return st;
  if (bytes == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  *bytes = eea::geodesic_ws_bytes(cfg->xsize, cfg->ysize);
  return EEA_OK;
}

eea_status eea_geodesic_field(int device, const eea_collision_cfg* cfg, const int8_t* d_grid, const int* d_sq, int clear_sq,
                              unsigned flags, const double* d_pose, unsigned P, const int* d_cells, unsigned n_cells,
                              unsigned max_rounds, int* d_geo, void* d_ws, unsigned* d_state, void* stream)
{
  eea::GeodesicArgs a;
  const eea_status st = geodesic_build_args(cfg, d_grid == nullptr || d_geo == nullptr || d_ws == nullptr || d_state == nullptr,
                                            clear_sq, flags, d_ws, 4u, "d_ws must be 4-byte aligned", d_pose, P, d_cells, n_cells,
                                            "the geodesic field needs a source list", a);
  if (st != EEA_OK) return st;
  const eea::CollisionParams c = grid_params(cfg);
  hipStream_t s = static_cast<hipStream_t>(stream);
  EEA_HIP(hipSetDevice(device));
  EEA_HIP(eea::launch_geodesic_begin(c, a, d_grid, d_sq, d_pose, d_cells, d_geo, d_ws, d_state, s));
  return geodesic_run_rounds(c, max_rounds, d_state, s, "eea_geodesic_field: the rounds did not reach a fixed point",
                             [&](unsigned first, unsigned count) {
                               return eea::launch_geodesic_rounds(c, first, count, d_geo, d_ws, d_state, s);
                             });
}

eea_status eea_geodesic_path_batch(int device, const eea_collision_cfg* cfg, const int* d_geo, const double* d_pose, unsigned P,
                                   unsigned n_steps, double* d_path, int* d_len, void* stream)
{
  const eea_status st = geodesic_cfg_refusal(cfg);
  if (st != EEA_OK) return st;
  if (d_geo == nullptr || d_pose == nullptr || d_path == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  if (n_steps == 0u) return fail(EEA_ERR_INVALID_ARGUMENT, "n_steps must be positive");
  if (P == 0u) return EEA_OK;
  EEA_HIP(hipSetDevice(device));
  EEA_HIP(eea::launch_geodesic_path(grid_params(cfg), d_geo, d_pose, P, n_steps, d_path, d_len, static_cast<hipStream_t>(stream)));
  return EEA_OK;
}

// ---- geodesic partition: each source's share of free space, its goal and the way there (partition_kernel.hip) ----
eea_status eea_partition_ws_bytes(const eea_collision_cfg* cfg, size_t* bytes)
{
  const eea_status st = geodesic_cfg_refusal(cfg);
  if (st != EEA_OK) return st;
  if (bytes == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  *bytes = eea::partition_ws_bytes(cfg->xsize, cfg->ysize);
  return EEA_OK;
}

eea_status eea_geodesic_partition(int device, const eea_collision_cfg* cfg, const int8_t* d_grid, const int* d_sq, int clear_sq,
                                  unsigned flags, const double* d_pose, unsigned P, const int* d_cells, unsigned n_cells,
                                  unsigned max_rounds, int* d_geo, int* d_owner, void* d_ws, unsigned* d_state, void* stream)
{
  // eea_geodesic_field's refusals in its order, then the label plane's
  eea::GeodesicArgs a;
  const eea_status st = geodesic_build_args(
      cfg, d_grid == nullptr || d_geo == nullptr || d_owner == nullptr || d_ws == nullptr || d_state == nullptr, clear_sq, flags, d_ws, 8u,
      "d_ws must be 8-byte aligned", d_pose, P, d_cells, n_cells, "the geodesic partition needs a source list", a);
  if (st != EEA_OK) return st;
  if (static_cast<unsigned long long>(a.P) + a.n_cells > 0x7fffffffull) {
    return fail(EEA_ERR_UNSUPPORTED, "more than 2^31 - 1 sources: a label is a non-negative int");
  }
  const eea::CollisionParams c = grid_params(cfg);
  hipStream_t s = static_cast<hipStream_t>(stream);
  EEA_HIP(hipSetDevice(device));
  EEA_HIP(eea::launch_partition_begin(c, a, d_grid, d_sq, d_pose, d_cells, d_geo, d_owner, d_ws, d_state, s));
  // (the planes are unpacked behind every batch, so the look that finds the field final finds them written)
  return geodesic_run_rounds(c, max_rounds, d_state, s, "eea_geodesic_partition: the rounds did not reach a fixed point",
                             [&](unsigned first, unsigned count) {
                               return eea::launch_partition_rounds(c, first, count, d_geo, d_owner, d_ws, d_state, s);
                             });
}

eea_status eea_partition_goals(int device, const eea_collision_cfg* cfg, int kind, const void* d_field, unsigned stride,
                               const int8_t* d_known, const int* d_geo, const int* d_owner, unsigned n_labels, double w_field,
                               double w_cost, int* d_goal_cell, double* d_goal_score, unsigned* d_area, void* stream)
{
  if (cfg == nullptr || d_field == nullptr || d_known == nullptr || d_geo == nullptr || d_owner == nullptr || d_goal_cell == nullptr ||
      d_goal_score == nullptr || d_area == nullptr) {
    return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  }
  const eea_status st = geodesic_cfg_refusal(cfg);
  if (st != EEA_OK) return st;
  if (kind != 0 && kind != 1) return fail(EEA_ERR_INVALID_ARGUMENT, "kind must be 0 (gain field) or 1 (mutual-information field)");
  if (stride == 0) return fail(EEA_ERR_INVALID_ARGUMENT, "stride must be positive");
  // (the comparisons are false for a NaN; the cap keeps a score of a finite field finite)
  if (!(w_field >= 0.0 && w_field <= 1e30) || !(w_cost >= 0.0 && w_cost <= 1e30)) {
    return fail(EEA_ERR_INVALID_ARGUMENT, "a weight must be finite and within [0, 1e30]");
  }
  if (n_labels == 0u) return EEA_OK;
  EEA_HIP(hipSetDevice(device));
  EEA_HIP(eea::launch_partition_goals(grid_params(cfg), kind, d_field, stride, d_known, d_geo, d_owner, n_labels, w_field, w_cost,
                                      d_goal_cell, d_goal_score, d_area, static_cast<hipStream_t>(stream)));
  return EEA_OK;
}

eea_status eea_partition_path_batch(int device, const eea_collision_cfg* cfg, const int* d_geo, const int* d_owner,
                                    const double* d_pose, unsigned P, const int* d_goal_cell, unsigned n_steps, double* d_path,
                                    int* d_len, void* stream)
{
  const eea_status st = geodesic_cfg_refusal(cfg);
  if (st != EEA_OK) return st;
  if (d_geo == nullptr || d_owner == nullptr || d_pose == nullptr || d_goal_cell == nullptr || d_path == nullptr) {
    return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  }
  if (n_steps == 0u) return fail(EEA_ERR_INVALID_ARGUMENT, "n_steps must be positive");
  if (P > 0x7fffffffu) return fail(EEA_ERR_UNSUPPORTED, "more than 2^31 - 1 robots: a label is a non-negative int");
  if (P == 0u) return EEA_OK;
  EEA_HIP(hipSetDevice(device));
  EEA_HIP(eea::launch_partition_path(grid_params(cfg), d_geo, d_owner, d_pose, P, d_goal_cell, n_steps, d_path, d_len,
                                     static_cast<hipStream_t>(stream)));
  return EEA_OK;
}

// ---- frontier regions: connected frontiers, their records and a goal per robot (frontier_kernel.hip) ----
eea_status eea_frontier_ws_bytes(const eea_collision_cfg* cfg, size_t* bytes)
{
  const eea_status st = geodesic_cfg_refusal(cfg);
  if (st != EEA_OK) return st;
  if (bytes == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  *bytes = eea::frontier_ws_bytes(cfg->xsize, cfg->ysize);
  return EEA_OK;
}

eea_status eea_frontier_regions(int device, const eea_collision_cfg* cfg, int kind, const int8_t* d_grid, const int* d_geo,
                                const int* d_owner, unsigned max_regions, int* d_root, int* d_region,
                                eea_frontier_region* d_regions, void* d_ws, unsigned* d_state, void* stream)
{
  const eea_status st = geodesic_cfg_refusal(cfg);
  if (st != EEA_OK) return st;
  if (d_grid == nullptr || d_root == nullptr || d_region == nullptr || d_ws == nullptr || d_state == nullptr) {
    return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  }
  if (d_regions == nullptr && max_regions != 0u) return fail(EEA_ERR_INVALID_ARGUMENT, "d_regions is null with max_regions > 0");
  if (d_owner != nullptr && d_geo == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "d_owner needs d_geo");
  if (kind != EEA_FRONTIER_OF_GRID && kind != EEA_FRONTIER_OF_MASK) {
    return fail(EEA_ERR_INVALID_ARGUMENT, "kind must be 0 (frontier of a grid) or 1 (a mask)");
  }
  if (reinterpret_cast<uintptr_t>(d_ws) % 8u != 0u) return fail(EEA_ERR_INVALID_ARGUMENT, "d_ws must be 8-byte aligned");
  EEA_HIP(hipSetDevice(device));
  EEA_HIP(eea::launch_frontier_regions(grid_params(cfg), kind, d_grid, d_geo, d_owner, max_regions, d_root, d_region, d_regions, d_ws,
                                       d_state, static_cast<hipStream_t>(stream)));
  return EEA_OK;
}

eea_status eea_frontier_goals(int device, const eea_frontier_region* d_regions, const unsigned* d_state, unsigned max_regions,
                              unsigned P, unsigned min_size, double w_size, double w_cost, int* d_goal_cell, int* d_goal_region,
                              double* d_goal_score, void* stream)
{
  if (d_regions == nullptr || d_state == nullptr || d_goal_cell == nullptr || d_goal_region == nullptr || d_goal_score == nullptr) {
    return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  }
  // (the comparisons are false for a NaN; the cap keeps a score finite)
  if (!(w_size >= 0.0 && w_size <= 1e30) || !(w_cost >= 0.0 && w_cost <= 1e30)) {
    return fail(EEA_ERR_INVALID_ARGUMENT, "a weight must be finite and within [0, 1e30]");
  }
  if (P > 0x7fffffffu) return fail(EEA_ERR_UNSUPPORTED, "more than 2^31 - 1 robots: a label is a non-negative int");
  if (P == 0u) return EEA_OK;
  EEA_HIP(hipSetDevice(device));
  EEA_HIP(eea::launch_frontier_goals(d_regions, d_state, max_regions, P, min_size, w_size, w_cost, d_goal_cell, d_goal_region,
                                     d_goal_score, static_cast<hipStream_t>(stream)));
  return EEA_OK;
}

// ---- frontier auction: a region for every robot, by distance and capacity (auction_kernel.hip) ----
eea_status eea_frontier_auction_ws_bytes(const eea_collision_cfg* cfg, unsigned P, unsigned max_regions, size_t* bytes)
{
  const eea_status st = geodesic_cfg_refusal(cfg);
  if (st != EEA_OK) return st;
  if (bytes == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  *bytes = eea::auction_ws_bytes(cfg->xsize, cfg->ysize, P, max_regions);
  return EEA_OK;
}

eea_status eea_frontier_auction(int device, const eea_collision_cfg* cfg, const int8_t* d_grid, const int* d_sq, int clear_sq,
                                unsigned flags, const int* d_region, const eea_frontier_region* d_regions,
                                const unsigned* d_fstate, unsigned max_regions, const double* d_pose, unsigned P,
                                unsigned n_auction, unsigned min_size, unsigned cells_per_robot, unsigned max_rounds,
                                unsigned n_steps, int* d_goal_region, int* d_goal_cell, int* d_goal_cost, double* d_path,
                                int* d_len, void* d_ws, unsigned* d_state, void* stream)
{
  const eea_status st = geodesic_cfg_refusal(cfg);
  if (st != EEA_OK) return st;
  if (d_grid == nullptr || d_region == nullptr || d_fstate == nullptr || (d_pose == nullptr && P != 0u) || d_goal_region == nullptr ||
      d_goal_cell == nullptr || d_goal_cost == nullptr || d_ws == nullptr || d_state == nullptr) {
    return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  }
  if (d_regions == nullptr && max_regions != 0u) return fail(EEA_ERR_INVALID_ARGUMENT, "d_regions is null with max_regions > 0");
  if (d_path == nullptr && n_steps != 0u) return fail(EEA_ERR_INVALID_ARGUMENT, "d_path is null with n_steps > 0");
  if ((flags & ~static_cast<unsigned>(EEA_GEODESIC_UNKNOWN_BLOCKS)) != 0u) return fail(EEA_ERR_INVALID_ARGUMENT, "unknown flag bits");
  if (clear_sq < 0) return fail(EEA_ERR_INVALID_ARGUMENT, "clear_sq must be >= 0");
  if (n_auction == 0u) return fail(EEA_ERR_INVALID_ARGUMENT, "n_auction must be positive");
  if (reinterpret_cast<uintptr_t>(d_ws) % 8u != 0u) return fail(EEA_ERR_INVALID_ARGUMENT, "d_ws must be 8-byte aligned");
  if (P > 65536u) return fail(EEA_ERR_UNSUPPORTED, "more than 65536 robots: a rank is counted against every bid");
  if (max_regions > 0x7fffffffu) return fail(EEA_ERR_UNSUPPORTED, "more than 2^31 - 1 records: a label is a non-negative int");
  const eea::CollisionParams c = grid_params(cfg);
  const eea::AuctionArgs a{ eea::GeodesicArgs{ clear_sq, (flags & EEA_GEODESIC_UNKNOWN_BLOCKS) != 0u, false, P, 0u }, P, max_regions,
                            min_size, cells_per_robot, n_steps };
  hipStream_t s = static_cast<hipStream_t>(stream);
  EEA_HIP(hipSetDevice(device));
  if (P == 0u) {
    EEA_HIP(eea::launch_auction_state(d_state, s));
    return EEA_OK;
  }
  EEA_HIP(eea::launch_auction_setup(c, a, d_grid, d_sq, d_regions, d_fstate, d_pose, d_goal_region, d_goal_cell, d_goal_cost, d_path,
                                    d_len, d_ws, d_state, s));
  const unsigned* const d_words = eea::auction_words(c, a, d_ws);
  for (unsigned round = 0; round < n_auction; ++round) {
    if (max_rounds == 0u) {
      // the waiting form looks at the round's counters first: an idle round changes nothing, nor does any behind it
      unsigned counters[2] = { 0u, 0u };
      EEA_HIP(hipMemcpyAsync(counters, d_words + 4u + 2u * (round & 1u), sizeof(counters), hipMemcpyDeviceToHost, s));
      EEA_HIP(hipStreamSynchronize(s));
      if (counters[0] == 0u || counters[1] == 0u) break;
    }
    EEA_HIP(eea::launch_auction_begin(c, a, round, d_grid, d_region, d_ws, s));
    const eea_status built = geodesic_run_rounds(c, max_rounds, d_words, s, "eea_frontier_auction: the rounds did not reach a fixed point",
                                                 [&](unsigned first, unsigned count) {
                                                   return eea::launch_auction_rounds(c, a, first, count, d_ws, s);
                                                 });
    if (built != EEA_OK) return built;
    EEA_HIP(eea::launch_auction_settle(c, a, round, d_pose, d_goal_region, d_goal_cell, d_goal_cost, d_path, d_len, d_ws, d_state, s));
  }
  if (max_rounds == 0u) EEA_HIP(hipStreamSynchronize(s));
  return EEA_OK;
}

// ---- goal paths: every robot's way to its own goal, one LDS window each (goto_kernel.hip) ----
eea_status eea_geodesic_goto_batch(int device, const eea_collision_cfg* cfg, const int8_t* d_grid, const int* d_sq, int clear_sq,
                                   unsigned flags, const double* d_pose, const int* d_goal, const int* d_mask, unsigned P,
                                   unsigned margin, unsigned n_steps, int* d_cost, int* d_status, double* d_path, int* d_len,
                                   unsigned* d_state, void* stream)
{
  const eea_status st = geodesic_cfg_refusal(cfg);
  if (st != EEA_OK) return st;
  if (d_grid == nullptr || d_cost == nullptr || d_status == nullptr || d_state == nullptr) {
    return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  }
  if ((d_pose == nullptr || d_goal == nullptr) && P != 0u) return fail(EEA_ERR_INVALID_ARGUMENT, "d_pose or d_goal is null with P > 0");
  if (d_path == nullptr && n_steps != 0u) return fail(EEA_ERR_INVALID_ARGUMENT, "d_path is null with n_steps > 0");
  if ((flags & ~static_cast<unsigned>(EEA_GEODESIC_UNKNOWN_BLOCKS)) != 0u) return fail(EEA_ERR_INVALID_ARGUMENT, "unknown flag bits");
  if (clear_sq < 0) return fail(EEA_ERR_INVALID_ARGUMENT, "clear_sq must be >= 0");
  if (P > 0x7fffffffu) return fail(EEA_ERR_UNSUPPORTED, "more than 2^31 - 1 robots");
  const eea::CollisionParams c = grid_params(cfg);
  const eea::GotoArgs a{ eea::GeodesicArgs{ clear_sq, (flags & EEA_GEODESIC_UNKNOWN_BLOCKS) != 0u, false, P, 0u }, P, margin, n_steps };
  EEA_HIP(hipSetDevice(device));
  EEA_HIP(eea::launch_goto(c, a, d_grid, d_sq, d_pose, d_goal, d_mask, d_cost, d_status, d_path, d_len, d_state,
                           static_cast<hipStream_t>(stream)));
  return EEA_OK;
}

// ---- footprint collision: a convex polygon base through the distance field (footprint_kernel.hip) ----
static_assert(sizeof(eea_footprint::x) == sizeof(double) * eea::kFootprintMaxVertices, "the header states the limit");

eea_status eea_footprint_radii(const eea_footprint* fp, double* r_in, double* r_out)
{
  eea::FootprintPlanes planes;
  const eea_status st = footprint_refusal(fp, planes);
  if (st != EEA_OK) return st;
  if (r_in != nullptr) *r_in = planes.r_in;
  if (r_out != nullptr) *r_out = planes.r_out;
  return EEA_OK;
}

eea_status eea_footprint_check_batch(int device, const eea_collision_cfg* cfg, const eea_footprint* fp, const int8_t* d_grid,
                                     const int* d_sq, const double* d_pose, unsigned P, int* d_hit, void* stream)
{
  eea::FootprintArgs args;
  const eea_status st = footprint_call_refusal(cfg, fp, d_grid, d_pose, d_hit, args);
  if (st != EEA_OK) return st;
  if (P == 0) return EEA_OK;
  EEA_HIP(hipSetDevice(device));
  EEA_HIP(eea::launch_footprint_check(grid_params(cfg), args, d_grid, d_sq, d_pose, P, d_hit, static_cast<hipStream_t>(stream)));
  return EEA_OK;
}

eea_status eea_footprint_traj_first(int device, const eea_collision_cfg* cfg, const eea_footprint* fp, const int8_t* d_grid,
                                    const int* d_sq, const double* d_traj, unsigned B, unsigned T, int* d_step, void* stream)
{
  eea::FootprintArgs args;
  const eea_status st = footprint_call_refusal(cfg, fp, d_grid, d_traj, d_step, args);
  if (st != EEA_OK) return st;
  if (T == 0 || T > 0x7fffffffu) return fail(EEA_ERR_INVALID_ARGUMENT, "T must be between 1 and 2^31 - 1");
  if (B == 0) return EEA_OK;
  EEA_HIP(hipSetDevice(device));
  EEA_HIP(eea::launch_footprint_traj_first(grid_params(cfg), args, d_grid, d_sq, d_traj, B, T, d_step,
                                           static_cast<hipStream_t>(stream)));
  return EEA_OK;
}

// ---- footprint planning: the polygon base in validate_control and the dynamic window (footprint_plan_kernel.hip) ----
eea_status eea_footprint_validate_control_batch(int device, const eea_collision_cfg* cfg, const eea_footprint* fp,
                                                const int8_t* d_grid, const int* d_sq, const double* d_x0, const double* d_u,
                                                double dt, double horizon, unsigned P, int* d_valid, void* stream)
{
  eea::FootprintArgs args;
  const eea_status st = footprint_call_refusal(cfg, fp, d_grid, d_x0, d_valid, args);
  if (st != EEA_OK) return st;
  if (d_u == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  if (P == 0) return EEA_OK;
  const unsigned steps = horizon_steps(horizon, dt);
  EEA_HIP(hipSetDevice(device));
  EEA_HIP(eea::launch_footprint_validate(grid_params(cfg), args, nullptr, d_grid, d_sq, d_x0, d_u, dt, steps, P, d_valid,
                                         static_cast<hipStream_t>(stream)));
  return EEA_OK;
}

eea_status eea_footprint_dwa_control_batch(int device, const eea_collision_cfg* ccfg, const eea_dwa_cfg* dcfg,
                                           const eea_footprint* fp, const int8_t* d_grid, const int* d_sq, const double* d_x0,
                                           const double* d_vb, const double* d_vref, const double* d_xt_ref, unsigned n_ref,
                                           double dt_ref, unsigned P, double* d_u_opt, int* d_found, void* stream)
{
  eea::FootprintArgs args;
  eea_status st = footprint_call_refusal(ccfg, fp, d_grid, d_x0, d_u_opt, args);
  if (st != EEA_OK) return st;
  // eea_dwa_control_batch's, in its order
  if (dcfg == nullptr || d_vb == nullptr || d_found == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  eea::DwaParams d;
  st = dwa_window_refusal(dcfg, d_vref, d_xt_ref, n_ref, dt_ref, d);
  if (st != EEA_OK) return st;
  if (P == 0) return EEA_OK;
  EEA_HIP(hipSetDevice(device));
  EEA_HIP(eea::launch_footprint_dwa(grid_params(ccfg), d, args, nullptr, d_grid, d_sq, d_x0, d_vb, d_vref, d_xt_ref, n_ref, dt_ref, P,
                                    d_u_opt, d_found, static_cast<hipStream_t>(stream)));
  return EEA_OK;
}

void eea_release_collision_caches(void)
{
  eea::release_collision_caches();
  eea::release_clearance_caches();
  eea::release_fleet_span_cache();  // (the span tables no fleet layer holds)
}

// ---- range sensing of a simulated fleet ------------------------------------------------------
unsigned eea_sense_ray_count(unsigned range_cells) { return 8u * range_cells; }

eea_status eea_sense_reveal_batch(int device, const eea_collision_cfg* cfg, unsigned range_cells, const int8_t* d_truth,
                                  int8_t* d_known, const double* d_pose, const int* d_mask, unsigned P, int* d_ranges,
                                  void* stream)
{
  if (cfg == nullptr || d_truth == nullptr || d_known == nullptr || d_pose == nullptr) {
    return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  }
  if (d_truth == d_known) return fail(EEA_ERR_INVALID_ARGUMENT, "d_truth and d_known must be different grids");
  const eea_status st = grid_cfg_refusal(cfg);
  if (st != EEA_OK) return st;
  if (range_cells == 0) return fail(EEA_ERR_INVALID_ARGUMENT, "range_cells must be positive");
  if (range_cells > 1024u) return fail(EEA_ERR_UNSUPPORTED, "range_cells above 1024");
  if (P == 0) return EEA_OK;
  const eea::CollisionParams c = grid_params(cfg);
  EEA_HIP(hipSetDevice(device));
  EEA_HIP(eea::launch_sense_reveal(c, range_cells, d_truth, d_known, d_pose, d_mask, P, d_ranges,
                                   static_cast<hipStream_t>(stream)));
  return EEA_OK;
}

eea_status eea_grid_census(int device, const eea_collision_cfg* cfg, const int8_t* d_grid, unsigned long long* d_counts,
                           void* stream)
{
  if (cfg == nullptr || d_grid == nullptr || d_counts == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  const eea_status st = grid_cfg_refusal(cfg);
  if (st != EEA_OK) return st;
  const eea::CollisionParams c = grid_params(cfg);
  EEA_HIP(hipSetDevice(device));
  EEA_HIP(eea::launch_grid_census(c, d_grid, d_counts, static_cast<hipStream_t>(stream)));
  return EEA_OK;
}

// ---- evidence grid: noisy scans fused into occupancy probabilities (evidence_kernel.hip) ----------
eea_status eea_evidence_table(const eea_evidence_cfg* ecfg, int8_t* table)
{
  if (ecfg == nullptr || table == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  eea::EvidenceParams ev;
  const eea_status st = evidence_cfg_refusal(ecfg, ev);
  if (st != EEA_OK) return st;
  eea::evidence_table(ev, table);
  return EEA_OK;
}

eea_status eea_sense_observe_batch(int device, const eea_collision_cfg* cfg, const eea_evidence_cfg* ecfg, unsigned range_cells,
                                   unsigned scan, unsigned robot0, const int8_t* d_truth, int32_t* d_evid, const double* d_pose,
                                   const int* d_mask, unsigned P, int* d_ranges, void* stream)
{
  if (cfg == nullptr || ecfg == nullptr || d_truth == nullptr || d_evid == nullptr || d_pose == nullptr) {
    return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  }
  eea_status st = grid_cfg_refusal(cfg);
  if (st != EEA_OK) return st;
  if (range_cells == 0) return fail(EEA_ERR_INVALID_ARGUMENT, "range_cells must be positive");
  eea::EvidenceParams ev;
  st = evidence_cfg_refusal(ecfg, ev);
  if (st != EEA_OK) return st;
  if (range_cells > eea::kEvidenceMaxR) {
    return fail(EEA_ERR_UNSUPPORTED, "range_cells above 127: the scan's window of (2R + 1)^2 bytes must fit the 64 KB of LDS");
  }
  if (P == 0) return EEA_OK;
  const eea::CollisionParams c = grid_params(cfg);
  EEA_HIP(hipSetDevice(device));
  EEA_HIP(eea::launch_evidence_observe(c, ev, range_cells, scan, robot0, d_truth, d_evid, d_pose, d_mask, P, d_ranges,
                                       static_cast<hipStream_t>(stream)));
  return EEA_OK;
}

eea_status eea_evidence_publish(int device, const eea_collision_cfg* cfg, const eea_evidence_cfg* ecfg, const int32_t* d_evid,
                                int8_t* d_known, unsigned long long* d_counts, void* stream)
{
  if (cfg == nullptr || ecfg == nullptr || d_evid == nullptr || d_known == nullptr) {
    return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  }
  eea_status st = grid_cfg_refusal(cfg);
  if (st != EEA_OK) return st;
  eea::EvidenceParams ev;
  st = evidence_cfg_refusal(ecfg, ev);
  if (st != EEA_OK) return st;
  const eea::CollisionParams c = grid_params(cfg);
  EEA_HIP(hipSetDevice(device));
  EEA_HIP(eea::launch_evidence_publish(c, ev, d_evid, d_known, d_counts, static_cast<hipStream_t>(stream)));
  return EEA_OK;
}

// ---- information-gain target ------------------------------------------------------------------
eea_status eea_sense_gain_field(int device, const eea_collision_cfg* cfg, unsigned range_cells, unsigned stride,
                                const int8_t* d_known, unsigned* d_gain, void* stream)
{
  if (cfg == nullptr || d_known == nullptr || d_gain == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  const eea_status st = gain_refusal(cfg, range_cells, stride);
  if (st != EEA_OK) return st;
  const eea::CollisionParams c = grid_params(cfg);
  EEA_HIP(hipSetDevice(device));
  EEA_HIP(eea::launch_gain_field(c, range_cells, stride, d_known, d_gain, static_cast<hipStream_t>(stream)));
  return EEA_OK;
}

// ---- mutual-information target ----------------------------------------------------------------
eea_status eea_sense_mi_table(const eea_collision_cfg* cfg, double p_unknown, double* h256, double* pass256)
{
  if (cfg == nullptr || h256 == nullptr || pass256 == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  const eea_status st = eea::p_unknown_refusal(p_unknown);
  if (st != EEA_OK) return st;
  eea::mi_table256(cfg->occupied_threshold, p_unknown, h256, pass256);
  return EEA_OK;
}

eea_status eea_sense_mi_field(int device, const eea_collision_cfg* cfg, unsigned range_cells, unsigned stride, double p_unknown,
                              const int8_t* d_known, double* d_mi, void* stream)
{
  if (cfg == nullptr || d_known == nullptr || d_mi == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  eea_status st = gain_refusal(cfg, range_cells, stride);
  if (st == EEA_OK) st = eea::p_unknown_refusal(p_unknown);
  if (st != EEA_OK) return st;
  const eea::CollisionParams c = grid_params(cfg);
  EEA_HIP(hipSetDevice(device));
  EEA_HIP(eea::launch_mi_field(c, range_cells, stride, p_unknown, d_known, d_mi, static_cast<hipStream_t>(stream)));
  return EEA_OK;
}

// ---- body layer: polygon robots as obstacles to one another (body_layer_kernel.hip) ----------------
eea_status eea_body_layer_create(int device, const eea_collision_cfg* cfg, const eea_footprint* fp, unsigned B, unsigned flags,
                                 eea_body_layer** out)
{
  static const char* const entry = "eea_body_layer_create";
  if (out == nullptr) return named(entry, fail(EEA_ERR_INVALID_ARGUMENT, "null argument"));
  *out = nullptr;
  if (cfg == nullptr || fp == nullptr) return named(entry, fail(EEA_ERR_INVALID_ARGUMENT, "null argument"));
  eea::FootprintArgs f;
  eea_status st = named(entry, footprint_on_grid_refusal(cfg, fp, f));
  if (st != EEA_OK) return st;
  if (B == 0) return named(entry, fail(EEA_ERR_INVALID_ARGUMENT, "a body layer needs at least one robot"));
  if ((flags & ~EEA_BODY_LAYER_NO_FILTER) != 0u) return named(entry, fail(EEA_ERR_INVALID_ARGUMENT, "unknown flag bits"));
  // near covers the cells [-box, size + box): box <= 1025
  const unsigned long long nw = static_cast<unsigned long long>(cfg->xsize) + 2ull * static_cast<unsigned>(f.box);
  const unsigned long long nh = static_cast<unsigned long long>(cfg->ysize) + 2ull * static_cast<unsigned>(f.box);
  if (nw > 0x7fffffffull || nh > 0x7fffffffull || nw * nh > (1ull << 31) || B > 0x7fffffffu) {
    return named(entry, fail(EEA_ERR_UNSUPPORTED, "a body layer of more than 2^31 near cells or robots"));
  }
  eea_body_layer* l = new (std::nothrow) eea_body_layer();
  if (l == nullptr) return named(entry, fail(EEA_ERR_HIP, "out of host memory"));
  l->device = device;
  l->flags = flags;
  l->fp = *fp;
  l->c = grid_params(cfg);
  l->f = f;
  l->v.box = f.box;
  l->v.Rn = 2 * f.box;  // 2 ceil(r_out / res) + 2
  l->v.near_w = static_cast<int>(nw);
  l->v.near_h = static_cast<int>(nh);
  l->v.B = B;
  l->v.flags = flags;
  const size_t n_cover = static_cast<size_t>(cfg->xsize) * cfg->ysize, n_maps = n_cover + static_cast<size_t>(nw * nh);
  const size_t snap_bytes = sizeof(double) * eea::kBodySnap * static_cast<size_t>(B);
  hipError_t err = hipSetDevice(device);
  if (err == hipSuccess) err = l->d_block.reserve(sizeof(int) * (n_maps + 2 * kBodyGuard));
  if (err == hipSuccess) err = hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(l->d_block.p), kBodyGuardWord, n_maps + 2 * kBodyGuard);
  if (err == hipSuccess) err = l->d_snap.reserve(snap_bytes);
  // before the first update: no robot is an obstacle
  if (err == hipSuccess) err = hipMemset(l->maps(), 0, sizeof(int) * n_maps);
  if (err == hipSuccess) err = hipMemset(l->d_snap.p, 0, snap_bytes);
  if (err == hipSuccess) err = hipDeviceSynchronize();
  if (err != hipSuccess) {
    (void)hipGetLastError();
    const std::string msg = std::string(entry) + ": " + std::to_string(n_maps) + " map cells: " + hipGetErrorString(err);
    eea_body_layer_destroy(l);
    return fail(EEA_ERR_HIP, msg);
  }
  l->v.cover = l->maps();
  l->v.near = l->maps() + n_cover;
  l->v.snap = as<double>(l->d_snap.p);
  *out = l;
  return EEA_OK;
}

void eea_body_layer_destroy(eea_body_layer* l)
{
  if (l == nullptr) return;
  if (l->d_block.p != nullptr || l->d_snap.p != nullptr) (void)hipSetDevice(l->device);
  delete l;  // its buffers; a free waits for their users
}

eea_status eea_body_layer_update(eea_body_layer* l, const double* d_pose, const int* d_mask, void* stream)
{
  if (l == nullptr || d_pose == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "eea_body_layer_update: null argument");
  EEA_HIP(hipSetDevice(l->device));
  EEA_HIP(eea::launch_body_layer_update(l->c, l->f, l->v, l->maps(), as<double>(l->d_snap.p), d_pose, d_mask,
                                        static_cast<hipStream_t>(stream)));
  return EEA_OK;
}

eea_status eea_body_layer_read(const eea_body_layer* l, int* h_cover, int* h_near, double* h_snapshot)
{
  if (l == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "eea_body_layer_read: null argument");
  EEA_HIP(hipSetDevice(l->device));
  EEA_HIP(hipDeviceSynchronize());
  const size_t n_cover = static_cast<size_t>(l->c.xsize) * l->c.ysize, n_near = static_cast<size_t>(l->v.near_w) * l->v.near_h;
  int guard[2 * kBodyGuard];
  EEA_HIP(hipMemcpy(guard, l->d_block.p, sizeof(int) * kBodyGuard, hipMemcpyDeviceToHost));
  EEA_HIP(hipMemcpy(guard + kBodyGuard, l->maps() + n_cover + n_near, sizeof(int) * kBodyGuard, hipMemcpyDeviceToHost));
  for (size_t k = 0; k < 2 * kBodyGuard; ++k) {
    if (guard[k] != kBodyGuardWord) return fail(EEA_ERR_HIP, "eea_body_layer_read: a guard word beside the maps was overwritten");
  }
  if (h_cover != nullptr) EEA_HIP(hipMemcpy(h_cover, l->v.cover, sizeof(int) * n_cover, hipMemcpyDeviceToHost));
  if (h_near != nullptr) EEA_HIP(hipMemcpy(h_near, l->v.near, sizeof(int) * n_near, hipMemcpyDeviceToHost));
  if (h_snapshot != nullptr) {
    EEA_HIP(hipMemcpy(h_snapshot, l->d_snap.p, sizeof(double) * eea::kBodySnap * static_cast<size_t>(l->v.B), hipMemcpyDeviceToHost));
  }
  return EEA_OK;
}

int eea_body_layer_box(const eea_body_layer* l) { return l != nullptr ? l->v.box : -1; }

eea_status eea_body_collision_check_batch(const eea_body_layer* l, const int8_t* d_grid, const int* d_sq, const double* d_pose,
                                          const int* d_self, unsigned P, int* d_hit, void* stream)
{
  // (the layer last: every other refusal can be reached without one)
  if (d_pose == nullptr || d_hit == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "eea_body_collision_check_batch: null argument");
  if (l == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "eea_body_collision_check_batch: null body layer");
  if (P == 0) return EEA_OK;
  EEA_HIP(hipSetDevice(l->device));
  const eea::BodyArgs a{ l->v, d_self, 0 };
  EEA_HIP(eea::launch_body_check(l->c, l->f, a, d_grid, d_sq, d_pose, P, d_hit, static_cast<hipStream_t>(stream)));
  return EEA_OK;
}

eea_status eea_body_validate_control_batch(const eea_body_layer* l, const int8_t* d_grid, const int* d_sq, const double* d_x0,
                                           const double* d_u, const int* d_self, double dt, double horizon, unsigned P,
                                           int* d_valid, void* stream)
{
  if (d_grid == nullptr || d_x0 == nullptr || d_valid == nullptr || d_u == nullptr) {
    return fail(EEA_ERR_INVALID_ARGUMENT, "eea_body_validate_control_batch: null argument");
  }
  if (l == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "eea_body_validate_control_batch: null body layer");
  if (P == 0) return EEA_OK;
  const unsigned steps = horizon_steps(horizon, dt);
  EEA_HIP(hipSetDevice(l->device));
  const eea::BodyArgs a{ l->v, d_self, 0 };
  EEA_HIP(eea::launch_footprint_validate(l->c, l->f, &a, d_grid, d_sq, d_x0, d_u, dt, steps, P, d_valid, static_cast<hipStream_t>(stream)));
  return EEA_OK;
}

eea_status eea_body_dwa_control_batch(const eea_body_layer* l, const eea_dwa_cfg* dcfg, const int8_t* d_grid, const int* d_sq,
                                      const double* d_x0, const double* d_vb, const double* d_vref, const double* d_xt_ref,
                                      unsigned n_ref, double dt_ref, const int* d_self, unsigned P, double* d_u_opt, int* d_found,
                                      void* stream)
{
  static const char* const entry = "eea_body_dwa_control_batch";
  if (d_grid == nullptr || d_x0 == nullptr || d_u_opt == nullptr || dcfg == nullptr || d_vb == nullptr || d_found == nullptr) {
    return named(entry, fail(EEA_ERR_INVALID_ARGUMENT, "null argument"));
  }
  eea::DwaParams d;
  const eea_status st = named(entry, dwa_window_refusal(dcfg, d_vref, d_xt_ref, n_ref, dt_ref, d));
  if (st != EEA_OK) return st;
  if (l == nullptr) return named(entry, fail(EEA_ERR_INVALID_ARGUMENT, "null body layer"));
  if (P == 0) return EEA_OK;
  EEA_HIP(hipSetDevice(l->device));
  const eea::BodyArgs a{ l->v, d_self, 0 };
  EEA_HIP(eea::launch_footprint_dwa(l->c, d, l->f, &a, d_grid, d_sq, d_x0, d_vb, d_vref, d_xt_ref, n_ref, dt_ref, P, d_u_opt, d_found,
                                    static_cast<hipStream_t>(stream)));
  return EEA_OK;
}

// ---- fleet layer: robots as obstacles to one another --------------------------------------------
eea_status eea_fleet_layer_create(int device, const eea_collision_cfg* cfg, int body_cells, unsigned B, eea_fleet_layer** out)
{
  if (out == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  *out = nullptr;
  eea_status st = collision_cfg_refusal(cfg);
  if (st != EEA_OK) return st;
  if (B == 0) return fail(EEA_ERR_INVALID_ARGUMENT, "a fleet layer needs at least one robot");
  if (body_cells < 0) return fail(EEA_ERR_INVALID_ARGUMENT, "the body radius of a fleet layer must be >= 0 cells");
  st = grid_cfg_refusal(cfg);
  if (st != EEA_OK) return st;
  const eea::CollisionParams c = collision_params(cfg);
  if (c.r_bnd < 0 || c.r_col < 0) return fail(EEA_ERR_INVALID_ARGUMENT, "the collision radii must not be negative");
  // the reach R' = r_col + body (the span table holds shorts; the padded map grows by R' on every side)
  if (c.r_col > 127 || body_cells > 127 || c.r_col + body_cells > 127) {
    return fail(EEA_ERR_UNSUPPORTED, "a fleet layer's reach r_col + body above 127 cells");
  }
  const int R = c.r_col + body_cells;
  const unsigned long long w = static_cast<unsigned long long>(c.xsize) + 2u * R, h = static_cast<unsigned long long>(c.ysize) + 2u * R;
  if (w > 0x7fffffffull || h > 0x7fffffffull || w * h > (1ull << 31) || B > 0x7fffffffu) {
    return fail(EEA_ERR_UNSUPPORTED, "a fleet layer of more than 2^31 centres or robots");
  }
  eea_fleet_layer* l = new (std::nothrow) eea_fleet_layer();
  if (l == nullptr) return fail(EEA_ERR_HIP, "fleet layer: out of host memory");
  l->device = device;
  l->body = body_cells;
  l->c = c;
  l->v.R = R;
  l->v.w = static_cast<int>(w);
  l->v.h = static_cast<int>(h);
  l->v.B = B;
  hipError_t err = hipSetDevice(device);
  if (err == hipSuccess) err = eea::acquire_fleet_spans(device, c, body_cells, &l->v.row_start, &l->v.spans, &l->n_spans);
  if (err == hipSuccess) err = l->d_count.reserve(sizeof(int) * static_cast<size_t>(w * h));
  if (err == hipSuccess) err = l->d_cell.reserve(sizeof(int) * 2 * static_cast<size_t>(B));
  // before the first update: no robot is an obstacle
  if (err == hipSuccess) err = hipMemset(l->d_count.p, 0, sizeof(int) * static_cast<size_t>(w * h));
  if (err == hipSuccess) err = hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(l->d_cell.p), eea::kFleetNotStamped, 2 * static_cast<size_t>(B));
  if (err == hipSuccess) err = hipDeviceSynchronize();  // (the fills are done when the layer is handed out, whatever stream reads it)
  if (err != hipSuccess) {
    (void)hipGetLastError();
    const std::string msg = std::string("fleet layer of ") + std::to_string(w) + " x " + std::to_string(h) + " centres: " + hipGetErrorString(err);
    eea_fleet_layer_destroy(l);
    return fail(EEA_ERR_HIP, msg);
  }
  l->v.count = as<int>(l->d_count.p);
  l->v.cell = as<int>(l->d_cell.p);
  *out = l;
  return EEA_OK;
}

void eea_fleet_layer_destroy(eea_fleet_layer* l)
{
  if (l == nullptr) return;
  if (l->v.row_start != nullptr) eea::release_fleet_spans(l->device, l->v.row_start);
  if (l->d_count.p != nullptr || l->d_cell.p != nullptr) (void)hipSetDevice(l->device);
  delete l;  // its buffers; a free waits for their users
}

int eea_fleet_layer_reach(const eea_fleet_layer* l) { return l != nullptr ? l->v.R : -1; }

eea_status eea_fleet_layer_update(eea_fleet_layer* l, const double* d_pose, const int* d_mask, void* stream)
{
  if (l == nullptr || d_pose == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  EEA_HIP(hipSetDevice(l->device));
  EEA_HIP(eea::launch_fleet_layer_update(l->c, l->v, l->n_spans, as<int>(l->d_count.p), as<int>(l->d_cell.p), d_pose, d_mask,
                                         static_cast<hipStream_t>(stream)));
  return EEA_OK;
}

eea_status eea_fleet_layer_read(const eea_fleet_layer* l, int* h_count, int* h_cell)
{
  if (l == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  EEA_HIP(hipSetDevice(l->device));
  EEA_HIP(hipDeviceSynchronize());
  if (h_count != nullptr) EEA_HIP(hipMemcpy(h_count, l->v.count, sizeof(int) * static_cast<size_t>(l->v.w) * l->v.h, hipMemcpyDeviceToHost));
  if (h_cell != nullptr) EEA_HIP(hipMemcpy(h_cell, l->v.cell, sizeof(int) * 2 * static_cast<size_t>(l->v.B), hipMemcpyDeviceToHost));
  return EEA_OK;
}

eea_status eea_fleet_collision_check_batch(const eea_fleet_layer* l, const int8_t* d_grid, const double* d_pose, const int* d_self,
                                           unsigned P, int* d_hit, void* stream)
{
  if (l == nullptr || d_pose == nullptr || d_hit == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  EEA_HIP(hipSetDevice(l->device));
  EEA_HIP(eea::launch_fleet_collision_check(l->c, l->v, d_grid, d_pose, d_self, P, d_hit, static_cast<hipStream_t>(stream)));
  return EEA_OK;
}

eea_status eea_dwa_control_batch(int device, const eea_collision_cfg* ccfg, const eea_dwa_cfg* dcfg,
                                 const int8_t* d_grid, const double* d_x0, const double* d_vb,
                                 const double* d_vref, const double* d_xt_ref, unsigned n_ref,
                                 double dt_ref, unsigned P, double* d_u_opt, int* d_found, void* stream)
{
  eea_status st = collision_cfg_refusal(ccfg);
  if (st != EEA_OK) return st;
  const eea::CollisionParams c = collision_params(ccfg);
  if (dcfg == nullptr || d_grid == nullptr || d_x0 == nullptr || d_vb == nullptr || d_u_opt == nullptr ||
      d_found == nullptr) {
    return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  }
  eea::DwaParams d;
  st = dwa_window_refusal(dcfg, d_vref, d_xt_ref, n_ref, dt_ref, d);
  if (st != EEA_OK) return st;
  EEA_HIP(hipSetDevice(device));
  EEA_HIP(eea::launch_dwa_control(c, d, d_grid, d_x0, d_vb, d_vref, d_xt_ref, n_ref, dt_ref, P, d_u_opt,
                                  d_found, static_cast<hipStream_t>(stream)));
  return EEA_OK;
}

}  // extern "C"
