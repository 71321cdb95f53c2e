// Shared declarations of the gfx950 kernels behind include/ergodic_amd.h.
// Host launchers are declared here and defined next to their kernels.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

struct eea_frontier_region;  // include/ergodic_amd.h: the record frontier_kernel.hip fills

namespace eea
{
constexpr int kBlock = 256;    // threads per workgroup: 4 wavefronts of 64 lanes
constexpr int kWave = 64;
constexpr int kMaxBasis = 32;  // K <= 32 (K^2 <= 1024 modes)
constexpr unsigned kSumGroup = 32, kSumFan = 8;  // record sum: agents per level-0 unit, level-0 records per level-1 record
__host__ __device__ constexpr int ck_record_len(int K2) { return (K2 + 2) & ~1; }

// numerics.hpp:59 of the reference
constexpr double kPi = 3.14159265358979323846;

enum : int { kModelOmni = 0, kModelSimpleCart = 1 };

// process-wide dispatch option (eea_set_option, EEA_OPT_* of include/ergodic_amd.h); defined in engine.cpp
int option(int id);
// Everything one control launch needs; passed by value (kernarg).
template <typename R>
struct ControlParams
{
  int T;              // steps_ (ergodic_control.hpp:199)
  int K;              // num_basis
  int chunk;          // points staged per contraction pass (multiple of 64)
  unsigned mem_stride;
  R dt, dt6, lx, ly, map_x, map_y, expl_weight;  // dt6 = dt / 6 (integrator.hpp:183,193)
  R half_dt;                                     // dt / 2, formed on the host: stays in scalar registers
  R pi_lx, pi_ly;     // PI / lx, PI / ly (basis.cpp:85)
  R inv_lx, inv_ly;   // 1 / lx, 1 / ly (sin/cos(pi x / lx) evaluation)
  R Rinv[9];          // column-major
  R umin[3], umax[3];
  const R* phik;      // [K^2]
  const R* lamdak;    // [K^2]
  // per-agent buffers (see eea_batch_io)
  const R* pose;
  R* ut;
  const R* mem_cols;
  const int* n_mem;
  R* u0;
  R* traj;
  R* ck;
  const R* ck_shared;  // [K^2] optional: consensus c_k used in place of the agent's own (one per launch); with
                       // ck_shared_parts > 0: that many sum records of rec_len reals (c_bar = sum of sums / sum of counts)
  int ck_shared_parts;
  int rec_len;         // K^2 + 1 rounded up to even: [sums over agents of c_k, number of agents, pad]
  // per-agent sum records (eea_batch_io::d_ck_rec): [B][rec_len] = [c_k, 1 (0 for a rejected agent), pad]; optional
  R* ck_rec;
  int rec_wave;        // eea_batch_io::rec_per_wavefront: the packed kernel writes one record per wavefront (sum of its agents')
  // device-bound exchange (eea_batch_io::d_rec_ready / d_ck_flag): rec_ready[b] = rec_seq once agent b's record is
  // visible device-wide (the record sum waits for the marks, not for the kernel); the consumer waits until
  // *ck_flag - ck_flag_seq >= 0 (mod 2^32) right before it reads ck_shared ("late binding": ~45 % into the wavefront's
  // lifetime) and reads it past its L1
  unsigned* rec_ready;
  unsigned rec_seq;
  const unsigned* ck_flag;
  unsigned ck_flag_seq;
  R* edx;
  R* bdx;
  R* rhot;
  int* status;
  const int* skip;    // [B] optional (eea_batch_io::d_skip): agents with a non-zero entry are left out of the launch
  long long* dbg;     // phase stamps of the A/B library's kernels (tools/ab/); null in the product
  // single-agent path: host-visible completion word, set to done_seq (system-scope release) after
  // u0 / status of agent 0 are written; null for batches
  int* done;
  int done_seq;
  // receding-horizon steps per launch (eea_control_batch_steps; 1 = eea_control_batch): step n reads pose row
  // n * pose_step_stride + b and writes u0 row n * u0_step_stride + b (strides in agents: 0 = the same row every step)
  int n_steps;
  unsigned pose_step_stride, u0_step_stride;
  // resident single-robot wavefront (control_wave_impl.hpp, RESIDENT instances): the host-mapped mailbox (ResidentMail<R>),
  // the request number it has seen already and the idle time (100 MHz ticks) after which it leaves; unused elsewhere
  void* res_mail;
  unsigned res_first;
  long long res_idle;
};

template <typename R>
size_t control_lds_bytes(int T, int K, int n_mem_max, int chunk);

// Launches the fused control kernel for B agents.  rollout_only: stop after the forward
// pass (optTraj), using ut as is (no shift).  Returns hipSuccess or the launch error.
template <typename R>
hipError_t launch_control(const ControlParams<R>& p, unsigned B, int model, int n_mem_max,
                          bool rollout_only, hipStream_t stream);

// The resident single-robot workgroup (control_kernel_impl.hpp control_resident_kernel; EEA_OPT_RESIDENT_CONTROL): one launch
// serves one robot's control() calls from a host-mapped mailbox until it has been idle for idle_ticks (100 MHz) or is told to
// leave.  The mailbox layout (host side: engine.cpp) is ResidentMailF64 / F32 below.
constexpr int kResidentMemCols = 128;  // capacity of the mapped replay-memory buffer (the shipped batch_size is 100)
template <typename R>
struct ResidentMail
{
  // host -> device: ONE 64-byte line, the request number written last -- the workgroup's poll fetches the whole line (16
  // lanes, one dword each: one PCIe read), so a new request number arrives together with its data
  alignas(64) R pose[3];
  R map_x, map_y;      // map_pos_ is refreshed on every call (ergodic_control.hpp:366-367)
  int n_mem;           // valid columns of the mapped replay-memory buffer
  int cmd;             // 1 = leave
  unsigned req;        // request number (only grows)
  // device -> host
  alignas(64) R u0[3];
  int status;
  int done;            // = the request's number once u0 / status are visible
  int alive;           // 0 once the workgroup has left
};
static_assert(offsetof(ResidentMail<double>, req) + sizeof(unsigned) <= 64 && offsetof(ResidentMail<double>, u0) == 64,
              "the request is one cache line");
// what the body reads instead of the mailbox: device memory, filled by the workgroup from the fetched line
template <typename R>
struct ResidentStage
{
  R pose[3];
  int n_mem;
};

template <typename R>
hipError_t launch_control_resident(const ControlParams<R>& p, int model, int n_mem_max, void* d_mail, void* d_stage,
                                   unsigned first_seen, long long idle_ticks, hipStream_t stream);

// The kernel that runs a control call, chosen in ONE place (engine.cpp control_form) for the launch, the resident form and
// the record layout (eea_batch_record_count, the consensus plan): lanes per agent -- 0 = one workgroup per agent
// (launch_control), 64 = one wavefront per agent (launch_control_wave), 8 / 16 / 32 = several agents per wavefront
// (launch_control_pack).
struct ControlForm
{
  int lanes;
  // sum records a launch of B agents writes with eea_batch_io::rec_per_wavefront: one per wavefront where agents share one
  unsigned records(unsigned B) const
  {
    if (lanes == 0 || lanes >= 64) return B;
    const unsigned A = 64u / static_cast<unsigned>(lanes);
    return (B + A - 1u) / A;
  }
};

// Wavefront-per-agent control kernel (control_wave_impl.hpp): horizons of at most 256 steps, K <= 16 or K = 20.
// launch_control_wave needs control_wave_eligible.
template <typename R>
bool control_wave_eligible(const ControlParams<R>& p);
template <typename R>
hipError_t launch_control_wave(const ControlParams<R>& p, unsigned B, int model, bool rollout_only,
                               hipStream_t stream);
// The wavefront kernel as a RESIDENT single-robot server (EEA_OPT_RESIDENT_CONTROL at horizons of one slot: fp64, T <= 64,
// K <= 16): one wavefront that serves p.res_mail until told to leave or idle.  hipErrorInvalidValue: the shape has no instance
bool control_wave_resident_eligible(const ControlParams<double>& p);
hipError_t launch_control_wave_resident(const ControlParams<double>& p, int model, hipStream_t stream);
// Several agents per wavefront (control_pack_impl.hpp): groups of 8 / 16 / 32 lanes per agent, fp64, K = 5 / 10,
// T <= 4 lanes.  control_pack_lanes: the group size for a batch of B agents (0 = one wavefront per agent); forced = the
// value of EEA_OPT_AGENT_LANES (read by control_form)
bool control_pack_eligible(const ControlParams<double>& p, int lanes);
int control_pack_lanes(const ControlParams<double>& p, unsigned B, int forced);
hipError_t launch_control_pack(const ControlParams<double>& p, unsigned B, int model, bool rollout_only, int lanes,
                               hipStream_t stream);
// sum of B per-agent records (ControlParams::ck_rec): one launch, a fixed tree (groups of kSumGroup agents in agent
// order, kSumFan group records per level-1 record, the level-1 records in order), finished by ticket inside the launch.
// d_ws: >= ck_sum_ws_elems(B, K2) reals, d_ctr: ck_sum_tickets(B, K2) tickets (zero before the first use; they reset
// themselves)
inline unsigned ck_sum_groups(unsigned B) { return (B + kSumGroup - 1) / kSumGroup; }
inline unsigned ck_sum_slices(int K2) { return static_cast<unsigned>(ck_record_len(K2) + 63) / 64u; }
inline size_t ck_sum_ws_elems(unsigned B, int K2)
{
  const size_t g0 = ck_sum_groups(B), g1 = (g0 + kSumFan - 1) / kSumFan;
  return (g0 + g1) * static_cast<size_t>(ck_record_len(K2));
}
inline size_t ck_sum_tickets(unsigned B, int K2)
{
  const size_t g1 = (ck_sum_groups(B) + kSumFan - 1) / kSumFan;
  return ck_sum_slices(K2) * (g1 + 1) + 1;  // per slice: level-1 tickets + the level-2 ticket; then the slices' ticket
}
// d_ready / seq / d_flag: the device-bound form (eea_ck_records_sum_bound): wait for rec_ready[b] == seq per agent inside
// the launch, publish *d_flag = seq behind the finished record; all null / 0: the plain form
template <typename R>
hipError_t launch_ck_records_sum(const R* d_rec, unsigned B, int K2, R* d_ws, unsigned* d_ctr, R* d_out, hipStream_t stream,
                                 const unsigned* d_ready = nullptr, unsigned seq = 0, unsigned* d_flag = nullptr);
// d_pub [n] = d_src [n] written through, then *d_flag = seq (one small launch behind an all-reduce)
template <typename R>
hipError_t launch_publish_record(const R* d_src, int n, R* d_pub, unsigned* d_flag, unsigned seq, hipStream_t stream);

// ---- phi_k path ----------------------------------------------------------------------
// Gaussians of a target passed to the fill kernel by value: [mean x, mean y (Fourier frame), cov_inv xx, yy]
constexpr int kMaxGaussArgs = 8;
constexpr int kFillPerThread = 16;  // grid points per thread of the fill kernel
template <typename R>
struct GaussArgs
{
  int n;
  R g[kMaxGaussArgs][4];
};
// both axis tables of a rebuild in one launch (cx: [K][nx], cy: [ny][K]); d_coord: the accumulated coordinates
template <typename R>
hipError_t launch_axis_tables(const R* d_coord, int nx, int ny, int K, R pi_lx, R pi_ly, R* d_cx, R* d_cy,
                              hipStream_t s);
// un-normalised Target::fill with the Gaussians in the kernel arguments; target_fill_blocks(P) partial sums
int target_fill_blocks(size_t P);
// (and, when d_cx != nullptr, the two axis tables in the same launch)
template <typename R>
hipError_t launch_target_fill_args(const R* d_coord, int nx, int ny, const GaussArgs<R>& ga, R* d_phi,
                                   R* d_partials, int K, R pi_lx, R pi_ly, R* d_cx, R* d_cy, hipStream_t s);
// configTarget for a sum of axis-aligned Gaussians in ONE launch of one workgroup: phi_k and the target's mass from the
// per-axis factors (phik_kernel.hip gaussian_phik_kernel); needs gaussian_phik_lds_bytes <= 160 KiB of LDS
size_t gaussian_phik_lds_bytes(int nx, int ny, int n_gauss, int K, size_t real_size);
template <typename R>
hipError_t launch_gaussian_phik(const R* d_coord, int nx, int ny, const GaussArgs<R>& ga, int K, R inv_lx, R inv_ly,
                                R* d_phik, R* d_mass, hipStream_t s, hipEvent_t stop = nullptr);
// spatialCoeff of an UN-normalised grid divided by its mass (the sum of d_mass_partials); d_mass[0] receives
// the mass.  stop (optional): an event bound to the completion of the last launch
template <typename R>
hipError_t launch_spatial_coeff_normalised(const R* d_phi_raw, int nx, int ny, int K, const R* d_cx, const R* d_cy,
                                           R* d_work, R* d_phik, const R* d_mass_partials, int n_mass, R* d_mass,
                                           hipStream_t s, hipEvent_t stop = nullptr);
// cos tables: out[k * n + i] = cos((k * pi_over_l) * coord[i]), k < K
template <typename R>
hipError_t launch_cos_tables(const R* d_coord, int n, int K, R pi_over_l, R* d_out, hipStream_t s);
// transposed layout: out[i * K + k]
template <typename R>
hipError_t launch_cos_tables_t(const R* d_coord, int n, int K, R pi_over_l, R* d_out, hipStream_t s);

// Target::fill without the normalisation: phi[iy*nx+ix] = sum_g exp(-0.5 d^T Sigma^-1 d).
// d_gauss: [n_gauss][4] = mean in the Fourier frame (mu - map_pos) and diag(cov_inv).
// Block partial sums of phi go to d_partials[*n_partials] (>= ceil(nx*ny/256) reals).
template <typename R>
hipError_t launch_target_fill(const R* d_xs, const R* d_ys, int nx, int ny, const R* d_gauss,
                              int n_gauss, R* d_phi, R* d_partials, int* n_partials, hipStream_t s);

// same on an arbitrary point list (d_px, d_py: P coordinates each)
template <typename R>
hipError_t launch_target_fill_points(const R* d_px, const R* d_py, unsigned P, const R* d_gauss,
                                     int n_gauss, R* d_phi, R* d_partials, int* n_partials,
                                     hipStream_t s);

// deterministic sum of n values -> d_out[0]
template <typename R>
hipError_t launch_reduce_sum(const R* d_in, int n, R* d_out, hipStream_t s);

// phi_vals *= 1 / d_sum[0]   (Target::fill's normalisation, target.cpp:87)
template <typename R>
hipError_t launch_scale_by_inv(R* d_phi, size_t n, const R* d_sum, hipStream_t s);

// spatialCoeff on a regular grid (separable form): two passes, atomics-free.
// d_cx: [K][nx], d_cy: [ny][K] (note the transposed layout of the y table),
// d_work: >= spatial_work_elems(nx, ny, K) reals, d_phik: [K^2] (col = k2*K + k1)
size_t spatial_work_elems(int nx, int ny, int K);
template <typename R>
hipError_t launch_spatial_coeff(const R* d_phi, int nx, int ny, int K, const R* d_cx, const R* d_cy,
                                R* d_work, R* d_phik, hipStream_t s);
// occupancy cells (int8) decoded through d_lut[256] inside the streaming kernel; d_raw receives the
// un-normalised sums, launch_normalise_by_first divides by element 0 -- or, with d_mass_out, the reduction launch divides
// by mode (0, 0)'s sum itself (the same bits, one launch less): d_raw = the normalised coefficients, *d_mass_out = the normaliser
template <typename R>
hipError_t launch_spatial_coeff_cells(const int8_t* d_occ, int nx, int ny, int K, const R* d_cx,
                                      const R* d_cy, const R* d_lut, R* d_work, R* d_raw, hipStream_t s,
                                      R* d_mass_out = nullptr);
template <typename R>
hipError_t launch_normalise_by_first(const R* d_raw, int K2, R* d_out, hipStream_t s);

// Weighted basis sum over an arbitrary point list (Basis::trajCoeff / spatialCoeff):
// out[m] = scale * sum_p w_p f_m(x_p, y_p); d_w may be null (w = 1).
// d_work: >= point_work_elems(P, K) reals.
size_t point_work_elems(unsigned P, int K);
template <typename R>
hipError_t launch_point_coeff(const R* d_x, const R* d_y, const R* d_w, unsigned P, int K, R pi_lx,
                              R pi_ly, R scale, R* d_work, R* d_out, hipStream_t s);

// ---- coverage fields (field_kernel.hip) --------------------------------------------------
// d_out [n_rec][nrows][nx] = the field `kind` (eea_field_kind) of the sum records d_rec [n_rec][ck_record_len(K^2)] on the grid
// rows row0 .. row0 + nrows - 1; d_cx: [K][nx], d_cy: [ny_total][K] (the layouts of launch_axis_tables), area = lx * ly
template <typename R>
hipError_t launch_records_field(int kind, unsigned n_rec, const R* d_rec, int K, const R* d_phik, const R* d_lamdak,
                                const R* d_cx, const R* d_cy, unsigned nx, unsigned row0, unsigned nrows, R area, R* d_out,
                                hipStream_t s);

// ---- collision path (integer, bit-exact) ------------------------------------------------
struct CollisionParams
{
  double xmin, ymin, resolution;
  unsigned xsize, ysize;
  int r_bnd, r_col, r_max;
  double occupied_threshold;
};
// the same grid, radii and threshold, field by field
inline bool same_params(const CollisionParams& a, const CollisionParams& b)
{
  return a.xmin == b.xmin && a.ymin == b.ymin && a.resolution == b.resolution && a.xsize == b.xsize && a.ysize == b.ysize &&
         a.r_bnd == b.r_bnd && a.r_col == b.r_col && a.r_max == b.r_max && a.occupied_threshold == b.occupied_threshold;
}
// checkCell's test !(cell / 100.0 < occupied_threshold) on getCell (collision.cpp:216-243, grid.cpp:177-184) as an integer
// cutoff, for the kernels that take it as one: the smallest int8 value v that passes it (the quotient does not fall as v
// rises, so the occupied values are an upper range of int8); 128: none does
inline int blocking_cutoff(double occupied_threshold)
{
  for (int v = -128; v <= 127; ++v) {
    if (!(static_cast<double>(v) / 100.0 < occupied_threshold)) return v;
  }
  return 128;
}
hipError_t launch_collision_check(const CollisionParams& c, const int8_t* d_grid,
                                  const double* d_pose, unsigned P, int* d_hit, hipStream_t s);
// integrate_twist (numerics.hpp:273-297) per pose; wrap: the heading normalised to [-pi, pi) afterwards
hipError_t launch_integrate_twist(const double* d_x0, const double* d_u, double dt, unsigned P, double* d_out, bool wrap, hipStream_t s);
hipError_t launch_validate_control(const CollisionParams& c, const int8_t* d_grid,
                                   const double* d_x0, const double* d_u, double dt, unsigned steps,
                                   unsigned P, int* d_valid, hipStream_t s);

struct DwaParams
{
  double dt, acc_dt, acc_lim[3], vmax[3], vmin[3];
  unsigned ns[3];  // vx, vy, vth samples (>= 1)
  unsigned steps;  // (unsigned)|horizon / dt|
};
hipError_t launch_dwa_control(const CollisionParams& c, const DwaParams& d, const int8_t* d_grid,
                              const double* d_x0, const double* d_vb, const double* d_vref,
                              const double* d_xt_ref, unsigned n_ref, double dt_ref, unsigned P,
                              double* d_u_opt, int* d_found, hipStream_t s);
// eea_tick_batch: step 1 (follow counters, skip mask) and steps 3 + 4 (validate_control; the dynamic window where it failed,
// per robot towards its own twist or along its optTraj, and the state update) of the fleet tick.  layer: null, or the fleet
// layer (below) in every collision test of both steps; robot r of the tick is robot r of the layer
struct FleetView;
hipError_t launch_tick_begin(int* d_follow, unsigned* d_count, int* d_skip, unsigned dwa_steps, unsigned P, hipStream_t s);
hipError_t launch_validate_and_dwa_fleet(const CollisionParams& c, const DwaParams& d, const FleetView* layer, const int8_t* d_grid,
                                         unsigned long long grid_epoch, const double* d_x0, const double* d_vb,
                                         const double* d_traj, unsigned n_ref, double dt_ref, double val_dt, unsigned val_steps,
                                         int* d_valid, int* d_follow, unsigned* d_count, double* d_u, int* d_source, unsigned P,
                                         hipStream_t s);
// frees the cached ring offsets and inflated-map buffers of every device
void release_collision_caches();

// ---- clearance queries: Collision::minDistance / minDirection (clearance_kernel.hip) ----------
// false: the (|d|^2, k) key of the parameter set does not fit 32 bits (hit_map_table.hpp).  Host work only, no HIP call.
bool clearance_supported(const CollisionParams& c);
// d_pose != null: the n poses [n][3]; d_pose == null: the centres of the n = xsize * ysize cells, row-major.  d_out [n][4]
// ints (msg, sqrd_obs, dx, dy), d_dmin [n], d_disp [n][2]: each may be null.  The caller has checked clearance_supported.
hipError_t launch_clearance(const CollisionParams& c, double boundary_radius, const int8_t* d_grid, const double* d_pose,
                            size_t n, int* d_out, double* d_dmin, double* d_disp, hipStream_t s);
// frees the cached visit-ordered offsets and key-map buffers of every device
void release_clearance_caches();

// ---- distance field: the exact Euclidean distance transform of the occupied cells (distance_kernel.hip) ----
// the largest xsize / ysize: a row of the plane fits a workgroup's LDS; squared distances and cell indices fit an int
constexpr unsigned kDistanceMaxSide = 8192;
// d_sq [ysize][xsize]: squared cell distance to the nearest occupied cell (-1: the grid has none); d_nearest (may be null):
// that cell's row-major index, the smallest among equals
hipError_t launch_distance_field(const CollisionParams& c, const int8_t* d_grid, int* d_sq, int* d_nearest, hipStream_t s);
// P poses [P][3] through a built field: d_out [P][4] ints (msg, sqrd_obs, dx, dy), d_dmin [P], d_disp [P][2]: each may be
// null; d_nearest may be null when d_out and d_disp are
hipError_t launch_distance_query(const CollisionParams& c, double boundary_radius, const int* d_sq, const int* d_nearest,
                                 const double* d_pose, unsigned P, int* d_out, double* d_dmin, double* d_disp, hipStream_t s);
// the worst step of each of B trajectories [B][T][3] (T >= 1): d_out [B][4], d_step [B], d_dmin [B]: each may be null;
// d_nearest may be null when d_out is
hipError_t launch_distance_traj_min(const CollisionParams& c, double boundary_radius, const int* d_sq, const int* d_nearest,
                                    const double* d_traj, unsigned B, unsigned T, int* d_out, int* d_step, double* d_dmin,
                                    hipStream_t s);

// ---- footprint collision: a convex polygon base against the occupied cells (footprint_kernel.hip) ----
// What the kernels read of a footprint, by value in the kernel arguments: the half-planes nx * bx + ny * by <= h of the body
// frame and the filter's thresholds (footprint_planes.hpp derives both on the host)
struct FootprintArgs
{
  unsigned n;
  int sq_hit, sq_free, box;
  int v_min;  // a cell is occupied iff its int8 >= v_min: blocking_cutoff(occupied_threshold)
  double nx[16], ny[16], h[16];
};
// d_hit [P] = 1 / 0 per pose of d_pose [P][3]; d_sq: a built distance field of the same grid, or null (every pose takes the
// exact test)
hipError_t launch_footprint_check(const CollisionParams& c, const FootprintArgs& f, const int8_t* d_grid, const int* d_sq,
                                  const double* d_pose, unsigned P, int* d_hit, hipStream_t s);
// d_step [B] = the first colliding step of each trajectory d_traj [B][T][3] (T >= 1), -1: none
hipError_t launch_footprint_traj_first(const CollisionParams& c, const FootprintArgs& f, const int8_t* d_grid, const int* d_sq,
                                       const double* d_traj, unsigned B, unsigned T, int* d_step, hipStream_t s);
// ---- footprint planning (footprint_plan_kernel.hip): launch_validate_control / launch_dwa_control /
// launch_validate_and_dwa_fleet with the footprint's verdict at every step; d_sq as above.  bodies: null, or the body layer
// (below) in every verdict; in the tick robot r is robot r of the layer
struct BodyView;
struct BodyArgs;
hipError_t launch_footprint_validate(const CollisionParams& c, const FootprintArgs& f, const BodyArgs* bodies, const int8_t* d_grid,
                                     const int* d_sq, const double* d_x0, const double* d_u, double dt, unsigned steps, unsigned P,
                                     int* d_valid, hipStream_t s);
hipError_t launch_footprint_dwa(const CollisionParams& c, const DwaParams& d, const FootprintArgs& f, const BodyArgs* bodies,
                                const int8_t* d_grid, const int* d_sq, const double* d_x0, const double* d_vb, const double* d_vref,
                                const double* d_xt_ref, unsigned n_ref, double dt_ref, unsigned P, double* d_u_opt, int* d_found,
                                hipStream_t s);
hipError_t launch_footprint_validate_and_dwa_fleet(const CollisionParams& c, const DwaParams& d, const FootprintArgs& f,
                                                   const BodyView* bodies, const int8_t* d_grid, const int* d_sq, const double* d_x0, const double* d_vb,
                                                   const double* d_traj, unsigned n_ref, double dt_ref, double val_dt,
                                                   unsigned val_steps, int* d_valid, int* d_follow, unsigned* d_count, double* d_u,
                                                   int* d_source, unsigned P, hipStream_t s);

// ---- fleet layer: robots as obstacles to one another (fleet_layer_kernel.hip, fleet_spans.hpp) ----
// What the collision kernels read of a layer.  count [h][w] over the centres [-R, xsize + R) x [-R, ysize + R) (the geometry
// of the inflated map with the layer's reach R = r_col + body): the number of stamped robots whose body a pose centred there
// collides with.  cell [B][2]: every robot's cell (x, y) at the last update, x = kFleetNotStamped for a robot that is no
// obstacle (masked, or outside the grid).  row_start [2R + 2] / spans: the offset set F as row spans (FleetSpan).
constexpr int kFleetNotStamped = -2147483647 - 1;
struct FleetSpan;
struct FleetView
{
  const int* count = nullptr;
  const int* cell = nullptr;
  const int* row_start = nullptr;
  const FleetSpan* spans = nullptr;
  int R = 0, w = 0, h = 0;
  unsigned B = 0;
};
// The span table of (radii, body) in the memory of `device`, built once and shared by the layers that use it.
// release_fleet_spans: a layer gives its table (named by d_row_start, the start of its allocation) back;
// release_fleet_span_cache frees the tables no layer holds.
hipError_t acquire_fleet_spans(int device, const CollisionParams& c, int body, const int** d_row_start, const FleetSpan** d_spans,
                               int* n_spans);
void release_fleet_spans(int device, const int* d_row_start);
void release_fleet_span_cache();
// One update, three stream operations and no host wait: clear the difference map, one wavefront per robot stamps +1 / -1 at
// the ends of its spans (and records its cell), a prefix sum along every row.  d_mask may be null (every robot is active)
hipError_t launch_fleet_layer_update(const CollisionParams& c, const FleetView& v, int n_spans, int* d_count, int* d_cell,
                                     const double* d_pose, const int* d_mask, hipStream_t s);
// collisionCheck of P poses with the layer: d_grid may be null (robots only), d_self may be null (no pose is a robot's own)
hipError_t launch_fleet_collision_check(const CollisionParams& c, const FleetView& v, const int8_t* d_grid, const double* d_pose,
                                        const int* d_self, unsigned P, int* d_hit, hipStream_t s);

// the layers' in-place inclusive prefix sum along every row of an int32 map [h][w] (fleet_layer_kernel.hip)
hipError_t launch_fleet_row_scan(int* d_map, int w, int h, hipStream_t s);

// ---- body layer: polygon robots as obstacles to one another (body_layer_kernel.hip) ----
// What the footprint kernels read of a layer.  cover [ysize][xsize]: the number of stamped robots whose body holds the cell.
// near [ysize + 2 box][xsize + 2 box] over the cells [-box, xsize + box) x [-box, ysize + box): the stamped robots whose cell
// lies within Chebyshev distance Rn of this one (a filter: 0 proves that no body shares a cell with a polygon placed here).
// snap [B][kBodySnap]: px, py, the sine and the cosine the stamp used, 1.0 / 0.0 = stamped or not.
constexpr int kBodySnap = 5;
constexpr unsigned kBodyLayerNoFilter = 1u;  // EEA_BODY_LAYER_NO_FILTER
struct BodyView
{
  const int* cover = nullptr;
  const int* near = nullptr;
  const double* snap = nullptr;
  int box = 0, Rn = 0, near_w = 0, near_h = 0;
  unsigned B = 0, flags = 0;
};
// the view and whose pose a query is: self [P] (null: nobody's, or with self_is_index the query's own index)
struct BodyArgs
{
  BodyView v;
  const int* self = nullptr;
  int self_is_index = 0;
};
// One update: a clear of both maps (one allocation, cover first), one stamp kernel, the row scans.  No host wait
hipError_t launch_body_layer_update(const CollisionParams& c, const FootprintArgs& f, const BodyView& v, int* d_maps, double* d_snap,
                                    const double* d_pose, const int* d_mask, hipStream_t s);
// the footprint's verdict of P poses on the grid (may be null: robots only) with the bodies of the others
hipError_t launch_body_check(const CollisionParams& c, const FootprintArgs& f, const BodyArgs& a, const int8_t* d_grid,
                             const int* d_sq, const double* d_pose, unsigned P, int* d_hit, hipStream_t s);

// ---- range sensing of a simulated fleet (sense_kernel.hip) -------------------------------
// every robot's 8 * range_cells rays through d_truth: the cells they cross are copied into d_known, d_ranges [P][8R]
// (optional) = the step at which a ray met a blocking cell or -1; c: the geometry and occupied_threshold (radii unused)
hipError_t launch_sense_reveal(const CollisionParams& c, unsigned range_cells, const int8_t* d_truth, int8_t* d_known,
                               const double* d_pose, const int* d_mask, unsigned P, int* d_ranges, hipStream_t s);
// d_counts[3] = cells < 0, cells >= 0 below the occupied threshold, blocking cells of d_grid [ysize][xsize]
hipError_t launch_grid_census(const CollisionParams& c, const int8_t* d_grid, unsigned long long* d_counts, hipStream_t s);
// (a cell blocks a ray iff cell >= blocking_cutoff(occupied_threshold), above)

// ---- evidence grid: noisy scans fused into occupancy probabilities (evidence_kernel.hip) ----
// eea_evidence_cfg, checked (entry_util.hpp: evidence_cfg_refusal)
struct EvidenceParams
{
  int w_occ, w_free, e_clip;
  double quantum;
  uint32_t thr_miss, thr_false, seed_lo, seed_hi;
};
constexpr unsigned kEvidenceMaxR = 127;     // the observe kernel's LDS window, (2R + 1)^2 bytes, must fit 64 KB
constexpr int kEvidenceMaxClip = 1024;      // the table of a publish launch: 2 * 1024 + 1 bytes in the kernel arguments
// table [2 e_clip + 1], entry e + e_clip = clamp(floor(100 sigma(e quantum) + 0.5), 1, 99); host only, the one place an exp is
// evaluated
void evidence_table(const EvidenceParams& ev, int8_t* table);
// one noisy scan of every robot's 8 * range_cells rays through d_truth, added into d_evid [ysize][xsize] (atomics: integers)
hipError_t launch_evidence_observe(const CollisionParams& c, const EvidenceParams& ev, unsigned range_cells, unsigned scan,
                                   unsigned robot0, const int8_t* d_truth, int32_t* d_evid, const double* d_pose, const int* d_mask,
                                   unsigned P, int* d_ranges, hipStream_t s);
// d_known [ysize][xsize] = -1 where d_evid is 0, else the table's byte of the clamped evidence; d_counts [3] (optional): the
// census of d_known.  The table of the launch is evidence_table's, carried as a kernel argument
hipError_t launch_evidence_publish(const CollisionParams& c, const EvidenceParams& ev, const int32_t* d_evid, int8_t* d_known,
                                   unsigned long long* d_counts, hipStream_t s);

// ---- information-gain field of a known grid (gain_kernel.hip) -----------------------------
// d_gain [ysize][xsize] = per candidate cell (both indices multiples of stride, the cell not blocking) the unknown cells the
// sensor's 8 * range_cells rays would cross from there through d_known, per beam, + 1 for an unknown own cell; 0 elsewhere
hipError_t launch_gain_field(const CollisionParams& c, unsigned range_cells, unsigned stride, const int8_t* d_known, unsigned* d_gain,
                             hipStream_t s);
// d_values [ysize][xsize] = (R)((double)gain + floor) on the candidates whose cell does not block, 0 elsewhere
template <typename R>
hipError_t launch_gain_values(const CollisionParams& c, unsigned stride, const int8_t* d_known, const unsigned* d_gain, double floor,
                              R* d_values, hipStream_t s);

// ---- mutual-information field of a known grid (mi_kernel.hip) -----------------------------
// h256 / pass256 [256], entry v + 128: h(v) and pass(v) of eea_sense_mi_table; host only, the one place a log is evaluated
void mi_table256(double occupied_threshold, double p_unknown, double* h256, double* pass256);
// d_mi [ysize][xsize] = per candidate cell (both indices multiples of stride, the cell not blocking) h(own) + the sum over the
// sensor's 8 * range_cells rays of sum_s reach_s h(v_s), reach_s = prod_{l < s} pass(v_l); +0.0 elsewhere.  The table of the
// launch is mi_table256's, carried as a kernel argument
hipError_t launch_mi_field(const CollisionParams& c, unsigned range_cells, unsigned stride, double p_unknown, const int8_t* d_known,
                           double* d_mi, hipStream_t s);
// d_values [ysize][xsize] = (R)(mi + floor) on the candidates whose cell does not block, 0 elsewhere
template <typename R>
hipError_t launch_mi_values(const CollisionParams& c, unsigned stride, const int8_t* d_known, const double* d_mi, double floor,
                            R* d_values, hipStream_t s);

// ---- geodesic field: 5-7 chamfer shortest paths through traversable cells (geodesic_kernel.hip) ----
// a workgroup owns a tile of kGeodesicTileX x kGeodesicTileY cells (the header publishes both)
constexpr unsigned kGeodesicTileX = 32, kGeodesicTileY = 32;
// the largest xsize * ysize: 7 * cells stays inside int
constexpr unsigned long long kGeodesicMaxCells = 1ull << 26;
// rounds the waiting form enqueues between two looks at the state
constexpr unsigned kGeodesicBatch = 16;
size_t geodesic_ws_bytes(unsigned xsize, unsigned ysize);
// what a call reads of its arguments beside the buffers
struct GeodesicArgs
{
  int clear_sq;
  bool unknown_blocks, keep_field;  // EEA_GEODESIC_UNKNOWN_BLOCKS, EEA_GEODESIC_CONTINUE
  unsigned P, n_cells;
};
// traversability plane, tile flags and round words into d_ws, d_geo = -1 (unless keep_field), the sources seeded, d_state =
// {0, 0, accepted sources, 0}: the state before round 0
hipError_t launch_geodesic_begin(const CollisionParams& c, const GeodesicArgs& a, const int8_t* d_grid, const int* d_sq,
                                 const double* d_pose, const int* d_cells, int* d_geo, void* d_ws, unsigned* d_state, hipStream_t s);
// rounds first .. first + count - 1, one launch each, then d_state[0] / [1] brought up to date
hipError_t launch_geodesic_rounds(const CollisionParams& c, unsigned first, unsigned count, int* d_geo, void* d_ws, unsigned* d_state,
                                  hipStream_t s);
// d_path [P][n_steps][3], d_len [P] (may be null): the descent of d_geo from each pose of d_pose [P][3]
hipError_t launch_geodesic_path(const CollisionParams& c, const int* d_geo, const double* d_pose, unsigned P, unsigned n_steps,
                                double* d_path, int* d_len, hipStream_t s);
// d_values [ysize][xsize] = (R)((double)field + floor) on the candidates whose cell does not block and has d_geo >= 0, 0
// elsewhere; kind 0: d_field is uint32, 1: double
template <typename R>
hipError_t launch_reachable_values(const CollisionParams& c, int kind, const void* d_field, unsigned stride, const int8_t* d_known,
                                   const int* d_geo, double floor, R* d_values, hipStream_t s);

// ---- geodesic partition: the field with the label of the cheapest source per cell, goals and paths (partition_kernel.hip) ----
// the workspace holds a 64-bit key per cell beside the geodesic field's planes; d_ws is 8-byte aligned
size_t partition_ws_bytes(unsigned xsize, unsigned ysize);
// traversability plane, key plane (all ones, or with keep_field rebuilt from d_geo / d_owner), tile flags and round words into
// d_ws, the sources seeded with their labels, d_state = {0, 0, accepted sources, 0}: the state before round 0
hipError_t launch_partition_begin(const CollisionParams& c, const GeodesicArgs& a, const int8_t* d_grid, const int* d_sq,
                                  const double* d_pose, const int* d_cells, const int* d_geo, const int* d_owner, void* d_ws,
                                  unsigned* d_state, hipStream_t s);
// rounds first .. first + count - 1, one launch each, d_state[0] / [1] brought up to date, the key plane unpacked into d_geo /
// d_owner
hipError_t launch_partition_rounds(const CollisionParams& c, unsigned first, unsigned count, int* d_geo, int* d_owner, void* d_ws,
                                   unsigned* d_state, hipStream_t s);
// per label < n_labels: d_area, and the candidate of the greatest score w_field * field - w_cost * geo (lowest index on a tie)
// into d_goal_cell / d_goal_score; kind 0: d_field is uint32, 1: double
hipError_t launch_partition_goals(const CollisionParams& c, int kind, const void* d_field, unsigned stride, const int8_t* d_known,
                                  const int* d_geo, const int* d_owner, unsigned n_labels, double w_field, double w_cost,
                                  int* d_goal_cell, double* d_goal_score, unsigned* d_area, hipStream_t s);
// d_path [P][n_steps][3], d_len [P] (may be null): robot q's way from its own cell to d_goal_cell[q] inside its region
hipError_t launch_partition_path(const CollisionParams& c, const int* d_geo, const int* d_owner, const double* d_pose, unsigned P,
                                 const int* d_goal_cell, unsigned n_steps, double* d_path, int* d_len, hipStream_t s);

// ---- frontier regions: the 8-connected components of a grid's frontier cells or of a mask (frontier_kernel.hip) ----
// the workspace holds two counts per 1024 cells; d_ws is 8-byte aligned
size_t frontier_ws_bytes(unsigned xsize, unsigned ysize);
// d_root / d_region [ysize][xsize], d_regions [min(n, max_regions)], d_state = {n, min(n, max_regions), members, 0}; kind:
// EEA_FRONTIER_OF_GRID / EEA_FRONTIER_OF_MASK; d_geo, d_owner, d_regions (max_regions == 0) may be null.  A fixed number of launches
hipError_t launch_frontier_regions(const CollisionParams& c, int kind, const int8_t* d_grid, const int* d_geo, const int* d_owner,
                                   unsigned max_regions, int* d_root, int* d_region, eea_frontier_region* d_regions, void* d_ws,
                                   unsigned* d_state, hipStream_t s);
// per robot q < P the record r < d_state[1] with entry_owner q, an entry and size >= min_size of the greatest score w_size * size
// - w_cost * entry_cost (lowest r on a tie) into d_goal_cell / d_goal_region / d_goal_score
hipError_t launch_frontier_goals(const eea_frontier_region* d_regions, const unsigned* d_state, unsigned max_regions, unsigned P,
                                 unsigned min_size, double w_size, double w_cost, int* d_goal_cell, int* d_goal_region,
                                 double* d_goal_score, hipStream_t s);

// ---- frontier auction: a region for every robot, by distance and capacity (auction_kernel.hip) ----
// what a call reads of its arguments beside the buffers (g: clear_sq and unknown_blocks)
struct AuctionArgs
{
  GeodesicArgs g;
  unsigned P, max_regions, min_size, cells_per_robot, n_steps;
};
// a key per cell, two unpacked planes, per robot a cell and a bid, per record slot two capacities and a count, eight words,
// and the geodesic field's planes; d_ws is 8-byte aligned
size_t auction_ws_bytes(unsigned xsize, unsigned ysize, unsigned P, unsigned max_regions);
// eight device words of d_ws: the tile rounds' state of the current build ([0]: final), then {unassigned placed robots, open
// regions} as the even and as the odd auction rounds read them
const unsigned* auction_words(const CollisionParams& c, const AuctionArgs& a, void* d_ws);
// d_state = {1, 0, 0, 0} and nothing else: what a call with no robot leaves
hipError_t launch_auction_state(unsigned* d_state, hipStream_t s);
// once per call: the traversability plane with the placed robots' cells open, their cells, every output in its "unassigned"
// state (-1; the pose in every row), the capacities, both counters, d_state = {1, 0, 0, 0}.  a.P > 0
hipError_t launch_auction_setup(const CollisionParams& c, const AuctionArgs& a, const int8_t* d_grid, const int* d_sq,
                                const eea_frontier_region* d_regions, const unsigned* d_fstate, const double* d_pose,
                                int* d_goal_region, int* d_goal_cell, int* d_goal_cost, double* d_path, int* d_len, void* d_ws,
                                unsigned* d_state, hipStream_t s);
// auction round `round`: the key plane seeded from the open regions and the state before tile round 0 (idle: no tile pending)
hipError_t launch_auction_begin(const CollisionParams& c, const AuctionArgs& a, unsigned round, const int8_t* d_grid,
                                const int* d_region, void* d_ws, hipStream_t s);
// tile rounds first .. first + count - 1 of the current build, one launch each, then its state words brought up to date
hipError_t launch_auction_rounds(const CollisionParams& c, const AuctionArgs& a, unsigned first, unsigned count, void* d_ws,
                                 hipStream_t s);
// behind the build of auction round `round`: unpack, bid, rank with accept and walk, update; d_state brought up to date
hipError_t launch_auction_settle(const CollisionParams& c, const AuctionArgs& a, unsigned round, const double* d_pose,
                                 int* d_goal_region, int* d_goal_cell, int* d_goal_cost, double* d_path, int* d_len, void* d_ws,
                                 unsigned* d_state, hipStream_t s);

// ---- goal paths: every robot's way to its own goal, one LDS window each (goto_kernel.hip) ----
// the cells of the largest window (the header publishes it): one 4-byte word per cell, 64 KB of LDS, two workgroups per CU
constexpr unsigned kGotoMaxCells = 16384;
// the workgroups of the largest launch: eight per CU at 256 CUs; a launch of fewer workgroups than robots strides over them
constexpr unsigned kGotoMaxBlocks = 2048;
// what a call reads of its arguments beside the buffers (g: clear_sq and unknown_blocks)
struct GotoArgs
{
  GeodesicArgs g;
  unsigned P, margin, n_steps;
};
// d_state = {0, 0, 0, 0}, then (a.P > 0) one workgroup per robot: d_cost, d_status, d_len (may be null) [P], d_path [P][n_steps][3]
// and the four counts of d_state {OK, WINDOW, CUT_OFF, NO_ROBOT + NO_GOAL}; d_mask [P] (may be null): 0 leaves a robot out.  Two
// launches, no workspace
hipError_t launch_goto(const CollisionParams& c, const GotoArgs& a, const int8_t* d_grid, const int* d_sq, const double* d_pose,
                       const int* d_goal, const int* d_mask, int* d_cost, int* d_status, double* d_path, int* d_len,
                       unsigned* d_state, hipStream_t s);

// ======================================================================================
// device helpers
// ======================================================================================
#if defined(__HIPCC__)

template <typename R>
__device__ __forceinline__ void sincos_r(R a, R* s, R* c);
template <>
__device__ __forceinline__ void sincos_r<double>(double a, double* s, double* c)
{
  sincos(a, s, c);
}
template <>
__device__ __forceinline__ void sincos_r<float>(float a, float* s, float* c)
{
  sincosf(a, s, c);
}

// sin(pi t), cos(pi t): exact argument reduction, no large-argument path
template <typename R>
__device__ __forceinline__ void sincospi_r(R t, R* s, R* c);
// fp64: n = rint(2t), r = t - n/2 in [-1/4, 1/4] (exact), Taylor series of sin(pi r), cos(pi r)
// in r^2 (8 and 9 terms: truncation < 5e-17), then the quadrant swap / sign from n mod 4.
// Max abs error 1.9e-16 against long-double references on 4.2e6 arguments (tools/ubench/sincos_check);
// about half the instructions of the device library's sincospi.
//  - the rounding adds 1.5 * 2^52: the sum's low word is n mod 2^32 (no conversion) for |t| < 2^50;
//    larger arguments (never produced by headings or in-domain positions) are first reduced
//    modulo 2 with v_fract (exact)
//  - Horner steps are written as v_fma_f64 with the coefficient in a scalar register pair: the
//    compiler's own choice (v_fmac_f64 on a copy of a coefficient held in vector registers) costs
//    a second instruction per step and 32 vector registers per kernel
__device__ __forceinline__ double fma_sc(double a, double b, double coeff)
{
  double d;
  asm("v_fma_f64 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "s"(coeff));
  return d;
}
__device__ __forceinline__ double mul_sc(double a, double coeff)
{
  double d;
  asm("v_mul_f64 %0, %1, %2" : "=v"(d) : "v"(a), "s"(coeff));
  return d;
}
__device__ __forceinline__ double add_sc(double a, double coeff)
{
  double d;
  asm("v_add_f64 %0, %1, %2" : "=v"(d) : "v"(a), "s"(coeff));
  return d;
}
template <>
__device__ __forceinline__ void sincospi_r<double>(double t, double* s, double* c)
{
  if (__builtin_expect(!(fabs(t) < 0x1p50), 0)) t = 2.0 * __builtin_amdgcn_fract(0.5 * t);
  // every constant comes from a scalar register pair (one per instruction is what the encoding allows): the
  // compiler's own lowering copies 64-bit literals into vector registers first (6 v_mov per evaluation)
  const double magic = 0x1.8p52;
  double nb;
  asm("v_fma_f64 %0, %1, 2.0, %2" : "=v"(nb) : "v"(t), "s"(magic));
  const int q = __double2loint(nb);
  const double n = add_sc(nb, -magic);
  const double r = fma(n, -0.5, t);
  const double z = r * r;
  // top Horner step as multiply + add (two scalar-register constants cannot share one instruction); its terms
  // are below 1e-5 of the result, so the extra rounding is invisible
  double ps = add_sc(mul_sc(z, -0x1.6fadb9f155744p-16), 0x1.e8f434d018d63p-12);
  ps = fma_sc(ps, z, -0x1.e3074fde8871fp-8);
  ps = fma_sc(ps, z, 0x1.50783487ee782p-4);
  ps = fma_sc(ps, z, -0x1.32d2cce62bd86p-1);
  ps = fma_sc(ps, z, 0x1.466bc6775aae2p+1);
  ps = fma_sc(ps, z, -0x1.4abbce625be53p+2);
  ps = fma_sc(ps, z, 0x1.921fb54442d18p+1);
  const double sv = ps * r;
  double pc = add_sc(mul_sc(z, 4.3030695870329473e-06), -0.0001046381049248457);
  pc = fma_sc(pc, z, 0.0019295743094039231);
  pc = fma_sc(pc, z, -0.025806891390014061);
  pc = fma_sc(pc, z, 0.23533063035889321);
  pc = fma_sc(pc, z, -1.3352627688545895);
  pc = fma_sc(pc, z, 4.0587121264167685);
  pc = fma_sc(pc, z, -4.934802200544679);
  pc = fma(pc, z, 1.0);
  const bool odd = (q & 1) != 0;
  const double s1 = odd ? pc : sv;
  const double c1 = odd ? sv : pc;
  // sin changes sign in quadrants 2,3; cos in quadrants 1,2
  const int ssign = (q & 2) << 30;
  const int csign = ((q + 1) & 2) << 30;
  *s = __hiloint2double(__double2hiint(s1) ^ ssign, __double2loint(s1));
  *c = __hiloint2double(__double2hiint(c1) ^ csign, __double2loint(c1));
}
// sin(pi r), cos(pi r) for |r| <= 1/16 (increments of a heading or of a basis angle over one step): no argument
// reduction, Taylor series in r^2 with 6 + 7 terms (truncation < 1e-19), 16 instructions instead of ~40
__device__ __forceinline__ void sincospi_small(double r, double* s, double* c)
{
  const double z = r * r;
  double ps = add_sc(mul_sc(z, -0.007370430945714351), 0.08214588661112823);
  ps = fma_sc(ps, z, -0.5992645293207921);
  ps = fma_sc(ps, z, 2.550164039877345);
  ps = fma_sc(ps, z, -5.16771278004997);
  ps = fma_sc(ps, z, 3.141592653589793);
  *s = ps * r;
  double pc = add_sc(mul_sc(z, 0.0019295743094039231), -0.02580689139001406);
  pc = fma_sc(pc, z, 0.2353306303588935);
  pc = fma_sc(pc, z, -1.3352627688545893);
  pc = fma_sc(pc, z, 4.058712126416768);
  pc = fma_sc(pc, z, -4.934802200544679);
  *c = fma(pc, z, 1.0);
}
__device__ __forceinline__ void sincospi_small(float r, float* s, float* c) { sincospif(r, s, c); }

template <>
__device__ __forceinline__ void sincospi_r<float>(float t, float* s, float* c)
{
  sincospif(t, s, c);
}

// numerics.hpp:78-90 of the reference: wrap to [-pi, pi)
template <typename R>
__device__ __forceinline__ R wrap_pi(R rad)
{
  const R pi = static_cast<R>(kPi);
  const R q = floor((rad + pi) / (R(2) * pi));
  rad = (rad + pi) - q * R(2) * pi;
  if (rad < R(0)) rad += R(2) * pi;
  return rad - pi;
}

// consensus c_k of mode m (eea_batch_io::d_ck_shared): the K^2 values themselves, or -- ck_shared_parts > 0 -- the
// sum of that many sum records divided by the sum of their agent counts (element K^2 of a record).  A record set that
// no agent contributed to (count 0: every agent of the producing pass was rejected, or the buffer is still zero) is no
// consensus at all: the agent keeps its own c_k (`own`) -- the reference's behaviour -- instead of 0 / 0
// agent-scope (sc1: write-through / L1-bypassing) accesses for data that crosses XCDs inside one launch
template <typename R>
__device__ __forceinline__ void store_agent(R* q, R v)
{
  __hip_atomic_store(q, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <typename R>
__device__ __forceinline__ R load_agent(const R* q)
{
  return __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The divisor is the same for every mode: the reciprocal of the summed agent counts is formed ONCE per wavefront (wavefront-
// uniform, kept in scalar registers) and the modes are multiplied by it -- the quotient per mode was nine fp64 divisions per lane
// of the wavefront kernels, 4 - 7 % of a consensus pass (profiles/r06_ablation.txt item 13).
template <typename R>
struct SharedCk
{
  R inv;      // 1 / (sum of the records' agent counts); unused with ck_shared_parts = 0
  bool have;  // some agent contributed
};
__device__ __forceinline__ double uniform_value(double v)
{
  union { double d; unsigned u[2]; } x;
  x.d = v;
  x.u[0] = __builtin_amdgcn_readfirstlane(x.u[0]);
  x.u[1] = __builtin_amdgcn_readfirstlane(x.u[1]);
  return x.d;
}
__device__ __forceinline__ float uniform_value(float v)
{
  union { float f; unsigned u; } x;
  x.f = v;
  x.u = __builtin_amdgcn_readfirstlane(x.u);
  return x.f;
}
template <typename R, typename P>  // P: ControlParams<R>, possibly in the kernel-argument address space
__device__ __forceinline__ SharedCk<R> shared_ck_begin(const P& p, const R* shared, int K2)
{
  SharedCk<R> sc{ R(1), true };
  if (p.ck_shared_parts <= 0) return sc;
  // a buffer another kernel fills WHILE this one runs (device-bound exchange) is read past the L1
  const bool bound = p.ck_flag != nullptr;
  R n = R(0);
  for (int i = 0; i < p.ck_shared_parts; ++i) {
    const R* const rec = shared + static_cast<size_t>(i) * p.rec_len;
    n += bound ? load_agent(rec + K2) : rec[K2];
  }
  n = uniform_value(n);
  sc.have = n > R(0);
  sc.inv = sc.have ? uniform_value(R(1) / n) : R(0);
  return sc;
}
template <typename R, typename P>
__device__ __forceinline__ R shared_ck_value(const P& p, const SharedCk<R>& sc, const R* shared, int m, R own)
{
  const bool bound = p.ck_flag != nullptr;
  if (p.ck_shared_parts <= 0) return bound ? load_agent(shared + m) : shared[m];
  R s = R(0);
  for (int i = 0; i < p.ck_shared_parts; ++i) {
    const R* const rec = shared + static_cast<size_t>(i) * p.rec_len;
    s += bound ? load_agent(rec + m) : rec[m];
  }
  return sc.have ? s * sc.inv : own;
}

// Device-bound exchange, consumer side: wait (bounded) until *flag has reached seq.  One lane polls past the L1 with a
// sleep between polls (MI355X_MICROARCH.md "polling-cost"); ~2 us per poll, 400 000 polls: about a second, then the
// caller reports EEA_ERR_TIMEOUT and goes on with the agent's own c_k.  Wavefront-uniform result.  The bound is a safety
// net against a producer that can never become resident, not a pacing device (every wait of the protocol is for work
// enqueued before the waiter), and generous: a loaded box must not turn a long queue into a time-out.
constexpr int kFlagPolls = 400000;
__device__ __forceinline__ bool wait_flag(const unsigned* flag, unsigned seq)
{
  for (int i = 0; i < kFlagPolls; ++i) {
    const unsigned v = __builtin_amdgcn_readfirstlane(load_agent(flag));
    if (static_cast<int>(v - seq) >= 0) return true;
    __builtin_amdgcn_s_sleep(32);
  }
  return false;
}

// std::clamp semantics (NaN passes through), ergodic_control.hpp:447-449
template <typename R>
__device__ __forceinline__ R clamp_std(R v, R lo, R hi)
{
  return (v < lo) ? lo : ((hi < v) ? hi : v);
}

template <typename R>
__device__ __forceinline__ R wave_inclusive_scan(R v)
{
  const int lane = threadIdx.x & (kWave - 1);
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const R t = __shfl_up(v, o, kWave);
    if (lane >= o) v += t;
  }
  return v;
}

// ---- matrix cores: D = A(16x4) B(4x16) + C, one operand element per lane -----------------------
// A[i][k]: lane = 16 k + i;  B[k][j]: lane = 16 k + j.  C/D: col = lane % 16 and
// row = lane/16 + 4 r (f64) or 4 (lane/16) + r (f32), r = accumulator register.
template <typename R>
struct Mfma;
template <>
struct Mfma<double>
{
  using acc_t = double __attribute__((ext_vector_type(4)));
  static __device__ __forceinline__ acc_t run(double a, double b, acc_t c)
  {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ int row(int lane, int r) { return (lane >> 4) + 4 * r; }
};
template <>
struct Mfma<float>
{
  using acc_t = float __attribute__((ext_vector_type(4)));
  static __device__ __forceinline__ acc_t run(float a, float b, acc_t c)
  {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ int row(int lane, int r) { return 4 * (lane >> 4) + r; }
};

// ---- DPP scans: row shifts inside 16-lane rows, row broadcasts across rows; no LDS traffic
// full row mask: lanes without a source read 0 through bound_ctrl (no "old" register to clear);
// partial row mask (row broadcasts): the unselected rows keep old = 0
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_or_zero(double v)
{
  constexpr bool kBound = ROW_MASK == 0xf;
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, ROW_MASK, 0xf, kBound);
  hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, ROW_MASK, 0xf, kBound);
  return __hiloint2double(hi, lo);
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_or_zero(float v)
{
  constexpr bool kBound = ROW_MASK == 0xf;
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xf, kBound));
}

// wave64 inclusive sum scan: row_shr 1,2,4,8 then row_bcast15 (rows 1,3) and row_bcast31
// (rows 2,3).  Lanes without a source keep the identity 0.
template <typename R>
__device__ __forceinline__ R wave_inclusive_scan_dpp(R v)
{
  v += dpp_or_zero<0x111, 0xf>(v);
  v += dpp_or_zero<0x112, 0xf>(v);
  v += dpp_or_zero<0x114, 0xf>(v);
  v += dpp_or_zero<0x118, 0xf>(v);
  v += dpp_or_zero<0x142, 0xa>(v);
  v += dpp_or_zero<0x143, 0xc>(v);
  return v;
}

// Inclusive scan over the workgroup (kBlock threads).  s_w: kBlock/kWave + 1 reals of LDS
// scratch.  Returns the inclusive prefix; *total receives the workgroup sum.
// Contains two __syncthreads().
template <typename R>
__device__ __forceinline__ R block_inclusive_scan(R v, R* s_w, R* total)
{
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const R s = wave_inclusive_scan(v);
  if (lane == kWave - 1) s_w[wave] = s;
  __syncthreads();
  R off = R(0), tot = R(0);
#pragma unroll
  for (int w = 0; w < kBlock / kWave; ++w) {
    const R ws = s_w[w];
    if (w < wave) off += ws;
    tot += ws;
  }
  __syncthreads();
  *total = tot;
  return s + off;
}

#endif  // __HIPCC__
}  // namespace eea
