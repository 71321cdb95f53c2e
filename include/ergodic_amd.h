/*
 * ergodic_amd.h -- C ABI of the MI355X (gfx950) ergodic receding-horizon engine.
 *
 * This is the drop-in boundary for the hot path of bostoncleek/ergodic_exploration:
 * one call of `ErgodicControl<ModelT>::control` (ergodic_control.hpp:224-311) plus the
 * phi_k rebuild `configTarget` (ergodic_control.hpp:362-416), for ModelT in
 * {models::Omni, models::SimpleCart}.  The reference has no FFI layer (its boundary is
 * the C++ template class); each entry point below names the reference interface it
 * replaces (file:line relative to the reference root).  INTEGRATION.md shows the binding a
 * maintainer adds on the reference side.
 *
 * Conventions
 *  - plain C types only; every function returns an eea_status (0 = ok); no exceptions
 *    cross the ABI.  eea_last_error() gives the message of the last failure on the
 *    calling thread.
 *  - "real" = double (EEA_PREC_F64) or float (EEA_PREC_F32), fixed per engine.
 *  - matrices use the reference's Armadillo layout: a "3 x T" matrix is T contiguous
 *    [x, y, theta] (or [vx, vy, w]) triples (column-major).
 *  - pointers named d_* are DEVICE pointers (HBM, caller-owned, same device as the
 *    engine); pointers named h_* / plain arrays are host memory.
 *  - `stream` is a hipStream_t passed as void* (NULL = the default stream); batch calls
 *    are asynchronous on it.  One engine per host thread (reentrant across engines).
 */
#ifndef ERGODIC_AMD_H
#define ERGODIC_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EEA_ABI_VERSION 6

/* models usable with ErgodicControl (Cart/Mecanum cannot run under it) */
enum { EEA_MODEL_OMNI = 0,        /* models::Omni        models/omni.hpp:164-215 */
       EEA_MODEL_SIMPLE_CART = 1  /* models::SimpleCart  models/cart.hpp:152-206 */ };

enum { EEA_PREC_F64 = 0, EEA_PREC_F32 = 1 };

typedef enum {
  EEA_OK = 0,
  EEA_ERR_INVALID_ARGUMENT = 1, /* reference: std::invalid_argument from a constructor */
  EEA_ERR_INVALID_TWIST = 2,    /* reference: SimpleCart::operator() throws, cart.hpp:167-170 */
  EEA_ERR_UNSUPPORTED = 3,      /* size outside what the kernels are built for */
  EEA_ERR_HIP = 4,              /* HIP runtime failure (no device, OOM, launch error) */
  EEA_ERR_NO_TARGET = 5,        /* control requested before any target was set */
  EEA_ERR_TIMEOUT = 6           /* per-agent status of the device-bound exchange: the shared c_k an agent waited for
                                   inside the kernel did not arrive (eea_batch_io::d_ck_flag); it used its own c_k */
} eea_status;

typedef struct eea_engine eea_engine;

/* Constructor arguments of ErgodicControl (ergodic_control.hpp:90-94, 187-222).
 * collision / buffer_size / batch_size are not engine state (the collision object is never read on this path; the
 * sampled replay-memory columns come in through mem_cols: from the host's ReplayBuffer for one robot, from the device
 * replay memory of a fleet -- eea_replay_* below, which takes buffer_size / batch_size -- without leaving the device). */
typedef struct {
  int model;          /* EEA_MODEL_* */
  int precision;      /* EEA_PREC_* */
  int device;         /* HIP device ordinal */
  double dt;          /* time step in integration */
  double horizon;     /* control horizon; steps = (unsigned)|horizon/dt| (truncating) */
  double resolution;  /* target grid resolution [m] */
  double expl_weight; /* ergodic exploration weight */
  unsigned num_basis; /* K: cosine basis functions per dimension (K^2 modes) */
  double Rinv[9];     /* inverse control weights, column-major 3x3 */
  double umin[3];     /* body twist lower limits */
  double umax[3];     /* body twist upper limits */
} eea_config;

/* ---- life cycle -------------------------------------------------------------------- */
/* ErgodicControl::ErgodicControl (ergodic_control.hpp:187-222).  EEA_ERR_INVALID_ARGUMENT
 * if steps == 1 (the reference throws) or steps == 0 (the reference has UB). */
eea_status eea_create(const eea_config* cfg, eea_engine** out);
void eea_destroy(eea_engine* e);
const char* eea_last_error(void);
unsigned eea_abi_version(void);

/* Process-wide dispatch options (no reference counterpart; every default reproduces the engine's own choice).
 * They replace the environment knobs of ABI 2: the library reads no environment variable. */
enum { EEA_OPT_CONTROL_KERNEL = 0,    /* 0 = automatic (wavefront-per-agent kernel where eligible), 1 = the
                                         workgroup-per-agent kernel for every control call */
       EEA_OPT_WORKGROUP_THREADS = 1, /* threads per agent of the workgroup-per-agent kernel: 0 = by horizon,
                                         or 64 / 128 / 256 */
       EEA_OPT_COLLISION_IMPL = 2,    /* Collision::collisionCheck implementation: 0 = cost model, 1 = ring
                                         search, 2 = inflated map (both bit-exact) */
       EEA_OPT_MAILBOX_POLL = 3,      /* eea_control: 1 = poll the completion word (default), 0 = wait for the stream */
       EEA_OPT_REBUILD_IMPL = 4,      /* configTarget rebuild of a Gaussian target: 0 = automatic (per-axis factors, one
                                         launch of one workgroup), 1 = fill the grid and stream it (Target::fill +
                                         Basis::spatialCoeff as two / three launches: what explicit grids take) */
       EEA_OPT_AGENT_LANES = 5,       /* lanes of a wavefront per agent in eea_control_batch[_steps] (short horizons share
                                         a wavefront: T <= 4 lanes, fp64, K = 5 / 10): 0 = by batch size and horizon
                                         (cost model), 64 = one wavefront per agent always, 8 / 16 / 32 = that group size
                                         wherever it is eligible (tests, A/B) */
       EEA_OPT_RESIDENT_CONTROL = 6,  /* eea_control (one robot, one control() per tick): 1 = a RESIDENT workgroup serves the calls
                                         from a host-mapped mailbox instead of one launch per call (the launch round trip is
                                         18-22 us whatever the shape).  It leaves by itself after EEA_OPT_RESIDENT_IDLE_MS
                                         without a call, on eea_resident_stop and on eea_destroy; while it is there,
                                         device-wide waits (hipDeviceSynchronize, hipFree) of the process take up to that
                                         long.  0 (default) = one launch per call */
       EEA_OPT_RESIDENT_IDLE_MS = 7,  /* how long the resident workgroup waits for the next call before it leaves, in
                                         milliseconds: 1 .. 60000, default 250 (a 10 Hz loop, exploration.hpp:232, keeps it
                                         alive).  Read when a resident workgroup is started */
       EEA_OPT_COUNT = 8 };
eea_status eea_set_option(int option, int value);
int eea_get_option(int option);

unsigned eea_steps(const eea_engine* e);      /* T = steps_ (ergodic_control.hpp:199) */
/* Lanes of a wavefront one agent of a plain eea_control_batch call of B agents occupies under the current options: 64 = one
 * wavefront per agent, 8 / 16 / 32 = several agents per wavefront (short horizons), 0 = the workgroup-per-agent kernel.
 * No reference counterpart (introspection for tests and capacity planning). */
unsigned eea_batch_agent_lanes(const eea_engine* e, unsigned B);
unsigned eea_num_modes(const eea_engine* e);  /* K^2 */
size_t eea_real_size(const eea_engine* e);    /* 8 or 4 */
double eea_time_step(const eea_engine* e);    /* ErgodicControl::timeStep, :350-354 */

/* ---- target distribution ----------------------------------------------------------- */
/* ErgodicControl::setTarget with a Target built from Gaussians (ergodic_control.hpp:356-360,
 * target.hpp:68-70): mu, sigma = 2 doubles per Gaussian, map frame.  As in the reference,
 * phi_k is NOT recomputed until the map extent changes. */
eea_status eea_set_target_gaussians(eea_engine* e, unsigned n, const double* mu, const double* sigma);

/* Basis::spatialCoeff on an explicit target grid (basis.hpp:99, basis.cpp:122-133):
 * phi_vals holds nx*ny reals, x fastest, on the grid configTarget builds for a domain
 * lx x ly (coordinates j*resolution by accumulation).  Sets lx, ly and phi_k directly
 * (no normalisation, as spatialCoeff).  phi_vals is a device pointer if on_device != 0. */
eea_status eea_set_target_grid(eea_engine* e, unsigned nx, unsigned ny, const void* phi_vals,
                               int on_device, double lx, double ly, void* stream);

/* Grid-tiled form of the same (multi-GPU target grids, BASELINE config 5): this rank holds rows
 * [row0, row0 + nrows) of an nx x ny_total grid in d_phi_rows (device, x fastest) and gets its
 * K^2 partial sums in d_phik_partial (device, real).  The caller adds the partials of all ranks
 * (one all-reduce of K^2 reals over RCCL) and installs the result with eea_set_phik. */
eea_status eea_spatial_coeff_rows(eea_engine* e, unsigned nx, unsigned ny_total, unsigned row0,
                                  unsigned nrows, const void* d_phi_rows, double lx, double ly,
                                  void* d_phik_partial, void* stream);
/* Target from an occupancy grid (BASELINE config 5: the in-tree surrogate of the mutual-information
 * map): phi(cell) = entropy(cell / 100.0) (numerics.hpp:164-179 with GridMap::getCell, grid.cpp:176-184),
 * normalised to sum 1 (the idiom of Target::fill, target.cpp:87), then Basis::spatialCoeff
 * (basis.cpp:122-133).  occ is the nav_msgs::OccupancyGrid::data buffer as GridMap holds it
 * (grid.cpp:63-94): int8, row-major, x fastest, nx*ny cells on the grid configTarget builds for a
 * domain lx x ly.  The entropy is applied inside the streaming kernel (one byte per cell read from
 * HBM, no fp64 target grid is materialised) and the normaliser is the (0,0) coefficient of the
 * un-normalised sums.  Sets lx, ly and phi_k.  occ is a device pointer if on_device != 0. */
eea_status eea_set_target_occupancy(eea_engine* e, unsigned nx, unsigned ny, const int8_t* occ,
                                    int on_device, double lx, double ly, void* stream);
/* Grid-tiled form (rows tiled across GPUs): this rank holds rows [row0, row0 + nrows) in d_occ_rows
 * (device) and gets its K^2 UN-normalised partial sums in d_sums_partial (device, real).  The caller
 * adds the partials of all ranks (one all-reduce of K^2 reals), divides by element 0 (the sum of the
 * entropies) and installs the result with eea_set_phik. */
eea_status eea_spatial_coeff_occupancy_rows(eea_engine* e, unsigned nx, unsigned ny_total, unsigned row0,
                                            unsigned nrows, const int8_t* d_occ_rows, double lx, double ly,
                                            void* d_sums_partial, void* stream);
/* installs phi_k (K^2 reals, device pointer if on_device != 0) for a domain lx x ly */
eea_status eea_set_phik(eea_engine* e, const void* phik, int on_device, double lx, double ly);
/* the last step of a grid-tiled occupancy target without a host round trip: phi_k = d_sums / d_sums[0], where d_sums
 * (device, K^2 reals) holds the un-normalised sums of eea_spatial_coeff_occupancy_rows after the all-reduce over the
 * ranks (element 0, mode (0,0), is the sum of the cell entropies: the normaliser of target.cpp:87).  Asynchronous
 * on `stream`; control calls enqueued on the same stream afterwards use the new phi_k. */
eea_status eea_set_phik_from_sums(eea_engine* e, const void* d_sums, double lx, double ly, void* stream);

/* ErgodicControl::configTarget (ergodic_control.hpp:362-416): refreshes map_pos; rebuilds
 * phi_k (Target::fill target.cpp:78-89 + Basis::spatialCoeff) only when the extent changed
 * by >= 1e-12.  *rebuilt (optional) reports whether the rebuild ran. */
eea_status eea_config_domain(eea_engine* e, double xmin, double xmax, double ymin, double ymax,
                             int* rebuilt, void* stream);
/* The same without the host wait: a rebuild (two or three launches) is only ENQUEUED on `stream` and the call returns;
 * control calls on the same stream afterwards are ordered by the stream, control calls on other streams are made to
 * wait for it by the engine (one hipStreamWaitEvent while it is in flight), the host-side getters wait for it.  The
 * caller orders the rebuild behind control calls still in flight on OTHER streams (they read the phi_k it replaces).
 * eea_control (single agent) uses this form internally. */
eea_status eea_config_domain_async(eea_engine* e, double xmin, double xmax, double ymin, double ymax,
                                   int* rebuilt, void* stream);

/* phi_k / lambda_k (basis.cpp:69-75) as doubles on the host, K^2 entries, col = k2*K + k1 */
eea_status eea_get_phik(eea_engine* e, double* h_phik);
eea_status eea_get_lamdak(eea_engine* e, double* h_lamdak);
/* normalised target grid of the last rebuild (Target::fill output) : nx*ny doubles; sizes via
 * eea_target_grid_size */
eea_status eea_target_grid_size(const eea_engine* e, unsigned* nx, unsigned* ny);
eea_status eea_get_target_grid(eea_engine* e, double* h_phi_vals);

/* ---- the hot path: agent-batched ErgodicControl::control --------------------------- */
/* Buffers of one batched call; B agents, each an independent reference ErgodicControl.
 * All pointers are device pointers to `real`; optional ones may be NULL. */
typedef struct {
  const void* d_pose;     /* [B][3]     current state x (map frame)                     */
  void* d_ut;             /* [B][T][3]  in: previous controls (warm start); out: updated
                                        controls.  The shift-left-by-one of :233-234
                                        happens inside the call                        */
  const void* d_mem_cols; /* [B][mem_stride][3] optional: the columns
                                        ReplayBuffer::sampleMemory would prepend
                                        (buffer.cpp:64-111), map frame                 */
  const int* d_n_mem;     /* [B] optional: valid columns per agent (<= mem_stride)     */
  unsigned mem_stride;    /* columns reserved per agent in d_mem_cols                  */
  void* d_u0;             /* [B][3]     out: ut.col(0) after the update (:310)         */
  void* d_traj;           /* [B][T][3]  out, optional: rk4_.solve rollout (:237)       */
  void* d_ck;             /* [B][K^2]   out, optional: trajectory coefficients (:267)  */
  void* d_edx;            /* [B][T][3]  out, optional: gradErgodicMetric (:270)        */
  void* d_bdx;            /* [B][T][3]  out, optional: gradBarrier (:273)              */
  void* d_rhot;           /* [B][T][3]  out, optional: co-state (:277)                 */
  int* d_status;          /* [B]        out, optional: per-agent eea_status            */
  const void* d_ck_shared;/* [K^2]      in, optional (ABI 2): decentralised-consensus mode.
                                        When set, fourier_diff = lamdak % (ck - phik)
                                        (:422) is formed with this shared c_k (e.g. the mean
                                        of all agents' c_k) instead of the agent's own; d_ck
                                        still receives the own c_k.  No counterpart in the
                                        single-agent reference: the semantics are those of its
                                        README ref. [2] (README.md:225-227).  NULL = reference
                                        behaviour.  With ck_shared_parts > 0 the buffer holds
                                        sum records instead (below)                           */
  void* d_ck_rec;         /* [B][eea_ck_record_len] out, optional (ABI 3): per-agent sum records
                                        [c_k (K^2 reals), 1, zero padding to an even length]; an
                                        agent rejected with EEA_ERR_INVALID_TWIST gets an all-zero
                                        record.  eea_ck_records_sum adds the B records in ONE small
                                        launch (fixed order); the result -- sums and agent count --
                                        is what d_ck_shared takes with ck_shared_parts > 0.  An agent
                                        left out by d_skip writes NO record (below): the buffer keeps
                                        what it held                                              */
  unsigned ck_shared_parts;/* ABI 3: 0 = d_ck_shared holds K^2 consensus values (ABI 2 form).
                                        n >= 1 = d_ck_shared holds n consecutive sum records
                                        (eea_ck_records_sum of earlier calls -- e.g. one per agent
                                        group -- all-reduced over the ranks or not): the kernel uses
                                        c_bar[m] = (sum_i rec_i[m]) x (1 / sum_i rec_i[K^2]) -- the
                                        reciprocal formed once per wavefront (ABI 6; a quotient per
                                        mode before: <= 1 ulp apart) --: no divide launch, and the
                                        exchange is one all-reduce of n records */
  /* ABI 4 -- device-bound exchange: producers and consumers of the shared c_k meet on the DEVICE, no host wait and no
   * stream wait anywhere (eea_comm_records_exchange_bound).  All optional (NULL / 0 = the forms above). */
  unsigned* d_rec_ready;  /* [B] out (with d_ck_rec): rec_ready[b] = rec_seq once agent b's record is visible
                                        device-wide -- written behind the drained, write-through record, about half
                                        way through the agent's wavefront; eea_ck_records_sum_bound polls these marks
                                        instead of waiting for the kernel to finish.  A record whose agents are ALL
                                        left out by d_skip gets no mark: the device-bound sum polls for it until its
                                        bound (about a second) runs out, then adds whatever the record holds and makes
                                        the agent count of the sum negative (consumers keep their own c_k and report
                                        EEA_ERR_TIMEOUT) -- with a skip set that can leave a record without agents, use
                                        the stream-ordered sum (eea_ck_records_sum, eea_comm_records_exchange_async,
                                        eea_consensus_plan) or set the marks of those records to rec_seq yourself */
  unsigned rec_seq;       /* sequence number of this pass (any value that grows from pass to pass, mod 2^32)     */
  const unsigned* d_ck_flag;/* in (with d_ck_shared): the kernel waits until *d_ck_flag has reached ck_flag_seq
                                        ((int)(*d_ck_flag - ck_flag_seq) >= 0) right before the first use of the shared
                                        c_k, and reads d_ck_shared past its L1: "late binding" -- the call can be
                                        launched before the exchange that fills d_ck_shared has run.  Bounded (about a
                                        second): then d_status[b] = EEA_ERR_TIMEOUT and the agent uses its own
                                        c_k.  The waiting wavefronts hold their execution slots: see
                                        eea_comm_records_exchange_bound for what must fit beside them             */
  unsigned ck_flag_seq;
  const int* d_skip;      /* [B] in, optional (ABI 5): agents with a non-zero entry are LEFT OUT of the call -- nothing of
                                        theirs is read or written, their warm start does not advance (a robot that
                                        follows a dynamic-window twist does not call control(), exploration.hpp:230-236;
                                        eea_tick_batch fills it).  That includes its record in d_ck_rec and its mark in
                                        d_rec_ready (with rec_per_wavefront: those of a wavefront whose agents are all
                                        left out): they keep what they held.  A caller who REUSES a record buffer across
                                        passes while the skip set changes must clear it before each pass, or an agent
                                        that is skipped now counts again with its old c_k (eea_consensus_plan clears
                                        its own slots)                                                           */
  int rec_per_wavefront;  /* ABI 6, with d_ck_rec: non-zero = where several agents share a wavefront (short horizons,
                                        eea_batch_agent_lanes < 64) the launch writes ONE record per wavefront -- [sum of
                                        the c_k of its accepted agents, their number, pad], the agents added in agent
                                        order -- instead of one per agent: d_ck_rec [eea_batch_record_count][record_len],
                                        d_rec_ready one mark per record.  Records are closed under addition, so
                                        eea_ck_records_sum / _bound / eea_comm_records_exchange_* take them as they are,
                                        with the record count in place of B: 4 - 8 x fewer bytes through the sum at the
                                        batch sizes that fill the chip with packed agents (27 MB per pass at 32 768
                                        agents otherwise: the sum, not the control kernel, then sets the pass time).
                                        Launches of one agent per wavefront or workgroup write per-agent records either
                                        way (count = B).  The sum of the records equals the per-agent sum up to the
                                        order of the additions (fixed, so still reproducible run to run)            */
} eea_batch_io;

/* how many records a launch of B agents writes to d_ck_rec (and marks in d_rec_ready) with rec_per_wavefront set: the number
 * of its wavefronts where agents share one (ceil(B / (64 / eea_batch_agent_lanes))), B otherwise.  0 for a null engine. */
unsigned eea_batch_record_count(const eea_engine* e, unsigned B);

/* length in reals of one sum record (eea_batch_io::d_ck_rec): K^2 + 1 rounded up to an even number */
unsigned eea_ck_record_len(const eea_engine* e);
/* d_sum [eea_ck_record_len] = sum of the B per-agent records d_ck_rec [B][eea_ck_record_len] (element K^2 = number
 * of agents that count): ONE launch of single-wavefront workgroups -- groups of 32 agents in agent order, 8 group
 * records per level-1 record, the level-1 records in order, finished by last-arrival tickets inside the launch -- a
 * fixed summation tree, run-to-run deterministic.  Asynchronous on `stream` (typically an exchange stream beside the
 * compute streams: the wavefronts use no LDS and <= 32 registers and are resident BESIDE a full fp64 K <= 10 control
 * kernel).  Concurrent calls on one engine must use distinct d_sum buffers. */
eea_status eea_ck_records_sum(eea_engine* e, unsigned B, const void* d_ck_rec, void* d_sum, void* stream);
/* ABI 6: the same sum with a CALLER-OWNED workspace -- d_ws (eea_ck_records_sum_ws_bytes: *ws_bytes) and d_tickets (*ticket_bytes,
 * zeroed once; the tickets reset themselves) -- instead of the engine's per-d_sum workspace cache: nothing is allocated or
 * looked up in the call, so it can be captured into a hipGraph and replayed for as long as the caller keeps the buffers
 * (eea_consensus_plan below does).  Same summation tree, same bits. */
eea_status eea_ck_records_sum_ws_bytes(const eea_engine* e, unsigned B, size_t* ws_bytes, size_t* ticket_bytes);
eea_status eea_ck_records_sum_ws(eea_engine* e, unsigned B, const void* d_ck_rec, void* d_sum, void* d_ws, void* d_tickets,
                                 void* stream);
/* ABI 4, device-bound form: the same sum, but the launch does not have to be ordered behind the control kernels that
 * write the records -- every unit of the sum polls the ready marks of its 32 agents (d_rec_ready[b] - seq >= 0 mod 2^32,
 * eea_batch_io::d_rec_ready / rec_seq of the producing calls) and starts when they are there.  d_flag != NULL: *d_flag = seq
 * is published (write-through, behind the drained sum record) by the wavefront that completes the sum -- what
 * eea_batch_io::d_ck_flag of the consuming calls waits for.  Agents that never report within about a second make the
 * record's agent count negative (consumers then keep their own c_k and report EEA_ERR_TIMEOUT).  Same summation tree, same
 * bits as eea_ck_records_sum. */
eea_status eea_ck_records_sum_bound(eea_engine* e, unsigned B, const void* d_ck_rec, const unsigned* d_rec_ready, unsigned seq,
                                    void* d_sum, unsigned* d_flag, void* stream);
/* d_pub [eea_ck_record_len] = d_src written through, then *d_flag = seq: publishes a record that another kernel produced with
 * ordinary stores (e.g. an all-reduce over the ranks) to control kernels that are already running and wait for the flag. */
eea_status eea_publish_record(eea_engine* e, const void* d_src, void* d_pub, unsigned* d_flag, unsigned seq, void* stream);

/* One receding-horizon optimisation per agent (ergodic_control.hpp:224-311, without the
 * configTarget call: use eea_config_domain first).  Asynchronous on `stream`. */
eea_status eea_control_batch(eea_engine* e, unsigned B, const eea_batch_io* io, void* stream);

/* ABI 4: n_steps CONSECUTIVE receding-horizon optimisations per agent in ONE launch -- what n_steps calls of
 * eea_control_batch do when each call's pose comes from a row of d_pose: step n runs control() (ergodic_control.hpp:224-311)
 * from pose row n * pose_step_stride + b and the controls step n - 1 left in d_ut (the warm start of :233-234), and
 * writes u = ut.col(0) to d_u0 row n * u0_step_stride + b.  Strides are in agents: 0 = the same row every step (a fixed
 * pose; only the last step's u0 is kept), >= B = d_pose [n_steps][stride][3] / d_u0 [n_steps][stride][3] -- a logged
 * pose sequence replayed through the controller (the replay harness of exploration.hpp:197-292 per agent), a
 * closed-loop simulation driven from the host in chunks, or a throughput run.  Bitwise the same d_ut / d_u0 as the n_steps
 * separate calls (tests/test_gpu_multi_step.py).  The other per-step outputs (d_ck, d_ck_rec, d_traj, stage outputs,
 * d_status) hold the LAST step's values; d_ck_shared / replay-memory columns are read unchanged by every step; the
 * device-bound exchange fields (d_rec_ready / d_ck_flag) are refused with n_steps > 1 (EEA_ERR_UNSUPPORTED): a step would
 * wait inside the kernel for an exchange the host can only enqueue after this call, which needs truly concurrent
 * hardware queues -- every wait of that protocol is for work enqueued BEFORE the waiter.  The
 * agent's wavefront carries on with its own stored controls (read back through L2) instead of the host launching again:
 * no launch gap, no kernel tail, no cold loads between steps.  Horizons / bases outside the wavefront-per-agent kernel's
 * range (T > 256, K > 16 and != 20) are issued as n_steps launches on the stream with the same semantics. */
eea_status eea_control_batch_steps(eea_engine* e, unsigned B, const eea_batch_io* io, unsigned n_steps,
                                   unsigned pose_step_stride, unsigned u0_step_stride, void* stream);

/* Forward rollout only: ErgodicControl::optTraj / path (ergodic_control.hpp:313-342),
 * RungeKutta::solve (integrator.hpp:135-152).  d_ut is used as is (no shift). */
eea_status eea_rollout_batch(eea_engine* e, unsigned B, const void* d_pose, const void* d_ut,
                             void* d_traj, int* d_status, void* stream);

/* ---- multi-GPU exchange steps of the agent batch (RCCL over xGMI) -------------------- */
/* The reference is single-agent; an agent batch sharded over the GPUs of a node (one process
 * per GPU, contiguous agent blocks, no collective inside the control computation) exchanges the
 * per-agent trajectory coefficients c_k the way decentralised ergodic control shares them
 * (reference README ref. [2], README.md:225-227).  These calls are what a C++ host uses to shard
 * without Python; RCCL is bound at run time (no link dependency).  All asynchronous on `stream`.
 *
 * Rank 0 obtains an id (EEA_COMM_ID_BYTES bytes) and hands it to the other ranks by any means
 * (file, socket, MPI, torch.distributed); every rank then creates its communicator.
 * id == NULL with nranks == 1 gives a local communicator without RCCL. */
#define EEA_COMM_ID_BYTES 128
typedef struct eea_comm eea_comm;
/* Binds the collectives to the RCCL at `path` (dlopen, own symbol scope) instead of the one already mapped into the process
 * or the default librccl.so -- for deployments that carry several RCCL builds; the one-GPU tests and bench.py point it at the
 * test double tests/fake_rccl/librccl.so.1 to run several ranks (processes) on one device.  Process-wide, before the first
 * other eea_comm_* call (EEA_ERR_UNSUPPORTED once the library is bound). */
eea_status eea_comm_set_library(const char* path);
eea_status eea_comm_get_unique_id(void* id);
eea_status eea_comm_create(int device, int nranks, int rank, const void* id, eea_comm** out);
void eea_comm_destroy(eea_comm* c);
int eea_comm_rank(const eea_comm* c);
int eea_comm_nranks(const eea_comm* c);
/* ABI 6: the number of ranks THE COLLECTIVE LIBRARY reports for this communicator (ncclCommCount) -- what a multi-GPU run shows to
 * prove that RCCL saw every rank; 0 for a local communicator (no library behind it), -1 if the library cannot tell. */
int eea_comm_library_nranks(const eea_comm* c);
/* sums[m] = sum over the B local agents of d_ck[b][m], m < K^2, and sums[K^2] = B (K^2 + 1 reals,
 * device): the local half of the consensus reduction */
eea_status eea_ck_sum(eea_engine* e, unsigned B, const void* d_ck, void* d_sums, void* stream);
/* one in-place-capable ncclAllGather: d_ck_all [nranks * B_local][K^2] in rank order (equal shards) */
eea_status eea_comm_allgather_ck(eea_engine* e, eea_comm* c, unsigned B_local, const void* d_ck_local,
                                 void* d_ck_all, void* stream);
/* consensus c_k: d_ck_shared[m] = mean over ALL agents of all ranks of c_k[m] -- eea_ck_sum, one
 * ncclAllReduce(sum) of K^2 + 1 reals (808 B at K = 10), one divide; feed it to
 * eea_batch_io::d_ck_shared */
eea_status eea_comm_consensus_ck(eea_engine* e, eea_comm* c, unsigned B_local, const void* d_ck_local,
                                 void* d_ck_shared, void* stream);
/* Asynchronous forms: the exchange runs on a stream the communicator owns, ordered after everything enqueued on
 * `compute_stream` so far (the pass that produced c_k), so that the next pass on the compute stream overlaps it;
 * eea_comm_wait makes a stream wait for the exchange started in `slot` (0 .. EEA_COMM_SLOTS - 1; the caller
 * rotates slots together with its c_k / result buffers). */
#define EEA_COMM_SLOTS 8
eea_status eea_comm_consensus_ck_async(eea_engine* e, eea_comm* c, unsigned B_local, const void* d_ck_local,
                                       void* d_ck_shared, void* compute_stream, int slot);
eea_status eea_comm_allgather_ck_async(eea_engine* e, eea_comm* c, unsigned B_local, const void* d_ck_local,
                                       void* d_ck_all, void* compute_stream, int slot);
eea_status eea_comm_wait(eea_comm* c, int slot, void* stream);
/* The whole exchange of one pass of an agent batch stepped as n_streams agent groups, in one call, STREAM-ORDERED: the
 * communicator's own (highest-priority) stream waits for everything enqueued so far on EACH of the group streams (one event
 * per group), then eea_ck_records_sum over the B_local per-agent records d_ck_rec (eea_batch_io::d_ck_rec of the groups'
 * control calls), then the all-reduce of the sum record over the ranks (none with one rank).  d_sum [eea_ck_record_len] then
 * feeds eea_batch_io::d_ck_shared with ck_shared_parts = 1 on every rank; the consuming streams call eea_comm_wait(c, slot, ..).
 * The form for hosts that exchange at their control rate (the reference's nodes: 10 Hz). */
eea_status eea_comm_records_exchange_async(eea_engine* e, eea_comm* c, unsigned B_local, const void* d_ck_rec,
                                           void* d_sum, void* const* group_streams, unsigned n_streams, int slot);
/* ABI 4 -- the same exchange DEVICE-BOUND, for a consensus on EVERY pass at the device's own rate (a pass of 4096 agents
 * takes ~23 us: no host wait and no stream wait fits into it).  Nothing is ordered by the host: on the communicator's
 * stream, eea_ck_records_sum_bound (polls the agents' ready marks until d_rec_ready - seq >= 0 (mod 2^32): it runs while
 * the producing control kernels are still in their backward halves), with an RCCL communicator the all-reduce of the sum record over the ranks +
 * eea_publish_record, and *d_flag = seq behind the finished d_sum.  The consuming control calls are launched WITHOUT
 * waiting, with eea_batch_io::d_ck_shared = d_sum, ck_shared_parts = 1, d_ck_flag = d_flag, ck_flag_seq = seq: they wait
 * inside the kernel, right before the first use of the shared c_k.  A consensus of lag n passes = pass i consumes seq i - n;
 * lag 1 is the previous step's c_bar (decentralised ergodic control, reference README ref. [2]).
 * The caller rotates d_ck_rec / d_sum over >= lag + 2 buffers (slot = buffer index, < EEA_COMM_SLOTS); d_rec_ready [B_local]
 * and d_flag [1] may be shared by all of them (sequence numbers only grow; zero them once, and start the sequence at 1:
 * zeroed marks and flags satisfy seq 0 at once).  A per-agent EEA_ERR_TIMEOUT in a d_status buffer that is reused from pass
 * to pass STAYS until the caller clears it (calls with d_ck_flag do not reset a status of 6; every other call rewrites
 * d_status).  Every launch that waits for a flag must leave room for what it waits for: the producers of that flag (control kernels of other agent groups, the
 * record sum's single-wavefront workgroups, the all-reduce) have to become resident BESIDE the waiting wavefronts -- two
 * agent groups per GPU of at most half its execution slots each do (the fp64 K <= 10 instance leaves registers for the
 * sum beside a full set of control wavefronts); a waiter that cannot be served gives up after about a second
 * (EEA_ERR_TIMEOUT in d_status, own c_k), it never hangs.  Host threads: none; the calling thread issues 1-3 launches.
 * With an RCCL COMMUNICATOR in the exchange the producers include the collective kernel (hundreds of threads, ~100 registers,
 * LDS of its own): it does not fit beside a full set of control wavefronts.  Every agent group waiting on the device for its
 * flag is then a dead-lock at full occupancy (every agent times out: measured in round 5 with a kernel-shaped test double,
 * profiles/r05_two_ranks.txt), and ONE waiting group (the other ordered behind the exchange with eea_comm_wait -- the event is
 * recorded behind the published record) still stalled once in a few thousand passes.  With a communicator use the
 * STREAM-ORDERED exchange -- eea_comm_records_exchange_async + eea_comm_wait for every consuming group -- at a lag of >= 2
 * passes: nothing waits inside a kernel, so nothing can hold the slots its producer needs.  The device-bound form is for
 * exchanges WITHOUT a collective kernel (one rank / a local communicator). */
eea_status eea_comm_records_exchange_bound(eea_engine* e, eea_comm* c, unsigned B_local, const void* d_ck_rec,
                                           const unsigned* d_rec_ready, unsigned seq, void* d_sum, unsigned* d_flag, int slot);
/* ---- ABI 6: the GATED exchange -- the device-bound exchange with the flag wait in front of the launch, not inside it -------
 * eea_stream_wait_flag enqueues a one-wavefront kernel on `stream` that returns once *d_flag - seq >= 0 (mod 2^32); what is
 * enqueued behind it on that stream starts after it.  A consensus pass of an agent group is then
 *     eea_stream_wait_flag(d_flag, seq - lag, .., group stream)           the sum record of pass i - lag is published
 *     eea_control_batch(.. d_ck_rec, d_rec_ready, rec_seq = seq, d_ck_shared = that record, ck_shared_parts = 1; NO d_ck_flag ..)
 * and once per pass eea_comm_records_exchange_bound(.., seq, d_sum, d_flag, slot).  Launches only: no event, no stream wait,
 * no host wait (an event record + wait pair costs the host 4.6 us on this runtime, a small launch 0.7 - 2.6).  Unlike the
 * in-kernel wait (eea_batch_io::d_ck_flag) the waiting group holds ONE execution slot, not its half of the chip: the
 * collective kernel of an RCCL communicator always finds room, so this form is safe WITH a communicator at a lag >= 2 (every
 * wait is still for work enqueued before the waiter).  Bounded: after about a second the gate gives up, adds 1 to *d_timeouts
 * (optional) and lets the stream go on -- the consuming launches then read whatever the record's slot holds at that moment: a
 * time-out is an error to be reported (the producer never became resident), not a mode of operation.  No reference counterpart. */
/* (No engine argument: the launch goes to the calling thread's CURRENT device, which must be the stream's -- it is after any
 * eea_* call on an engine or communicator of that device.) */
eea_status eea_stream_wait_flag(const unsigned* d_flag, unsigned seq, unsigned* d_timeouts, void* stream);

/* ---- ABI 6: the consensus loop of a rank as ONE replayable device graph ----------------------------------------------------
 * The stream-ordered exchange above costs the host ~6 C-ABI calls and ~11 runtime calls per pass (two group launches, their
 * eea_comm_wait, eea_comm_records_exchange_async): 35-40 us of host time per 23 us pass (profiles/r05_exchange_modes.txt) -- the
 * host, not xGMI, limits a consensus on every pass.  A plan captures `passes_per_launch` consecutive passes of that SAME protocol
 * -- per pass and agent group one eea_control_batch (records out, the sum record of pass i - lag in: ck_shared_parts = 1), then
 * on the exchange branch the record sum and the all-reduce over the ranks (nothing without an RCCL communicator) -- into one
 * hipGraph; eea_consensus_plan_launch replays it with ONE runtime call.  Nothing waits inside a kernel (the rule of
 * eea_comm_records_exchange_bound for exchanges with a collective kernel holds by construction); lag >= 2 keeps the collective
 * off the critical path of a pass.  The plan owns the record / sum buffers (lag + 2 slots, rotating; one record per wavefront
 * where agents share one: eea_batch_io::rec_per_wavefront), the record sum's
 * workspaces, the group streams and events; the caller owns what eea_batch_io names (d_pose, d_ut, d_u0, optional d_mem_cols /
 * d_n_mem / mem_stride, d_status, d_skip per group: the exchange fields of group_io are ignored) and may rewrite the CONTENTS of
 * those buffers between launches (new poses), not the pointers.  Across launches the protocol continues: pass 0 of a launch
 * consumes the record of the last passes of the launch before (the first `lag` passes ever consume an empty record: own c_k).
 * d_skip: its contents may change between launches like any other buffer's.  A skipped agent writes no record, so a plan with
 * d_skip in any group EMPTIES a slot's records inside the graph before the pass that writes them: only the agents a pass runs
 * count in its sum record, and a pass that skips everybody leaves an empty one (count 0: its consumers use their own c_k).
 * The TARGET may change between launches as long as the domain stays: phi_k is read at replay time.  The DOMAIN -- lx, ly and
 * the map origin, which eea_config_domain and every target entry that takes (lx, ly) can change -- is captured BY VALUE: while
 * any of the four differs from its value at eea_consensus_plan_create, eea_consensus_plan_launch enqueues nothing and returns
 * EEA_ERR_UNSUPPORTED (eea_last_error: the domain changed since the plan was created, the plan must be re-created); destroy the
 * plan and create a new one, or restore the old values.
 * With several ranks every rank creates and launches its plan the same number of times (the all-reduces pair up in order).
 * A plan refers to its engine and communicator: destroy it before either.
 * EEA_ERR_UNSUPPORTED: the collective library cannot be captured -- use the per-call form.  No reference counterpart
 * (decentralised ergodic control shares c_k, README.md:225-227). */
typedef struct eea_consensus_plan eea_consensus_plan;
typedef struct eea_consensus_desc {
  unsigned n_groups;             /* 1 .. 8 agent groups (contiguous slices of the rank's batch), each on a stream of its own */
  const unsigned* group_agents;  /* [n_groups] agents per group */
  const eea_batch_io* group_io;  /* [n_groups] the groups' buffers */
  unsigned lag;                  /* pass i consumes the sum record of pass i - lag: 1 .. EEA_COMM_SLOTS - 2 */
  unsigned passes_per_launch;    /* passes one launch replays; rounded UP to a multiple of the slot count lag + 2 */
} eea_consensus_desc;
eea_status eea_consensus_plan_create(eea_engine* e, eea_comm* c, const eea_consensus_desc* d, eea_consensus_plan** out);
/* replays the plan's passes, asynchronous on `stream`; launch a plan on ONE stream (its launches must run in order) */
eea_status eea_consensus_plan_launch(eea_consensus_plan* p, void* stream);
/* passes one launch replays (after rounding), and the device address of the sum record [eea_ck_record_len] the LAST pass of a
 * launch leaves (sum over all ranks of the agents' c_k, element K^2 = agent count); either pointer may be NULL */
eea_status eea_consensus_plan_info(const eea_consensus_plan* p, unsigned* passes_per_launch, const void** d_last_sum);
void eea_consensus_plan_destroy(eea_consensus_plan* p);

/* in-place ncclAllReduce(sum) of n reals: the K^2 partial sums of a grid-tiled phi_k
 * (eea_spatial_coeff_rows / eea_spatial_coeff_occupancy_rows) */
eea_status eea_comm_allreduce_sum(eea_engine* e, eea_comm* c, void* d_buf, unsigned n, void* stream);
/* the same on the communicator's own stream, ordered after `compute_stream` like the asynchronous forms above */
eea_status eea_comm_allreduce_sum_async(eea_engine* e, eea_comm* c, void* d_buf, unsigned n, void* compute_stream,
                                        int slot);

/* ---- single agent, host pointers (what ErgodicControl<ModelT>::control binds to) ---- */
/* vec control(const GridMap& grid, const vec& x) (ergodic_control.hpp:224-311) including
 * configTarget(grid): grid bounds in, u = ut.col(0) out.  The warm-start controls live in
 * the engine.  mem_cols: 3 x n_mem doubles (map frame) or NULL.  Synchronous. */
eea_status eea_control(eea_engine* e, double xmin, double xmax, double ymin, double ymax,
                       const double x[3], const double* h_mem_cols, unsigned n_mem,
                       double u_out[3]);
/* EEA_OPT_RESIDENT_CONTROL: tells the engine's resident workgroup (if one is there) to leave and returns when it has; the
 * next eea_control starts another one.  For a caller about to make device-wide waits (hipDeviceSynchronize, hipFree,
 * hipMalloc) that would otherwise take up to the idle time.  The warm-start controls are kept (they are in device memory
 * after every request).  No reference counterpart; EEA_OK also when nothing was resident. */
eea_status eea_resident_stop(eea_engine* e);
/* mat optTraj() const (ergodic_control.hpp:313-317): 3 x T doubles */
eea_status eea_opt_traj(eea_engine* e, double* h_traj);
/* read / overwrite the engine-held warm-start controls ut_ (3 x T doubles) */
eea_status eea_get_ut(eea_engine* e, double* h_ut);
eea_status eea_set_ut(eea_engine* e, const double* h_ut);

/* ---- Basis hot loops as free functions (Basis::trajCoeff / spatialCoeff) ----------- */
/* c_k = (1/n) sum_i f_k(xt_i)  (basis.cpp:109-120).  h_xt: rows x n column-major, rows >= 2 */
eea_status eea_basis_traj_coeff(int device, double lx, double ly, unsigned num_basis,
                                const double* h_xt, unsigned rows, unsigned n, double* h_ck);
/* phi_k = sum_p f_k(grid_p) phi_vals_p  (basis.cpp:122-133) for an arbitrary point list.
 * h_phi_grid: 2 x P column-major */
eea_status eea_basis_spatial_coeff(int device, double lx, double ly, unsigned num_basis,
                                   const double* h_phi_vals, const double* h_phi_grid, unsigned P,
                                   double* h_phik);

/* RungeKutta::solve (forward, integrator.hpp:135-152) for a body-twist model without an
 * engine: x0[3], h_ut 3 x steps, h_xt out 3 x steps, steps = (unsigned)|horizon/dt|.
 * EEA_ERR_INVALID_TWIST mirrors SimpleCart's throw. */
eea_status eea_rk4_rollout(int device, int model, double dt, double horizon, const double x0[3],
                           const double* h_ut, double* h_xt);
/* Target::fill (target.cpp:78-89) on an arbitrary point list: h_phi_grid 2 x P, trans[2];
 * h_phi_vals out, normalised to sum 1. */
eea_status eea_target_fill(int device, unsigned n_gauss, const double* mu, const double* sigma,
                           const double trans[2], const double* h_phi_grid, unsigned P,
                           double* h_phi_vals);

/* ---- next rows of the scope table: collision lookups ------------------------------- */
/* Collision::collisionCheck (collision.cpp:126-141) for P poses on one occupancy grid
 * (GridMap, grid.cpp:143-184).  d_grid: int8 row-major [ysize][xsize]; d_pose: [P][3]
 * doubles; d_hit: [P] ints (1 = collision).  Bit-exact integer semantics incl. the
 * world2Grid wrap of negative coordinates. */
typedef struct {
  double xmin, ymin, resolution;
  unsigned xsize, ysize;
  double boundary_radius, search_radius, obstacle_threshold, occupied_threshold;
} eea_collision_cfg;
eea_status eea_collision_check_batch(int device, const eea_collision_cfg* cfg, const int8_t* d_grid,
                                     const double* d_pose, unsigned P, int* d_hit, void* stream);
/* validate_control (numerics.hpp:312-330): integrate_twist rollout + collisionCheck per
 * step; d_x0 [P][3], d_u [P][3] doubles; d_valid [P] ints (1 = collision free). */
eea_status eea_validate_control_batch(int device, const eea_collision_cfg* cfg, const int8_t* d_grid,
                                      const double* d_x0, const double* d_u, double dt,
                                      double horizon, unsigned P, int* d_valid, void* stream);

/* ABI 6: integrate_twist (numerics.hpp:273-297) for P poses: d_out [P][3] = d_x0 + Rot(theta) * (the body-frame displacement of the
 * constant twist d_u over dt); the motion update of the replay harness / a simulated fleet between ticks, on the device so that
 * the tick loop needs no host round trip.  d_out may be d_x0.  normalize_heading != 0: the heading through normalize_angle_PI
 * (numerics.hpp:77-89) as the reference's callers do (validate_control :325); 0: as integrate_twist returns it. */
eea_status eea_integrate_twist_batch(int device, const double* d_x0, const double* d_u, double dt, unsigned P, double* d_out,
                                     int normalize_heading, void* stream);

/* DynamicWindow::control (dynamic_window.cpp:92-189), both overloads, for P robots on one grid:
 * velocity window from the current twist d_vb (dynamic_window.cpp:191-235), vx x vy x vth sample
 * grid built by repeated += (first strict minimum wins), constant-twist rollouts with a collision
 * check per step (objective, :237-286).
 *   mode "vref"  (d_xt_ref == NULL): cost = |vref - u|^2,            d_vref [P][3]
 *   mode "traj"  (d_xt_ref != NULL): cost = distance to the reference trajectory
 *                                     d_xt_ref [P][n_ref][3], time step dt_ref
 * d_u_opt [P][3] out, d_found [P] out (0 = "DWA Failed! Not even 1 solution found").
 * Mode "traj" reads column round((n_ref - 1) t / (n_ref dt_ref)) of the reference at every rollout step, t = 0, dt, 2 dt, ...
 * by repeated += over the (unsigned)|horizon / dt| steps.  The reference's xt_ref.col(j) (:277) throws past the last column;
 * here the call returns EEA_ERR_INVALID_ARGUMENT before anything is launched (d_u_opt / d_found untouched) when
 * !(n_ref * dt_ref > 0) or when a step's column lies outside [0, n_ref - 1] -- e.g. dt = dt_ref = 0.1, horizon 2.0 needs
 * n_ref >= 19.  More than 8192 samples: EEA_ERR_UNSUPPORTED (the costs of one robot's samples live in 64 KiB of LDS). */
typedef struct {
  double dt, horizon, acc_dt, acc_lim_x, acc_lim_y, acc_lim_th;
  double max_vel_x, min_vel_x, max_vel_y, min_vel_y, max_rot_vel, min_rot_vel;
  unsigned vx_samples, vy_samples, vth_samples;
} eea_dwa_cfg;
eea_status eea_dwa_control_batch(int device, const eea_collision_cfg* ccfg, const eea_dwa_cfg* dcfg,
                                 const int8_t* d_grid, const double* d_x0, const double* d_vb,
                                 const double* d_vref, const double* d_xt_ref, unsigned n_ref,
                                 double dt_ref, unsigned P, double* d_u_opt, int* d_found, void* stream);

/* ---- one tick of the exploration loop for a FLEET (ABI 5) ----------------------------------------------------------
 * Exploration<ModelT>::control's loop body (exploration.hpp:220-279) for B robots on one shared occupancy grid, on the
 * device, one stream, no host round trip:
 *   1. a robot that follows a dynamic-window twist counts a step; after dwa_steps = (unsigned)|horizon / dt| of the DWA
 *      configuration it replans (:223-228);
 *   2. every robot that does not follow one: u = ErgodicControl::control(grid, pose) (:230-236) -- eea_control_batch with
 *      d_skip for the others (their warm start stays as it is, as in the reference);
 *   3. validate_control(collision, grid, pose, u, val_dt, val_horizon) (:238);
 *   4. on a predicted collision: a follower re-runs the dynamic window towards its own twist and stops following
 *      (:243-251); the others track optTraj() -- the rollout of the UPDATED controls -- and follow the result if one was
 *      found (:254-277).  u = 0 where the dynamic window finds nothing.
 * State carried between ticks, per robot, device memory owned by the caller, zero before the first tick: d_follow_dwa,
 * d_dwa_count, d_u.  addStateMemory (:209) and sampleMemory come in front of the tick: io->d_mem_cols / d_n_mem as for eea_control_batch, filled on
 * the same stream by eea_replay_append_sample (the fleet's replay memory in device memory, below) or by the caller.
 * io->d_u0, d_traj, d_skip are ignored (the tick supplies its own); everything else of io is passed to the control call.
 * fp64 engines only (poses and twists are the doubles the collision / DWA kernels take).
 * Step 4 tracks optTraj(): T = eea_steps(e) columns every cfg.dt.  A dynamic-window rollout that would read past them (the
 * rule of eea_dwa_control_batch with n_ref = T, dt_ref = cfg.dt: e.g. an engine horizon of 1.0 under a DWA horizon of 2.0) is
 * refused with EEA_ERR_INVALID_ARGUMENT before step 1: nothing is launched, the state and the outputs stay as they were. */
typedef struct {
  int* d_follow_dwa;      /* [B]       in/out: follow_dwa (:191)                                                 */
  unsigned* d_dwa_count;  /* [B]       in/out: i (:194)                                                          */
  double* d_u;            /* [B][3]    in/out: the commanded twist u (kept while a DWA twist is followed)        */
  const double* d_vb;     /* [B][3]    in: body twists from odometry (vb_, :161-174)                             */
  const int8_t* d_grid;   /* [ysize][xsize] in: the occupancy grid (grid_)                                       */
  double* d_traj;         /* [B][T][3] scratch: optTraj() of the robots that ran control()                       */
  int* d_valid;           /* [B]       scratch / out: validate_control's result (1 = collision free)            */
  int* d_skip;            /* [B]       scratch: robots that follow a DWA twist this tick                         */
  int* d_source;          /* [B]       out, optional: who produced u -- 0 control(), 1 a followed DWA twist,
                                       2 DWA tracking optTraj(), 3 DWA re-run towards the followed twist        */
  double val_dt, val_horizon;
  unsigned long long grid_epoch; /* 0: the grid's content may have changed since the last tick.  Otherwise the caller vouches
                                       that (d_grid, grid_epoch) names ONE content (bump it with every map update, ~1 Hz
                                       against the loop's 10 Hz): the inflated collision map of the last tick on this stream
                                       is reused instead of rebuilt                                                */
} eea_tick_io;
eea_status eea_tick_batch(eea_engine* e, unsigned B, const eea_batch_io* io, const eea_tick_io* tick,
                          const eea_collision_cfg* ccfg, const eea_dwa_cfg* dcfg, void* stream);

/* ---- the replay memory of a FLEET in device memory (additive to ABI 6: detect these entries by symbol) --------------------
 * ReplayBuffer (buffer.hpp / buffer.cpp) for B robots: one store of `capacity` poses and a count per robot, in device memory;
 * append and sampleMemory are kernels that fill the d_mem_cols / d_n_mem buffers eea_control_batch / eea_tick_batch take, so
 * a closed fleet loop -- eea_replay_append_sample, eea_tick_batch, eea_integrate_twist_batch on one stream -- needs no host
 * round trip between ticks.  No existing struct or entry changes and eea_abi_version() stays 6: a caller built against this
 * header that may meet an older library looks the entries up by symbol (dlsym).  The layout of the store is private
 * (eea_replay_read reads it).
 * The random stream: Armadillo's global randi stream (buffer.cpp:99) is host state and cannot be pinned; the contract is the
 * distribution -- batch_size draws with replacement, uniform on [0, n - 1].  A draw is a pure function of (seed, draw, global
 * robot id, column): Philox4x32-10 with counter (j, robot0 + b, draw_lo, draw_hi) (robot0 + b mod 2^32) and key (seed_lo,
 * seed_hi); r64 = out[0] | out[1] << 32; index = (r64 * n) >> 64 (bias <= n / 2^64).  So a run is reproducible, a robot's
 * draws do not depend on how the fleet is sharded over ranks (each shard passes the global id of its first robot), and a
 * robot that skips control() in a tick simply leaves that tick's draw unused.  `draw` is the caller's tick counter.
 * real_size: 8 or 4 -- the `real` of the engine the columns are for (d_pose, d_mem_cols and eea_replay_read use it). */
typedef struct eea_replay eea_replay;
/* ReplayBuffer::ReplayBuffer(buffer_size, batch_size) per robot.  EEA_ERR_INVALID_ARGUMENT (before any HIP call): B, capacity
 * or batch_size == 0, real_size not 8 / 4, out == NULL.  EEA_ERR_HIP with a message: the store's size overflows or cannot be
 * allocated. */
eea_status eea_replay_create(int device, unsigned B, unsigned capacity, unsigned batch_size, uint64_t seed, unsigned robot0,
                             size_t real_size, eea_replay** out);
void eea_replay_destroy(eea_replay* r);
/* ReplayBuffer::append (buffer.cpp:54-62) of d_pose [B][3] for every robot with d_mask[b] != 0 (d_mask == NULL: all).  A
 * full store drops the pose and counts the drop (the reference's "Buffer is full" branch; not a ring).  Asynchronous. */
eea_status eea_replay_append(eea_replay* r, const void* d_pose, const int* d_mask, void* stream);
/* The columns ReplayBuffer::sampleMemory (buffer.cpp:64-111) prepends, per robot with n = its count: n == 0: d_n_mem[b] = 0;
 * n <= batch_size: the n stored poses in order, d_n_mem[b] = n (:75-89); otherwise batch_size draws (:91-108, stream above),
 * d_n_mem[b] = batch_size.  d_mem_cols [B][mem_stride][3] reals, columns past d_n_mem[b] are not written; mem_stride <
 * batch_size is EEA_ERR_INVALID_ARGUMENT.  Asynchronous. */
eea_status eea_replay_sample(eea_replay* r, uint64_t draw, void* d_mem_cols, int* d_n_mem, unsigned mem_stride, void* stream);
/* The per-tick form in ONE launch: append, then sample from the memory that includes the new pose (the reference's order,
 * exploration.hpp:209 then :232).  Bitwise what eea_replay_append followed by eea_replay_sample gives. */
eea_status eea_replay_append_sample(eea_replay* r, const void* d_pose, const int* d_mask, uint64_t draw, void* d_mem_cols,
                                    int* d_n_mem, unsigned mem_stride, void* stream);
/* Synchronising readers (tests, checkpoints, logs): wait for the device, then h_count [B] = poses stored per robot and
 * *h_dropped = appends refused by full stores since creation / the last reset, all robots (either may be NULL);
 * h_cols [n][3] reals = poses first .. first + n - 1 of robot b (EEA_ERR_INVALID_ARGUMENT past the robot's count). */
eea_status eea_replay_counts(eea_replay* r, unsigned* h_count, unsigned long long* h_dropped);
eea_status eea_replay_read(eea_replay* r, unsigned b, unsigned first, unsigned n, void* h_cols);
/* empties every robot's store and zeroes the drop counter.  Asynchronous. */
eea_status eea_replay_reset(eea_replay* r, void* stream);
/* The POOLED memory (additive to ABI 6: detect by symbol): columns for every robot drawn from the stored poses of ALL B robots
 * of `r` -- the shared past of decentralised ergodic control (the reference README's ref. [2]) in the slot sampleMemory's
 * columns take; the estimator keeps the form of buffer.cpp:64-111 (all poses in order while they fit, :75-89; otherwise
 * uniform draws with replacement, :91-108).  The control kernels are handed other columns and compute what they computed.
 * The pool: the stored poses in robot-major order -- robot 0's slots 0 .. n_0 - 1, then robot 1's, ...; off[q] = sum_{p<q} n_p
 * (64-bit), N = off[B]; the counts are the ones the device holds at the call's place in the stream (behind earlier appends
 * on it).  Robot b: N_b = N - n_b with exclude_self != 0 (the pool without its own poses), N otherwise; w = min(N_b, n_cols)
 * columns.  N_b <= n_cols: column j is pool pose j (N_b == 0: nothing).  Otherwise column j is the pool pose
 * g = (r64 * N_b) >> 64 (N_b a 64-bit factor; bias <= N_b / 2^64), r64 = out[0] | out[1] << 32 of Philox4x32-10 with counter
 * (j, robot0 + b, draw_lo, draw_hi) and key (seed_lo, seed_hi ^ 0x9E3779B9): the xor keeps these draws apart from the robot's
 * own-memory draws at the same (draw, robot, column), which would otherwise sit at the same relative position of both pools.
 * With exclude_self, g >= off[b] stands for g + n_b.  The pose of g: robot q = the last one with off[q] <= g (a robot without
 * poses is never chosen), slot g - off[q].
 * accumulate == 0: the columns go to [0, w) of row b of d_mem_cols [B][mem_stride][3], d_n_mem[b] = w, columns past w are not
 * written.  accumulate != 0: base = d_n_mem[b] as the device holds it at that place in the stream (below 0 counts as 0); the
 * columns go to [base, base + w') with w' = min(w, mem_stride - base) (0 when base >= mem_stride), d_n_mem[b] = base + w'; a
 * clipped robot gets the first w' columns of its sequence.  Pooled columns behind the robot's own: eea_replay_append_sample,
 * then this call with accumulate on the same buffers and the same stream.
 * EEA_ERR_INVALID_ARGUMENT, before any launch: r, d_mem_cols or d_n_mem null; n_cols == 0; mem_stride == 0; accumulate == 0
 * and mem_stride < n_cols.  EEA_ERR_HIP: a launch failed.
 * Asynchronous on `stream`: two launches (the offsets, then the sampler; a robot's columns come from other robots' rows, so
 * the call is ordered behind an append by the stream, never fused with it); a repeated call reads nothing on the host,
 * allocates nothing and makes no synchronising call.  The offsets buffer (B + 1 64-bit words) belongs to `r` and is allocated
 * by eea_replay_create; every call rewrites it, so the calls on one eea_replay are issued on one stream or ordered by the
 * caller.  Ranks: the pool is the object's own robots -- a fleet sharded over ranks pools per rank, robot0 enters only the
 * counter; a pool across ranks is not built. */
eea_status eea_replay_pool_sample(eea_replay* r, uint64_t draw, unsigned n_cols, int exclude_self, int accumulate,
                                  void* d_mem_cols, int* d_n_mem, unsigned mem_stride, void* stream);

/* ---- coverage of a fleet's history (additive to ABI 6, after eea_replay_*: detect these entries by symbol) ------------------
 * How ergodic is what the fleet has done so far: eps = sum_k lamda_k (c_k - phi_k)^2, the metric whose gradient control()
 * descends (gradErgodicMetric, ergodic_control.hpp:419-446), with c_k over ALL stored poses.  The reference never forms it and
 * only samples its history (<= batch_size columns, buffer.cpp:64-111).  Both calls are asynchronous on `stream`, read nothing
 * on the host and make no synchronising call; eea_abi_version() stays 6.
 *
 * eea_replay_history_records: d_rec [B][eea_ck_record_len(e)] reals of the engine's `real`; row b is the SUM RECORD of robot
 * b's whole stored history in the format of eea_batch_io::d_ck_rec: for m = k2 * K + k1 < K^2
 *     rec[b][m] = sum_{i < n_b} cos(k1 (pi / lx) (x_i - map_x)) cos(k2 (pi / ly) (y_i - map_y))
 * -- Basis::trajCoeff (basis.cpp:109-120) without the 1/N and, as there, without the h_k normalisation --, rec[b][K^2] = n_b,
 * the robot's count as the device holds it, and the padding exactly 0 (a robot without poses: an all-zero record).  The poses
 * are used as stored (map frame), shifted by map_pos as control() shifts the memory columns (ergodic_control.hpp:243-244);
 * nothing is clipped to the domain.  lx, ly, map_x, map_y are the engine's current ones (eea_config_domain): a recompute
 * from the poses, since every term changes when the map grows.  Ordered behind an in-flight eea_config_domain_async rebuild
 * the way control calls on that stream are.  A robot's record is a pure function of its own poses and the domain, added in a
 * fixed order: it does not depend on B, on the robot's index or on the other robots' counts -- two calls give the same bits, a
 * shard of a fleet the bits the whole fleet gives for its robots.  Sum records are closed under addition:
 * eea_ck_records_sum over the B rows is the fleet's record (N = sum n_b at element K^2), eea_comm_allreduce_sum adds the
 * fleet records of the ranks.  fp32 engines: counts are exact up to 2^24 poses per record.
 * EEA_ERR_INVALID_ARGUMENT before any launch: a null argument, r's real_size != eea_real_size(e), different devices;
 * EEA_ERR_NO_TARGET: no domain yet. */
eea_status eea_replay_history_records(eea_engine* e, eea_replay* r, void* d_rec, void* stream);
/* The ergodic metric of n_rec sum records d_rec [n_rec][eea_ck_record_len(e)] -- history records, the fleet record, or the
 * consensus sum records of control passes (the metric of the planned horizons): c_m = rec[m] / rec[K^2], c = 0 for every m
 * where rec[K^2] <= 0; d_metric[j] = sum_m lamda_m (c_m - phi_m)^2 with the engine's current phi_k and lamda_k
 * (basis.cpp:69-75), added in a fixed order; d_ck [n_rec][K^2] (optional) receives the c_m.  One wavefront per record.
 * EEA_ERR_INVALID_ARGUMENT: e, d_rec or d_metric null, n_rec == 0; EEA_ERR_NO_TARGET: no phi_k yet. */
eea_status eea_records_metric(eea_engine* e, unsigned n_rec, const void* d_rec, void* d_metric, void* d_ck, void* stream);

/* ---- coverage fields (additive to ABI 6: detect by symbol) -----------------------------------------------------------------
 * What the metric summarises, as maps: n_rec sum records d_rec [n_rec][eea_ck_record_len(e)] -- history records, the fleet
 * record, an all-reduced record, the consensus records of control passes -- taken back from the K^2 cosine coefficients to
 * the grid configTarget builds (ergodic_control.hpp:387-408; Fourier frame, x_i and y_j by repeated += resolution from 0, the
 * sequence of eea_set_target_grid).  The reference has no counterpart beyond publishing its target (Target::markers).
 * d_field [n_rec][nrows][nx] reals of the engine's `real`, x fastest (the layout of eea_set_target_grid's phi_vals); row r of
 * record j is grid row row0 + r of a grid of nx x ny_total points, which need not be the target grid's own size; row0 = 0,
 * nrows = ny_total: the whole grid; a rank that holds a row tile asks for its rows as with eea_spatial_coeff_rows.  With
 * c_m = rec[m] / rec[K^2] (0 for every m where rec[K^2] <= 0, the rule of eea_records_metric), m = k2 K + k1:
 *     field[j][r][i] = sum_m a_m cos((k1 (pi / lx)) x_i) cos((k2 (pi / ly)) y_{row0 + r})          (basis.cpp:85's grouping)
 *   EEA_FIELD_DENSITY    a_m = w_k1 w_k2 c_m / (lx ly), w_0 = 1, w_k = 2: the band-limited visit density (w_k / l is the inverse
 *                        squared norm of cos(k pi x / l) on [0, l]); its mean over the domain is 1 / (lx ly);
 *   EEA_FIELD_DEFICIT    a_m = w_k1 w_k2 (phi_m - c_m) / (lx ly): positive where the target wants more than the record has
 *                        delivered; an all-zero record gives the band-limited target itself;
 *   EEA_FIELD_POTENTIAL  a_m = lamda_m (c_m - phi_m): the potential whose gradient, times expl_weight, is edx
 *                        (ergodic_control.hpp:418-436); unweighted, as eea_records_metric is.
 * lx, ly, phi_k, lamda_k: the engine's current ones.  Asynchronous on `stream`; ordered behind an in-flight
 * eea_config_domain_async rebuild as eea_records_metric is.  The axis tables are cached per (nx, ny_total, lx, ly) in buffers
 * of the field's own (the phi_k path's tables are never touched): a repeated call reads nothing on the host, allocates nothing
 * and makes no synchronising call; a first call, or one after a change, builds them (and waits for the device when it has to
 * grow them).  A record's field is a pure function of the record, the domain, phi_k and the grid point, the modes added in a
 * fixed order: a record alone gives the bits it gives inside a batch, a row tile the bits of the same rows of the whole grid.
 * Before any launch -- EEA_ERR_INVALID_ARGUMENT: e, d_rec or d_field null (or not aligned to the engine's real); n_rec, nx,
 * ny_total or nrows 0; row0 + nrows > ny_total; an unknown kind.  EEA_ERR_UNSUPPORTED: nx * ny_total > 2^31 (or an axis of
 * 2^26 points and more).  EEA_ERR_NO_TARGET: no phi_k yet.  Every K (1 .. 32) and both precisions. */
typedef enum { EEA_FIELD_DENSITY = 0, EEA_FIELD_DEFICIT = 1, EEA_FIELD_POTENTIAL = 2 } eea_field_kind;
eea_status eea_records_field(eea_engine* e, int kind, unsigned n_rec, const void* d_rec, unsigned nx, unsigned ny_total,
                             unsigned row0, unsigned nrows, void* d_field, void* stream);

/* ---- range sensing of a simulated fleet (additive to ABI 6: detect these entries by symbol) ----------------------------------
 * The sensor of a simulated fleet, as eea_integrate_twist_batch is its motion: every robot casts rays through a ground-truth
 * occupancy grid and the cells the rays cross become known.  The reference states the loop in words (README.md:74-76,
 * "simulating a 360 degree range finder ... after the robot has fully explored the space, the mutual information is zero") and
 * has the map's consumer -- entropy() (numerics.hpp:164-179): an unknown cell (-1) is worth 0.7, a known one 1e-3, which is the
 * target eea_set_target_occupancy builds from the known grid.  This is NOT OccupancyMapper (mapping.cpp), which fuses laser
 * scans from outside in the order they arrive: here every write to a cell stores that cell's true value, so the result does
 * not depend on the order of robots, rays or calls, is exact in integers and needs no atomics.
 * d_truth (read only) and d_known (updated in place; the caller initialises it, normally to -1) are int8 grids of cfg's
 * geometry, row-major [ysize][xsize]; cfg's radii are not read and not checked.  R = range_cells.
 *   the robot's cell (i0, j0) = GridMap::world2Grid(x, y) (grid.cpp:143-159, with the x86-64 wrap, as the collision calls); a
 *     robot whose cell fails gridBounds (grid.cpp:96-100) reveals nothing and hits nothing (the rule of mapping.cpp:81-86); the
 *     heading is not used (360 degrees);
 *   8R rays: with side, k = divmod(q, 2R), ray q aims at the offset (tx, ty) = (R, -R + k), (R - k, R), (-R, R - k),
 *     (-R + k, -R) for side 0 .. 3 -- the perimeter of the square [-R, R]^2;
 *   step s = 1 .. R of a ray sits at (dx, dy) = (d(tx, s), d(ty, s)), d(m, s) = sgn(m) ((2 s |m| + R) div 2R): the major axis
 *     moves a cell per step, the minor one is s |m| / R rounded half away from zero -- a closed form in s, no running error;
 *   a ray, for s = 1, 2, ..: it ends without a hit where dx^2 + dy^2 > R^2 or where (i0 + dy, j0 + dx) is off the grid;
 *     otherwise known[i][j] = truth[i][j], and if !(truth[i][j] / 100.0 < occupied_threshold) -- checkCell's test on getCell
 *     (collision.cpp:216-243, grid.cpp:177-184), so a truth cell of -1 lets the ray through and stays -1 -- the ray's range
 *     is s and it ends; a ray that ends without a hit has range -1;
 *   known[i0][j0] = truth[i0][j0]; the robot's own cell never blocks its rays.
 * In an obstacle-free grid the rays reach every cell of the disc dx^2 + dy^2 <= R^2 and none outside it.
 * d_pose [P][3] doubles; d_mask [P] (optional): a robot with d_mask[b] == 0 is left out -- nothing of it is read or written,
 * its row of d_ranges included; d_ranges [P][eea_sense_ray_count(R)] ints (optional): the rays' ranges, a row of -1 for a robot
 * off the grid.  Every output is a pure function of (truth, known before, poses, mask, cfg, R).
 * eea_grid_census overwrites d_counts[3] with, over the xsize * ysize cells of d_grid: the cells < 0 (unknown); the cells >= 0
 * with cell / 100.0 < occupied_threshold; the blocking cells (!(cell / 100.0 < occupied_threshold)) -- a loop's progress
 * measure without reading the grid back (integers: no summation order enters).
 * Both calls are asynchronous on `stream`, read nothing on the host, allocate nothing and make no synchronising call; P == 0
 * is EEA_OK with nothing launched.  Before any HIP call -- EEA_ERR_INVALID_ARGUMENT: cfg, d_truth, d_known, d_pose, d_grid or
 * d_counts null; d_truth == d_known; xsize or ysize 0; resolution <= 0; range_cells == 0.  EEA_ERR_UNSUPPORTED: range_cells >
 * 1024 (up to there 2 s |m| + R stays far inside 32 bits).  eea_abi_version() stays 6. */
unsigned eea_sense_ray_count(unsigned range_cells); /* 8 * range_cells */
eea_status eea_sense_reveal_batch(int device, const eea_collision_cfg* cfg, unsigned range_cells, const int8_t* d_truth,
                                  int8_t* d_known, const double* d_pose, const int* d_mask, unsigned P, int* d_ranges,
                                  void* stream);
eea_status eea_grid_census(int device, const eea_collision_cfg* cfg, const int8_t* d_grid, unsigned long long* d_counts,
                           void* stream);

/* ---- evidence grid: the fleet's NOISY scans fused into occupancy probabilities (additive to ABI 6: detect these entries by symbol)
 * eea_sense_reveal_batch copies the truth: a cell of `known` is -1 or exact.  Here the same sensor is noisy, every scan is evidence
 * in integer log-odds units, and a publication step turns the evidence into the int8 probabilities 1 .. 99 that the tick, the
 * census, the gain count and eea_sense_mi_field read.  It is NOT a port of OccupancyMapper: updateCell (mapping.cpp:341-348) rounds
 * every single update through int8 with a truncating cast, so its grid depends on the order of every beam of every robot.  This
 * grid is ORDER-FREE -- commutative integer adds, a counter-based noise stream, every output a pure function of its inputs -- and
 * claims no parity with mapping.cpp; it borrows the sensor-model constants (prob_occ_ 0.90, prob_free_ 0.35, prior 0.5,
 * mapping.cpp:66-74) and the formula logOdds2Prob (mapping.cpp:51-54).
 * The rays and step offsets d(m, s), the disc test and the grid test, blocks(v) = !(v / 100.0 < occupied_threshold), the robot's
 * cell with the off-grid rule, and the mask are exactly those of eea_sense_reveal_batch above.  cfg's radii are not read.
 * eea_evidence_cfg: w_occ / w_free (1 .. 32767): the evidence units added for a hit / subtracted for a miss; e_clip (1 .. 1024):
 * the evidence is clamped to [-e_clip, e_clip] AT PUBLICATION ONLY (the grid itself keeps counting); quantum (finite, > 0): log-odds
 * per unit; thr_miss / thr_false: probabilities thr / 2^32 -- a truly blocking cell is missed with thr_miss, a non-blocking cell
 * raises a false alarm with thr_false; (seed_lo, seed_hi): the key of the noise stream.
 * eea_evidence_table: a pure host function, no HIP call.  table has 2 e_clip + 1 bytes; entry e + e_clip =
 * clamp(floor(100.0 * sigma(e * quantum) + 0.5), 1, 99) with sigma(l) = 1.0 - 1.0 / (1.0 + exp(l)) in double: to nearest, not the
 * reference's truncation (which would leave its own 0.90 at the mercy of the last bit of exp).  The one place an exp is evaluated;
 * the device only looks these bytes up.
 * eea_sense_observe_batch: ONE noisy scan of every robot, fused into d_evid (int32 [ysize][xsize]; the caller zeroes it once).
 *   what a scan sees: for robot b let g = robot0 + b; for the grid cell (i, j) let r be word j & 3 of Philox4x32-10 (the replay
 *     memory's generator) at the counter (j >> 2, i, g, scan) under the key (seed_lo, seed_hi).  The cell APPEARS BLOCKING in this
 *     robot's scan iff blocks(truth[i][j]) ? !(r < thr_miss) : (r < thr_false).  One outcome per (robot, scan, cell), whichever
 *     ray reaches the cell; the robot's own cell never appears blocking;
 *   the rays march exactly as in the reveal with "blocks" replaced by "appears blocking".  A cell is TOUCHED if it is the robot's
 *     own cell or a ray visits it (the cell that ends a ray included).  d_ranges [P][eea_sense_ray_count(R)] (optional) receives
 *     the step of the ending cell or -1; a robot off the grid gets a row of -1, a masked-out one is not written;
 *   fusion: each robot adds +w_occ to every touched cell that appears blocking and -w_free to every other touched cell, at most
 *     once per cell per scan however many of its rays cross the cell.  Plain two's-complement int32 adds: the result is a pure
 *     function of (truth, evid before, poses, mask, cfgs, R, scan, robot0) and does not depend on the order of robots, rays,
 *     workgroups or calls -- one call over P robots equals calls over its parts with robot0 advanced.  Keeping
 *     scans * robots * max(w_occ, w_free) below 2^31 is the CALLER's business.
 *   Asynchronous on `stream`: no host read, no allocation, no synchronising call; P == 0 is EEA_OK with nothing launched.
 * eea_evidence_publish: EVERY element of d_known (int8 [ysize][xsize]) is overwritten with
 *   e == 0 ? -1 : table[clamp(e, -e_clip, e_clip) + e_clip],   e = d_evid[i][j], table = eea_evidence_table's:
 * evidence that cancels to zero is the prior again, "unknown", which eea_sense_mi_field prices with p_unknown.  d_counts [3]
 * (optional) receives what eea_grid_census gives on the published grid, in the same launch sequence.  The launch carries the
 * table's <= 2049 bytes in its arguments: asynchronous on `stream`, no host wait, no allocation.
 * Before any HIP call -- EEA_ERR_INVALID_ARGUMENT: cfg, ecfg, table, d_truth, d_evid, d_pose or d_known null; xsize or ysize 0;
 * resolution <= 0; range_cells == 0; w_occ or w_free outside 1 .. 32767; e_clip outside 1 .. 1024; quantum not finite or <= 0.
 * EEA_ERR_UNSUPPORTED: range_cells > 127 (only the LDS form is built: the scan's window of (2R + 1)^2 bytes must fit 64 KB).
 * eea_abi_version() stays 6. */
typedef struct {
  int w_occ, w_free;            /* 1 .. 32767: evidence units added for a hit, subtracted for a miss */
  int e_clip;                   /* 1 .. 1024: evidence is clamped to [-e_clip, e_clip] at publication only */
  double quantum;               /* finite, > 0: log-odds per unit */
  uint32_t thr_miss, thr_false; /* probability = thr / 2^32; a truly blocking cell is missed with thr_miss,
                                   a non-blocking cell raises a false alarm with thr_false */
  uint32_t seed_lo, seed_hi;
} eea_evidence_cfg;
eea_status eea_evidence_table(const eea_evidence_cfg* ecfg, int8_t* table);
eea_status eea_sense_observe_batch(int device, const eea_collision_cfg* cfg, const eea_evidence_cfg* ecfg, unsigned range_cells,
                                   unsigned scan, unsigned robot0, const int8_t* d_truth, int32_t* d_evid, const double* d_pose,
                                   const int* d_mask, unsigned P, int* d_ranges, void* stream);
eea_status eea_evidence_publish(int device, const eea_collision_cfg* cfg, const eea_evidence_cfg* ecfg, const int32_t* d_evid,
                                int8_t* d_known, unsigned long long* d_counts, void* stream);

/* ---- information-gain target of an exploring fleet (additive to ABI 6: detect these entries by symbol) -------------------------
 * What a scan from each cell of the KNOWN grid would reveal, as the target phi_k: the exact, integer form of the reference's
 * description (README.md:74-76: information obtained by "simulating a 360 degree range finder", "zero after the robot has fully
 * explored the space") with the sensor eea_sense_reveal_batch defines.  It is not FCMI (no noise model, no expectation over
 * measurements): a count of the unknown cells the sensor's beams would cross (the expectation over measurements, for an ideal
 * beam, is eea_sense_mi_field below).  Against the entropy() surrogate of
 * eea_set_target_occupancy: an unknown cell no ray can reach attracts nobody, the field is zero once nothing is left to see,
 * and the re-target needs no host wait.
 * eea_sense_gain_field: d_known (int8 [ysize][xsize], read only) -> d_gain (uint32 [ysize][xsize], EVERY element overwritten).
 * With R = range_cells and the rays, step offsets d(m, s), disc test, grid test and
 * blocks(cell) = !(cell / 100.0 < occupied_threshold) exactly as eea_sense_reveal_batch defines them above:
 *   a cell (i0, j0) with i0 % stride == 0 && j0 % stride == 0 is a candidate; every other cell gets 0;
 *   a candidate whose own cell blocks gets 0 (a robot cannot stand there);
 *   any other candidate gets [known[i0][j0] < 0] + sum over the 8R rays q, over the steps s ray q makes from (i0, j0) when it is
 *     cast through `known` itself, of [known[i][j] < 0]: the ray ends where it leaves the disc or the grid; it also ends on the
 *     first blocking cell, which is visited -- and counted if it is negative -- before it ends the ray; unknown cells let the
 *     ray through, as they do in the reveal.
 * The sum is PER BEAM: a cell that several rays cross counts once per ray, as beam-based mutual-information estimators count
 * (near the candidate the rays overlap about 2.5-fold); it is not the number of distinct cells a reveal would change (which,
 * for a truth that is free wherever `known` is unknown, it bounds from above and shares its zero set with).  The largest value is 8 R^2 + 1 <= 2^23 + 1: exact in fp32 too.
 * Integers only, no atomics across workgroups, a pure function of (known, cfg, R, stride).  Asynchronous on `stream`: reads
 * nothing on the host, allocates nothing and makes no synchronising call.  Before any HIP call -- EEA_ERR_INVALID_ARGUMENT: cfg,
 * d_known or d_gain null; xsize or ysize 0; resolution <= 0; range_cells == 0; stride == 0.  EEA_ERR_UNSUPPORTED: range_cells >
 * 1024.
 * eea_set_target_gain: that field -> phi_k of engine e, all on `stream`.  The value grid is nx = xsize, ny = ysize in the
 * engine's real: v[i][j] = (real)((double)gain[i][j] + floor) on the candidates whose cell does not block, 0 elsewhere -- with
 * floor > 0 the target of a fully explored map degrades to uniform over the free candidates.  phi_k is BITWISE what
 * eea_spatial_coeff_rows (whole grid: row0 = 0, nrows = ny) followed by eea_set_phik_from_sums give for v: the same launches.
 * d_gain (optional) receives the integer field.  The field and value workspaces belong to the engine: a first call, or a
 * growing one, may wait for the device to allocate; a repeated call reads nothing on the host, allocates nothing and makes no
 * synchronising call, and control calls enqueued on `stream` afterwards use the new phi_k.  The engine's bookkeeping is left as
 * eea_set_target_occupancy leaves it (the grid's nx / ny, no Target::fill grid to read back, an in-flight
 * eea_config_domain_async rebuild is waited for first).  With floor == 0 and zero total gain phi_k is non-finite (0 / 0), exactly
 * as an all-zero grid is through those two entries: a caller stops on eea_grid_census or passes a floor.
 * Before any launch -- the field call's errors (d_gain may be null), and EEA_ERR_INVALID_ARGUMENT: e null; floor negative or not
 * finite; lx or ly <= 0.  EEA_ERR_UNSUPPORTED: xsize * ysize > 2^31.  eea_abi_version() stays 6. */
eea_status eea_sense_gain_field(int device, const eea_collision_cfg* cfg, unsigned range_cells, unsigned stride,
                                const int8_t* d_known, unsigned* d_gain, void* stream);
eea_status eea_set_target_gain(eea_engine* e, const eea_collision_cfg* cfg, unsigned range_cells, unsigned stride,
                               const int8_t* d_known, double floor, double lx, double ly, unsigned* d_gain, void* stream);

/* ---- mutual-information target of an exploring fleet (additive to ABI 6: detect these entries by symbol) ------------------------
 * The information a scan from each cell of the KNOWN grid is EXPECTED to yield, as the target phi_k: the Shannon mutual
 * information between the map and an ideal (noise-free) beam, taken over every outcome of the beam -- the quantity entropy()
 * (numerics.hpp:164-179) and the reference's README.md:74-76 describe, which is zero once the map is known.  Against the count of
 * eea_sense_gain_field it reads the occupancy probabilities 1 .. 99 of a SLAM grid, and an unknown cell behind forty others is
 * worth less than one at the frontier, because a beam will hardly get that far.  It is not the FSMI paper's estimator: there is
 * no sensor-noise kernel.  OccupancyMapper stays out as well.
 * Rays, step offsets d(m, s), the disc test, the grid test, blocks(cell) = !(cell / 100.0 < occupied_threshold) and the candidate
 * lattice are exactly those of eea_sense_reveal_batch / eea_sense_gain_field above.  Per int8 cell value v, with
 * 0 < p_unknown < 1:
 *   o(v)    = p_unknown if v < 0, else (double)min(v, 100) / 100.0;
 *   h(v)    = 0.0 if o is 0 or 1, else -o log(o) - (1.0 - o) log(1.0 - o) (natural log, double, on the host: entropy()'s formula
 *             without its 1e-3 / 0.7 clamps);
 *   pass(v) = 0.0 if blocks(v), else 1.0 - o(v).  blocks looks at the cell VALUE: at a threshold >= 0 an unknown cell never
 *             blocks, whatever p_unknown is.
 * Per candidate (i0, j0) (i0 % stride == 0 && j0 % stride == 0) whose own cell does not block, all in fp64, every product and
 * sum rounded on its own, in exactly this order:
 *   total = h(own)
 *   for q = 0 .. 8R - 1:                      (ray order)
 *     reach = 1.0; beam = 0.0                 (the robot's own cell never attenuates its rays)
 *     for the steps s = 1, 2, .. ray q makes through `known` (it ends leaving the disc or the grid):
 *       beam  = beam + reach * h(v_s)
 *       reach = reach * pass(v_s)             (a blocking cell contributes, then ends the ray: reach becomes +0.0)
 *     total = total + beam
 *   mi[i0][j0] = total
 * Every other element (off the lattice, or a blocking own cell) gets +0.0; EVERY element of d_mi is overwritten.
 * This IS the mutual information: for a beam through independent cells the measurement Z is the index of the first occupied
 * cell or "none", a function of the map, so I(M; Z) = H(Z) = sum_s (prod_{l < s} (1 - o_l)) h(o_s) (the chain rule over "does
 * the beam end at cell s, given it got there"); enumerating all 2^n maps of n = 1, 3, 6 cells agrees to 2e-16 (tests/test_mi.py
 * repeats that in exact fractions).  The hard stop at blocks() cells keeps the beam consistent with the reveal's sensor and the
 * planner's notion of an obstacle.  Once reach is +0.0 every further term is +0.0 and x + 0.0 == x bitwise for x >= 0: marching
 * a dead ray on, or stopping, changes no bit.  The largest value is ln 2 (8 R^2 + 1).
 * eea_sense_mi_table: a pure host function, no HIP call: entry v + 128 of h256 / pass256 (256 doubles each) receives h(v) /
 * pass(v) for v = -128 .. 127, of cfg only occupied_threshold is read.  It is the one place a log is evaluated, and the field
 * entries use exactly these doubles (the launch carries them): the field is held to bits independently of anybody's libm.
 * EEA_ERR_INVALID_ARGUMENT: cfg, h256 or pass256 null; p_unknown not finite or outside (0, 1).
 * eea_sense_mi_field: d_known (int8 [ysize][xsize], read only) -> d_mi (double [ysize][xsize]).  A pure function of (known, cfg,
 * R, stride, p_unknown); no atomics.  Asynchronous on `stream`: reads nothing of the device on the host, allocates nothing and
 * makes no synchronising call.  Before any HIP call -- the errors of eea_sense_gain_field (d_mi in d_gain's place), then
 * EEA_ERR_INVALID_ARGUMENT: p_unknown not finite or outside (0, 1).  range_cells > 1024 is EEA_ERR_UNSUPPORTED.
 * eea_set_target_mi: that field -> phi_k of engine e, all on `stream`, as eea_set_target_gain does it for the count:
 * v[i][j] = (real)(mi[i][j] + floor) on the candidates whose cell does not block, 0 elsewhere; phi_k is BITWISE what
 * eea_spatial_coeff_rows (whole grid) followed by eea_set_phik_from_sums give for v: the same launches.  d_mi (optional) receives
 * the field.  Workspaces (shared with eea_set_target_gain), the repeated call that neither allocates nor waits, the engine's
 * bookkeeping and the refusals (e null; floor; lx, ly; xsize * ysize > 2^31) are eea_set_target_gain's; with floor == 0 and a
 * fully known map phi_k is non-finite (0 / 0), as there.  eea_abi_version() stays 6. */
eea_status eea_sense_mi_table(const eea_collision_cfg* cfg, double p_unknown, double* h256, double* pass256);
eea_status eea_sense_mi_field(int device, const eea_collision_cfg* cfg, unsigned range_cells, unsigned stride, double p_unknown,
                              const int8_t* d_known, double* d_mi, void* stream);
eea_status eea_set_target_mi(eea_engine* e, const eea_collision_cfg* cfg, unsigned range_cells, unsigned stride, double p_unknown,
                             const int8_t* d_known, double floor, double lx, double ly, double* d_mi, void* stream);

/* ---- fleet layer: the robots of a fleet as obstacles to one another (additive to ABI 6: detect these entries by symbol) --------
 * eea_tick_batch validates every twist against the occupancy grid only: the robots of a tick drive through one another.  A
 * fleet layer is built from the fleet's poses, every tick, on the device, and eea_tick_batch_fleet adds it to every collision
 * test of steps 3 and 4.  "Avoid" is the reference's own: Collision::collisionCheck (collision.cpp:126-243) on a grid in which
 * the other robots' bodies are occupied cells.  Integer arithmetic throughout.  With r_bnd, r_col, r_max the cell radii of cfg
 * (floor(boundary_radius / resolution), floor((boundary_radius + obstacle_threshold) / resolution), floor(search_radius /
 * resolution)) and S the offsets (cell - centre) at which collisionCheck's ring search r_bnd .. r_max can report a collision
 * (those within r_col):
 *   body radius    body_cells >= 0, in cells, given at creation; the natural value is r_bnd; 0 makes a robot a single cell;
 *   offset set     F = { o + d : o in S, d integer, d.d <= body_cells^2 }; S is closed under 90-degree rotations, so F = -F;
 *                  the reach is R' = r_col + body_cells;
 *   obstacles      at an update, every robot j that is active (d_mask[j] != 0, or d_mask == NULL) and whose cell lies inside
 *                  the grid bounds; its cell is GridMap::world2Grid of its pose (grid.cpp:143-159) with the x86-64 wrap, as
 *                  everywhere else; a robot's cell is an obstacle whatever occupied_threshold is;
 *   collision      a pose with centre cell c collides with robot j iff c - cell_j in F; robot b never collides with itself;
 *   verdict        (the static verdict as without a layer) OR (the pose collides with any other robot);
 *   staleness      the other robots stand still at their cells of the last update for a whole rollout: a snapshot, as the grid
 *                  itself is.
 * This equals the reference run on a grid of its own per robot -- copy the grid, set every cell within d.d <= body_cells^2 of
 * each other obstacle robot's cell to 100, then collisionCheck / validate_control / DynamicWindow::control on that grid --
 * whenever every disc lies inside the grid and occupied_threshold <= 1.0.  Near the edge the rule keeps the WHOLE body: it does
 * not clip the disc to the grid (a pose outside the grid still collides with the part of a body that the grid would cut off).
 * What follows from the reference's ring search: with body_cells < r_bnd a robot nearer than the hollow of the ring is not seen
 * (as a small obstacle under the robot's centre is not); and robots that start inside each other's F stand still -- every
 * rollout of both that has not left F by its first step, the zero twist's included, predicts a collision, so validate_control
 * fails and the dynamic window finds nothing (u = 0).
 *
 * The layer holds an int32 count per centre cell over [-R', xsize + R') x [-R', ysize + R') (row-major, row pitch xsize + 2 R':
 * count[(cy + R') * (xsize + 2 R') + cx + R'] = the obstacle robots j with (cx, cy) - cell_j in F) and a [B][2] table of the
 * robots' cells (x, y), both entries EEA_FLEET_NOT_STAMPED for a robot that is no obstacle.  Before the first update no robot
 * is one.
 * eea_fleet_layer_create: EEA_ERR_INVALID_ARGUMENT before any HIP call -- cfg or out null, B == 0, body_cells < 0, xsize or
 *   ysize 0, resolution <= 0, the configuration errors of the collision calls; EEA_ERR_UNSUPPORTED -- R' > 127, more than 2^31
 *   centres.  The row spans of F are cached per (device, radii, body_cells) and shared between layers.
 * eea_fleet_layer_update: d_pose [B][3] doubles, d_mask [B] ints or NULL.  Three stream operations -- clear, one wavefront per
 *   robot adds +1 / -1 at the ends of its spans of F (2 x spans atomic adds per robot, not |F|), a prefix sum along every row --
 *   asynchronous on `stream`: reads nothing on the host, allocates nothing, makes no synchronising call.  The calls that read
 *   the layer are issued on the same stream or ordered behind it by the caller.
 * eea_fleet_layer_reach: R' (-1 for a null layer).
 * eea_fleet_layer_read: for tests and tools; h_count [(ysize + 2 R')][(xsize + 2 R')] ints, h_cell [B][2] ints, either may be
 *   NULL.  Synchronises the device.
 * eea_fleet_collision_check_batch: eea_collision_check_batch of P poses on d_grid (the layer's geometry and radii) with the
 *   layer; d_self [P] ints or NULL: the robot a pose belongs to, -1 (or NULL) for none; d_grid == NULL: robots only.
 * eea_tick_batch_fleet: eea_tick_batch with the layer in steps 3 and 4 -- validate_control and the dynamic window see the other
 *   robots; robot r of the tick is robot r of the layer.  ccfg must give the layer's geometry, radii and threshold and B the
 *   layer's B (and the layer live on the engine's device), else EEA_ERR_INVALID_ARGUMENT: nothing is launched and the state is
 *   untouched.  Everything else as eea_tick_batch.  A closed loop: eea_fleet_layer_update, eea_tick_batch_fleet,
 *   eea_integrate_twist_batch on one stream, no host wait. */
#define EEA_FLEET_NOT_STAMPED (-2147483647 - 1)
typedef struct eea_fleet_layer eea_fleet_layer;
eea_status eea_fleet_layer_create(int device, const eea_collision_cfg* cfg, int body_cells, unsigned B, eea_fleet_layer** out);
void eea_fleet_layer_destroy(eea_fleet_layer* l);
eea_status eea_fleet_layer_update(eea_fleet_layer* l, const double* d_pose, const int* d_mask, void* stream);
int eea_fleet_layer_reach(const eea_fleet_layer* l);
eea_status eea_fleet_layer_read(const eea_fleet_layer* l, int* h_count, int* h_cell);
eea_status eea_fleet_collision_check_batch(const eea_fleet_layer* l, const int8_t* d_grid, const double* d_pose, const int* d_self,
                                           unsigned P, int* d_hit, void* stream);
eea_status eea_tick_batch_fleet(eea_engine* e, unsigned B, const eea_batch_io* io, const eea_tick_io* tick,
                                const eea_collision_cfg* ccfg, const eea_dwa_cfg* dcfg, const eea_fleet_layer* l, void* stream);

/* ---- clearance queries: Collision::minDistance / minDirection (collision.cpp:65-124) -------------------------------
 * How close a pose is to an occupied cell, and in which direction, by the reference's own search (collision.cpp:148-243):
 * the Bresenham rings r_bnd .. r_max around the pose's cell (radii in cells as for eea_collision_check_batch), four cells
 * per step; the occupied in-grid cell of the smallest squared cell distance is kept -- of equal distances the first one
 * visited (a strict <) -- and the search stops with "crash" at the first cell within r_col.  The rings have gaps; a cell in
 * a gap is not seen, as in the reference.  Per pose (eea_clearance, and the doubles the two reference functions return):
 *   crash      msg 0, sqrd_obs = dx = dy = 0;          dmin = 0.0;                     disp = (0, 0)
 *   obstacle   msg 1, sqrd_obs, (dx, dy) = cell - pose's cell;
 *              dmin = sqrt((double)sqrd_obs) * resolution - boundary_radius;           disp = (resolution * dx, resolution * dy)
 *   none       msg 2, sqrd_obs = -1, dx = dy = 0;      dmin = DBL_MAX;                 disp = (DBL_MAX, DBL_MAX)
 * bit for bit the reference's x86-64 results.  A call runs one wavefront per pose (or cell) or goes through a key map built
 * from the grid per call (EEA_OPT_COLLISION_IMPL: 0 = cost model, 1 / 2 force the one / the other).  Both calls are
 * asynchronous on `stream`; the buffers are device memory.  P == 0 is EEA_OK.
 * Before the device is selected -- EEA_ERR_INVALID_ARGUMENT: cfg, d_grid or d_pose null; every output null; xsize or ysize 0;
 * resolution <= 0; the configuration errors of the collision calls.  EEA_ERR_UNSUPPORTED: xsize * ysize > 2^31; a search
 * radius of so many cells that (largest squared distance + 1) * (cells the search visits) exceeds 2^32 - 1 (with r_bnd = 0:
 * an r_max above 196 cells).  No output is touched then.  eea_abi_version() stays 6. */
enum { EEA_COLLISION_CRASH = 0, EEA_COLLISION_OBSTACLE = 1, EEA_COLLISION_NONE = 2 }; /* CollisionMsg, collision.hpp:55-60 */
typedef struct eea_clearance {
  int msg, sqrd_obs, dx, dy;
} eea_clearance;
/* Collision::minDistance (collision.cpp:65-93) + minDirection (collision.cpp:95-124) of P poses d_pose [P][3]; d_out [P],
 * d_dmin [P] and d_disp [P][2] may each be NULL, not all three. */
eea_status eea_clearance_batch(int device, const eea_collision_cfg* cfg, const int8_t* d_grid, const double* d_pose, unsigned P,
                               eea_clearance* d_out, double* d_dmin, double* d_disp, void* stream);
/* the same for the centre of every grid cell, row-major [ysize][xsize] (collision.cpp:65-93 per cell; the displacement is
 * resolution * (dx, dy) of d_field); either output may be NULL, not both */
eea_status eea_clearance_field(int device, const eea_collision_cfg* cfg, const int8_t* d_grid, eea_clearance* d_field,
                               double* d_dmin, void* stream);

/* ---- distance field: the exact Euclidean distance transform of the occupied cells ------------------------------------
 * No reference counterpart (the reference README lists a distance field under "Future Improvements").  The ring search above
 * has gaps, sees nothing inside r_bnd and nothing beyond r_max; these calls give the exact distance, in cells, from every
 * cell to the nearest occupied in-grid cell -- not an approximation, a chamfer or a bounded search.  A cell is occupied by
 * checkCell's test, !(int8 / 100.0 < occupied_threshold); cells come from world2Grid as everywhere else (x86 wrap included).
 * They stand beside the reference-exact calls and change none of them.  All three are asynchronous on `stream`; the buffers
 * are device memory; no cache is kept between calls.  eea_abi_version() stays 6.
 * Before the device is selected, with no output touched -- EEA_ERR_INVALID_ARGUMENT: cfg or a required buffer null (each
 * call lists its own); xsize or ysize 0; resolution <= 0; the configuration errors of the collision calls.
 * EEA_ERR_UNSUPPORTED: xsize or ysize above EEA_DISTANCE_MAX_SIDE (a row of the field is held in a workgroup's LDS; squared
 * distances (xsize-1)^2 + (ysize-1)^2 and cell indices xsize * ysize stay far inside int). */
#define EEA_DISTANCE_MAX_SIDE 8192
enum { EEA_COLLISION_OFF_GRID = 3 }; /* eea_clearance.msg of the distance queries: the pose's cell fails gridBounds */
/* Build.  d_sq [ysize][xsize]: the squared cell distance from cell (i, j) to the nearest occupied cell; 0 on an occupied
 * cell; -1 everywhere when the grid has no occupied cell.  d_nearest [ysize][xsize] (may be NULL): the row-major index of
 * that cell, -1 when there is none; among occupied cells at the same squared distance the smallest index.  Integer minima
 * throughout: bit-reproducible.  Required: cfg, d_grid, d_sq. */
eea_status eea_distance_field(int device, const eea_collision_cfg* cfg, const int8_t* d_grid, int* d_sq, int* d_nearest,
                              void* stream);
/* P poses d_pose [P][3] through a built field; d_out [P], d_dmin [P], d_disp [P][2] may each be NULL, not all three;
 * d_nearest may be NULL when d_out and d_disp are.  P == 0 is EEA_OK.  Required: cfg, d_sq, d_pose.  Per pose:
 *   off the grid  msg 3 (EEA_COLLISION_OFF_GRID), sqrd_obs = -1, dx = dy = 0;  dmin = 0.0;      disp = (0, 0)
 *   empty field   msg 2 (none),                   sqrd_obs = -1, dx = dy = 0;  dmin = DBL_MAX;  disp = (DBL_MAX, DBL_MAX)
 *   sq <= r_col^2 msg 0 (crash)   }  sqrd_obs = sq, (dx, dy) = nearest cell - pose's cell,
 *   otherwise     msg 1 (obstacle)}  dmin = sqrt((double)sq) * resolution - boundary_radius (a correctly rounded root, one
 *                                    product, one difference; negative inside the bounding radius), disp = resolution * (dx, dy)
 * Unlike eea_clearance_batch a crash keeps its real values (the field knows them), and there is no r_bnd and no r_max: every
 * occupied cell counts at any distance.  Off the map is not free space: hence the message of its own and the conservative
 * constants. */
eea_status eea_distance_query_batch(int device, const eea_collision_cfg* cfg, const int* d_sq, const int* d_nearest,
                                    const double* d_pose, unsigned P, eea_clearance* d_out, double* d_dmin, double* d_disp,
                                    void* stream);
/* The worst step of each of B trajectories d_traj [B][T][3] (the layout of eea_rollout_batch's output, eea_control_batch's
 * d_traj and eea_tick_io.d_traj): the query's answer at that step (d_out [B], d_dmin [B]) and the step's index (d_step [B]);
 * each may be NULL, not all three; d_nearest may be NULL when d_out is.  An off-grid step is worse than any on-grid one,
 * among on-grid steps the smallest sq is worst, among equals the earliest step; an empty field gives none at step 0.
 * Required: cfg, d_sq, d_traj.  T == 0 (or above 2^31 - 1) is EEA_ERR_INVALID_ARGUMENT, B == 0 is EEA_OK. */
eea_status eea_distance_traj_min(int device, const eea_collision_cfg* cfg, const int* d_sq, const int* d_nearest,
                                 const double* d_traj, unsigned B, unsigned T, eea_clearance* d_out, int* d_step, double* d_dmin,
                                 void* stream);

/* ---- geodesic field: shortest paths through free space (additive to ABI 6: detect these entries by symbol) ---------------
 * No reference counterpart.  Every other distance here is straight-line; these give the cost of getting somewhere: the
 * shortest-path distance through traversable cells from a set of source cells, as a field on the grid.  Seeded from the
 * fleet's poses it is a reachability mask for the targets (eea_set_target_reachable); seeded from goal cells, descending it
 * gives a detour path in the layout the dynamic window's trajectory mode reads (eea_geodesic_path_batch).  Grid, the cell of
 * a pose (world2Grid, x86 wrap included), gridBounds and blocks(v) = !(v / 100.0 < occupied_threshold) as everywhere else.
 * Integers with a unique answer: bit-reproducible.
 *   traversable   a cell (i, j) in the grid with !blocks(grid[i][j]); with EEA_GEODESIC_UNKNOWN_BLOCKS also grid[i][j] >= 0;
 *                 with d_sq != NULL also d_sq[i][j] == -1 || d_sq[i][j] > clear_sq.  d_sq is eea_distance_field's plane of the
 *                 same grid, clear_sq >= 0 a squared cell radius (r_col^2 for the disc, ceil(r_out / res)^2 for a polygon).
 *   moves         the four axis moves cost 5, the four diagonal moves cost 7 (the 5-7 chamfer).  A move goes only INTO a
 *                 traversable cell; a diagonal move also needs both cells it passes between to be traversable (no corner
 *                 cutting).
 *   sources       the cells of d_pose [P][3] (poses failing gridBounds are skipped) and / or the row-major indices d_cells
 *                 [n_cells] (negative or out-of-range ones are skipped).  A source's own cell is seeded with 0 whenever it is in
 *                 the grid and does not block: the unknown test and the clearance test are waived for it (a robot is where it
 *                 is, and must be able to leave a tight spot).  Nothing moves into a non-traversable source cell.
 *   field         geo[i][j] (int32) = the cost of the cheapest move sequence from any source cell to (i, j); -1 where there is
 *                 none (blocking cells, non-traversable non-source cells, cells cut off from every source, every cell when no
 *                 source is accepted).  EVERY element is overwritten.
 * Limits: xsize * ysize <= 2^26 (7 * cells < 2^31) and sides of at most EEA_DISTANCE_MAX_SIDE, else EEA_ERR_UNSUPPORTED.
 * The build works on tiles of EEA_GEODESIC_TILE_X x EEA_GEODESIC_TILE_Y cells, in rounds of one launch each: a tile whose
 * neighbourhood changed in the round before is relaxed to its own fixed point, values only go down, and every value ever
 * written is the cost of a real move sequence.  Nothing waits inside a kernel.
 * eea_geodesic_ws_bytes: host only; the bytes d_ws must hold for the grid of cfg (positive, monotone in the grid's size).  d_ws
 *   is device memory aligned to 4 bytes (any allocation's start is); its contents mean nothing between calls.
 * eea_geodesic_field: d_state [4] (uint32, device) receives [0] 1 if the field is final, else 0; [1] the number of rounds that
 *   changed something; [2] the number of accepted sources (entries of the two lists, not distinct cells); [3] 0.
 *   max_rounds > 0: at most that many rounds are enqueued on `stream`; nothing of the device is read on the host, nothing is
 *     allocated and no synchronising call is made; a round that finds nothing pending exits at once.  If the budget runs out
 *     first d_state[0] = 0, every element of d_geo is -1 or the cost of a real move sequence (>= the final value), and no
 *     element that is -1 in the final field holds anything else.
 *   max_rounds == 0: the call runs to the end and WAITS on `stream` for it: it reads d_state[0] on the host after every
 *     16 rounds (as eea_set_target_occupancy, this form is not for a loop that must not wait).
 *   EEA_GEODESIC_CONTINUE: d_geo is taken as it stands -- valid when it comes from an earlier call with the same or a smaller
 *     traversable set and the same or fewer sources (this call's are the same or more) --, the sources are seeded again and every
 *     tile is pending; it ends at the same bits as a fresh call.  d_state counts this call's rounds.
 *   Before the device is selected, with no output touched -- EEA_ERR_INVALID_ARGUMENT: cfg, d_grid, d_geo, d_ws or d_state null;
 *   no source list with entries (d_pose null or P == 0, and d_cells null or n_cells == 0) without EEA_GEODESIC_CONTINUE;
 *   clear_sq < 0; unknown flag bits; d_ws not 4-byte aligned; the configuration errors of the distance calls.  EEA_ERR_UNSUPPORTED: the limits above.
 * eea_geodesic_path_batch: per pose of d_pose [P][3], from d_geo alone, d_path [P][n_steps][3] (the layout d_xt_ref of the
 *   three dynamic-window entries reads) and d_len [P] (may be NULL).  With c the pose's cell: if c is off the grid or
 *   geo[c] < 0, len = -1 and all n_steps rows hold the pose itself.  Otherwise, until geo[c] == 0 or n_steps way-points are
 *   written: among the eight moves tried in the order (di, dj) = (0,+1) (+1,0) (0,-1) (-1,0) (+1,+1) (+1,-1) (-1,-1) (-1,+1)
 *   take the first whose target n has geo[n] >= 0 and geo[n] + cost == geo[c] (for a diagonal both passed-between cells must have
 *   geo >= 0 as well); the way-point is the centre of n, x = (double)(j * res) + res / 2.0 + xmin and likewise y, with the
 *   heading of the move, atan2(di, dj) as one of eight literal doubles k pi / 4 in [-pi, pi) (0, pi/2, -pi, -pi/2, pi/4, 3pi/4,
 *   -3pi/4, -pi/4 in the order above; no atan2 runs on the device); c = n.  In a final field such a move exists for every
 *   reachable non-source cell; where a field that is not final has none the walk ends.  Rows past the end repeat the last
 *   way-point -- before any way-point: the centre of the pose's own cell with the pose's heading, so a pose on a source cell
 *   gets n_steps such rows and len 0.  len = the number of moves written, <= n_steps.  One lane per pose; asynchronous on
 *   `stream`.  P == 0 is EEA_OK.  EEA_ERR_INVALID_ARGUMENT: cfg, d_geo, d_pose or d_path null; n_steps == 0; the configuration
 *   errors above.  EEA_ERR_UNSUPPORTED: the limits above.
 * eea_set_target_reachable: phi_k of engine e from a field the caller already has, restricted to reachable cells.  kind 0:
 *   d_field is the uint32 field of eea_sense_gain_field; kind 1: the double field of eea_sense_mi_field.  The value grid is
 *   v[i][j] = (real)((double)field[i][j] + floor) on the candidates (both indices multiples of stride) whose cell of d_known does
 *   not block and has d_geo[i][j] >= 0, 0 elsewhere; phi_k is BITWISE what eea_spatial_coeff_rows (whole grid) followed by
 *   eea_set_phik_from_sums give for v: the launches of eea_set_target_gain, on `stream`, in both engine precisions.  Workspaces,
 *   the repeated call that neither allocates nor waits, the engine's bookkeeping and the refusals (e, cfg or d_known null;
 *   xsize or ysize 0; resolution <= 0; stride == 0; floor; lx, ly; xsize * ysize > 2^31) are eea_set_target_gain's, and
 *   EEA_ERR_INVALID_ARGUMENT: d_field or d_geo null, kind outside {0, 1}.  With floor > 0 and a fully explored map the target is
 *   uniform over the reachable candidates only; with nothing reachable phi_k is non-finite, as an all-zero grid is there.
 * eea_abi_version() stays 6. */
#define EEA_GEODESIC_TILE_X 32 /* the build's tile, published so that tests can size scenes from it */
#define EEA_GEODESIC_TILE_Y 32
enum { EEA_GEODESIC_UNKNOWN_BLOCKS = 1, EEA_GEODESIC_CONTINUE = 2 };
eea_status eea_geodesic_ws_bytes(const eea_collision_cfg* cfg, size_t* bytes);
eea_status eea_geodesic_field(int device, const eea_collision_cfg* cfg, const int8_t* d_grid, const int* d_sq, int clear_sq,
                              unsigned flags, const double* d_pose, unsigned P, const int* d_cells, unsigned n_cells,
                              unsigned max_rounds, int* d_geo, void* d_ws, unsigned* d_state, void* stream);
eea_status eea_geodesic_path_batch(int device, const eea_collision_cfg* cfg, const int* d_geo, const double* d_pose, unsigned P,
                                   unsigned n_steps, double* d_path, int* d_len, void* stream);
eea_status eea_set_target_reachable(eea_engine* e, const eea_collision_cfg* cfg, int kind, const void* d_field, unsigned stride,
                                    const int8_t* d_known, const int* d_geo, double floor, double lx, double ly, void* stream);

/* ---- geodesic partition: each robot's share of free space, its goal and the way there (additive to ABI 6: detect these
 * entries by symbol) -------------------------------------------------------------------------------------------------------
 * No reference counterpart.  eea_geodesic_field says how far a cell is from the nearest source; these say WHICH source that is
 * (the geodesic Voronoi partition of free space), pick per source the best cell of its own region under a score, and walk from
 * a robot to its own goal -- from one build, where one field per robot would need B.  Integers and fixed-order fp64 with a
 * unique answer: bit-reproducible.
 * eea_geodesic_partition: the grid, the traversable set, the moves, the accepted sources with their waived tests, d_state,
 *   the two forms of max_rounds, the limits and the refusals are eea_geodesic_field's.  In addition:
 *   labels        the label of a source is its index in the concatenated list: pose q has label q, cell k has label P + k.
 *                 Entries that are not accepted keep their index and own nothing.
 *   key           every cell carries the pair (cost, label) under lexicographic order: an accepted source's cell holds
 *                 (0, the smallest label accepted there), every other traversable cell the least of (neighbour's cost + move
 *                 cost, neighbour's label) over the legal moves into it.  Adding a positive cost is monotone for this order, so
 *                 the fixed point is unique: min over sources s of (d_s(cell), s).
 *   outputs       d_geo (int32 [ysize][xsize]) is BITWISE what eea_geodesic_field writes for the same arguments; d_owner (int32
 *                 [ysize][xsize]) is the smallest label among the sources at that cost, -1 exactly where d_geo is -1.  EVERY
 *                 element of both planes is overwritten.
 *   The build is eea_geodesic_field's (tiles of EEA_GEODESIC_TILE_X x EEA_GEODESIC_TILE_Y cells, rounds of one launch each,
 *   nothing waits inside a kernel) on one 64-bit word per cell, cost in the high half and label in the low half, kept in d_ws and
 *   read and written whole, so that no reader can pair a new cost with an old label; a last launch unpacks it into the planes.
 *   A budgeted call that is not final leaves, per cell, -1 / -1 or the cost and label of a real move sequence (the cost >= the
 *   final one and >= that label's single-source cost); no cell that is finally -1 holds anything else.
 *   EEA_GEODESIC_CONTINUE: the words are rebuilt from d_geo / d_owner as they stand -- valid when both come from a call with
 *   the same source lists and the same or a smaller traversable set --; the call ends at the bits of a fresh call.
 *   eea_partition_ws_bytes: host only; the bytes d_ws must hold (positive, monotone in the grid's size).  d_ws is device memory
 *   aligned to 8 bytes; its contents mean nothing between calls.
 *   EEA_ERR_INVALID_ARGUMENT besides eea_geodesic_field's: d_owner null; d_ws not 8-byte aligned.  EEA_ERR_UNSUPPORTED besides
 *   its limits: P + n_cells > 2^31 - 1.
 * eea_partition_goals: kind 0: d_field is the uint32 field of eea_sense_gain_field; kind 1: the double field of
 *   eea_sense_mi_field (finite).  Per label r < n_labels:
 *   d_area[r]        (uint32) the number of cells with owner r.
 *   candidate        a cell with owner r, both indices multiples of stride, whose cell of d_known does not block, and whose
 *                    field value is > 0.
 *   score            w_field * (double)field - w_cost * (double)geo: both products rounded on their own, then subtracted, in
 *                    fp64 with no contraction.
 *   d_goal_cell[r]   (int32) the row-major index of the candidate with the greatest score, the lowest index on a tie; -1: r has
 *                    no candidate.
 *   d_goal_score[r]  (double) that score; 0.0 when there is no candidate.
 *   Owners < 0 or >= n_labels are ignored.  Max and min are exact and commutative: the answer does not depend on the schedule.
 *   No workspace (d_goal_score's own 8 bytes hold an order-preserving integer of the score during the call); asynchronous on
 *   `stream`: nothing is allocated, waited for or read on the host.  n_labels == 0 is EEA_OK and touches nothing.
 *   Before the device is selected -- EEA_ERR_INVALID_ARGUMENT: cfg, d_field, d_known, d_geo, d_owner, d_goal_cell, d_goal_score
 *   or d_area null; kind outside {0, 1}; stride == 0; a weight that is not finite or outside [0, 1e30] (the cap keeps a score
 *   finite); the configuration errors of the geodesic calls.  EEA_ERR_UNSUPPORTED: their limits.
 * eea_partition_path_batch: eea_geodesic_path_batch walks towards the NEAREST source; here robot q (pose q of d_pose [P][3],
 *   label q) gets the path from its own cell to ITS goal g = d_goal_cell[q], in the same layout d_path [P][n_steps][3], d_len
 *   [P] (may be NULL).  If g < 0, g is off the grid, d_owner[g] != q, d_geo[g] < 0 or the pose is off the grid: len = -1 and all
 *   rows hold the pose.  Otherwise descend from g: among the eight moves in eea_geodesic_path_batch's order take the first whose
 *   target n has geo[n] + cost == geo[c] and owner[n] == owner[c] (for a diagonal both passed-between cells must have geo >= 0),
 *   until geo == 0.  The owner condition is needed: at a tie cell the cost-only rule can step into a neighbour's region and end
 *   on the wrong robot; in a final field the constrained step always exists and the walk ends on q's own cell.  (A walk that
 *   finds no step or ends elsewhere -- planes that are not final, or not of these poses -- gives len = -1 and the pose, too.)
 *   The cells reversed are c_0 (the robot's cell) .. c_m = g: row k < min(m, n_steps) holds the centre of c_{k+1} by
 *   grid2World's arithmetic with the heading of the FORWARD move c_k -> c_{k+1}, one of the same eight literals (the opposite
 *   of the descent's move index: 0 <-> 2, 1 <-> 3, 4 <-> 6, 5 <-> 7).  Rows past the end repeat the last way-point -- before
 *   any way-point: the centre of the robot's own cell with the pose's heading, so m = 0 gives len 0.  len = the number of moves
 *   written, <= n_steps.  One lane per robot (it walks once to count m, once more to write the rows); asynchronous on `stream`.
 *   P == 0 is EEA_OK.  Refusals: eea_geodesic_path_batch's, EEA_ERR_INVALID_ARGUMENT for d_owner or d_goal_cell null, and
 *   EEA_ERR_UNSUPPORTED for P > 2^31 - 1 (a label is a non-negative int).
 * eea_abi_version() stays 6. */
eea_status eea_partition_ws_bytes(const eea_collision_cfg* cfg, size_t* bytes);
eea_status eea_geodesic_partition(int device, const eea_collision_cfg* cfg, const int8_t* d_grid, const int* d_sq, int clear_sq,
                                  unsigned flags, const double* d_pose, unsigned P, const int* d_cells, unsigned n_cells,
                                  unsigned max_rounds, int* d_geo, int* d_owner, void* d_ws, unsigned* d_state, void* stream);
eea_status eea_partition_goals(int device, const eea_collision_cfg* cfg, int kind, const void* d_field, unsigned stride,
                               const int8_t* d_known, const int* d_geo, const int* d_owner, unsigned n_labels, double w_field,
                               double w_cost, int* d_goal_cell, double* d_goal_score, unsigned* d_area, void* stream);
eea_status eea_partition_path_batch(int device, const eea_collision_cfg* cfg, const int* d_geo, const int* d_owner,
                                    const double* d_pose, unsigned P, const int* d_goal_cell, unsigned n_steps, double* d_path,
                                    int* d_len, void* stream);

/* ---- frontier regions: connected frontiers, their statistics and a goal per robot (additive to ABI 6: detect these entries
 * by symbol) ---------------------------------------------------------------------------------------------------------------
 * No reference counterpart.  eea_partition_goals scores single cells: a one-cell hole in explored space scores like the edge
 * of an unexplored room, and a goal has no identity.  These group the member cells of a grid into connected regions, each
 * with a label, a rank, a size, a centroid (as two sums), a bounding box and an entry cell, and pick per robot the region to go
 * for.  Integers with a unique answer (and one fp64 score of fixed arithmetic): bit-reproducible.
 * eea_frontier_regions:
 *   members       kind EEA_FRONTIER_OF_GRID: a cell (i, j) of value v = d_grid[i][j] with v >= 0, !blocks(v) -- the literal
 *                 !(v / 100.0 < occupied_threshold) --, and at least one of its four axis neighbours INSIDE the grid of value
 *                 < 0.  Off-grid neighbours are not unknown; a cell with only a diagonal unknown neighbour is no frontier.
 *                 kind EEA_FRONTIER_OF_MASK: a cell with d_grid[i][j] != 0 (any class a caller has).
 *                 With d_geo != NULL both kinds also require d_geo[i][j] >= 0: the reachable cells of eea_geodesic_field's or
 *                 eea_geodesic_partition's plane.  d_owner (eea_geodesic_partition's) is only read with d_geo.
 *   regions       the connected components of the members under 8-connectivity (no passed-between condition).  The label of a
 *                 region is its root: the least row-major index of a member.  Regions are ranked 0 .. n - 1 by ascending root.
 *   d_root        (int32 [ysize][xsize]) the root of the cell's region, -1 for a non-member.
 *   d_region      (int32 [ysize][xsize]) the rank of the cell's region, -1 for a non-member; ranks >= max_regions are written
 *                 as they are.  EVERY element of both planes is overwritten.
 *   d_regions     [max_regions] records; record r < min(n, max_regions) is written, the others are not touched:
 *                 size, sum_i / sum_j (sums of the members' rows / columns: the centroid is sum / size), i_min .. j_max (the
 *                 bounding box), root; entry_cell = the member with the least (d_geo, row-major index), entry_cost = its
 *                 d_geo, entry_owner = d_owner[entry_cell]; each of the three is -1 without the plane it needs; reserved = 0.
 *                 entry_cost and entry_cell share one aligned 8-byte word, cost << 32 | cell, so that the entry is one 64-bit
 *                 atomic minimum.
 *   d_state       (uint32 [4], device) [0] n; [1] min(n, max_regions); [2] the number of member cells; [3] 0.
 *   max_regions == 0 is allowed (d_regions may then be NULL): only the planes and the state are written.
 *   The build is label-equivalence union-find on tiles of EEA_GEODESIC_TILE_X x EEA_GEODESIC_TILE_Y cells in a fixed number
 *   of launches, whatever the map: every tile labels its own components in LDS and stores, per member, the index of its local
 *   root into d_root; one lane per pair of member neighbours across a tile border unites their sets with a lock-free union
 *   (find both roots, hang the larger under the smaller with an atomic minimum, go on with the link that was displaced; the
 *   larger index of the pair falls in every turn, so every loop is bounded and none waits for another workgroup); then every
 *   member takes the root of its set, roots are counted per 1024 consecutive cells and ranked by one scan, and the members add
 *   into their records with integer atomics, combined per wavefront first.  Nothing waits inside a kernel; asynchronous on
 *   `stream`: nothing is allocated, waited for or read on the host.
 *   eea_frontier_ws_bytes: host only; the bytes d_ws must hold (positive, monotone in the grid's size).  d_ws is device memory
 *   aligned to 8 bytes; its contents mean nothing between calls.
 *   Before the device is selected, with no output touched -- EEA_ERR_INVALID_ARGUMENT: cfg, d_grid, d_root, d_region, d_ws or
 *   d_state null; d_regions null with max_regions > 0; d_owner without d_geo; kind outside {0, 1}; d_ws not 8-byte aligned; the
 *   configuration errors of the geodesic calls.  EEA_ERR_UNSUPPORTED: their limits (xsize * ysize <= 2^26, sides of at most
 *   EEA_DISTANCE_MAX_SIDE).
 * eea_frontier_goals: each robot q < P picks among the records r < d_state[1] (read on the device; d_state and max_regions are
 *   those of the eea_frontier_regions call that wrote d_regions) with entry_owner == q, entry_cell >= 0 and size >= min_size
 *   the one of the greatest score, the lowest r on a tie.
 *   score            w_size * (double)size - w_cost * (double)entry_cost: both products rounded on their own, then subtracted,
 *                    in fp64 with no contraction (eea_partition_goals' arithmetic).
 *   d_goal_cell[q]   (int32) that record's entry_cell, or -1.
 *   d_goal_region[q] (int32) r, or -1.
 *   d_goal_score[q]  (double) the score, or 0.0.  EVERY element of the three is overwritten.
 *   The goal cell g has d_owner[g] == q and d_geo[g] >= 0 by construction, so d_goal_cell goes straight into
 *   eea_partition_path_batch and every robot with a goal gets len >= 0.  A robot whose region holds no entry gets -1.
 *   No workspace (d_goal_score's own 8 bytes hold an order-preserving integer of the score during the call); asynchronous on
 *   `stream`.  P == 0 is EEA_OK and touches nothing.  Before the device is selected -- EEA_ERR_INVALID_ARGUMENT: d_regions,
 *   d_state, d_goal_cell, d_goal_region or d_goal_score null; a weight that is not finite or outside [0, 1e30].
 *   EEA_ERR_UNSUPPORTED: P > 2^31 - 1.
 * eea_abi_version() stays 6. */
typedef struct eea_frontier_region { /* 56 bytes, 8-byte aligned */
  uint64_t sum_i, sum_j; /* sums of the members' rows / columns: centroid = sum / size */
  int32_t entry_cell;    /* member with the least (geo, row-major index); -1 without d_geo */
  int32_t entry_cost;    /* its geo; -1 without d_geo */
  int32_t root;          /* the region's label: least row-major index of a member */
  uint32_t size;         /* members */
  int32_t i_min, i_max, j_min, j_max;
  int32_t entry_owner;   /* d_owner[entry_cell]; -1 without d_owner */
  int32_t reserved;      /* 0 */
} eea_frontier_region;
enum { EEA_FRONTIER_OF_GRID = 0, EEA_FRONTIER_OF_MASK = 1 };
eea_status eea_frontier_ws_bytes(const eea_collision_cfg* cfg, size_t* bytes);
eea_status eea_frontier_regions(int device, const eea_collision_cfg* cfg, int kind, const int8_t* d_grid, const int* d_geo,
                                const int* d_owner, unsigned max_regions, int* d_root, int* d_region,
                                eea_frontier_region* d_regions, void* d_ws, unsigned* d_state, void* stream);
eea_status eea_frontier_goals(int device, const eea_frontier_region* d_regions, const unsigned* d_state, unsigned max_regions,
                              unsigned P, unsigned min_size, double w_size, double w_cost, int* d_goal_cell, int* d_goal_region,
                              double* d_goal_score, void* stream);

/* ---- frontier auction: a region for every robot, by distance and capacity (additive to ABI 6: detect these entries by
 * symbol) -----------------------------------------------------------------------------------------------------------------
 * No reference counterpart.  eea_frontier_goals gives a robot a region only if the robot OWNS the region's entry cell: a robot
 * whose share of free space holds no frontier stands still, and nothing limits how many robots go for one region or sends a
 * second robot to a large one.  The missing quantity is the distance from ANY robot to ANY region; a partition sourced at the
 * regions gives it for the whole fleet in one build (the nearest-frontier rule), and repeating the build with the full regions
 * closed makes it an auction.  The result is a function of the inputs alone: integers with a unique answer, way-points from the
 * literal arithmetic of eea_geodesic_path_batch.  Bit-reproducible.
 * eea_frontier_auction: d_region, d_regions, d_fstate and max_regions are the rank plane, the records, the state and the bound
 *   of one eea_frontier_regions call on the same grid (d_fstate[1] is read on the device); d_grid, d_sq, clear_sq are
 *   eea_geodesic_field's; flags takes only EEA_GEODESIC_UNKNOWN_BLOCKS.
 *   robot cell    c_q: the cell of pose q by eea_geodesic_field's source rule.  A robot is PLACED if that cell is in the grid and
 *                 does not block; a robot that is not placed never bids.
 *   enterable     a cell that is traversable exactly as eea_geodesic_field defines it, or the cell of a placed robot (a robot
 *                 is where it is: the test is waived for its cell, as it is for a source) -- for every robot, in every auction
 *                 round, so the plane is built once per call.
 *   eligible      a region r < min(d_fstate[1], max_regions) with size >= min_size.  Its capacity cap_r is 1 if
 *                 cells_per_robot == 0, else ceil(size_r / cells_per_robot) (in 64 bits); rem_r = cap_r before round 0.
 *   round a       a = 0 .. n_auction - 1.  If no placed robot is unassigned or no eligible region has rem_r > 0 the round is
 *                 idle and does nothing.  Otherwise:
 *     seeds       every cell g with d_region[g] = r, r eligible, rem_r > 0 and !blocks(d_grid[g]) holds the key (0, r), whether
 *                 it is enterable or not; nothing moves INTO a seed that is not enterable.
 *     field       the unique fixed point of eea_geodesic_partition's key rule on these seeds: the 5-7 chamfer moves into
 *                 enterable cells only, a diagonal one between two enterable cells, the key (cost, label) under lexicographic
 *                 order with label = region rank.
 *     bid         an unassigned placed robot q with a key (cost, r) at c_q bids for r with K_q = cost << 32 | q.
 *     accept      region r accepts the min(rem_r, bidders_r) bidders of the smallest K; rem_r drops by that number.
 *     an accepted robot gets d_goal_region[q] = r, d_goal_cost[q] = cost, and the walk from c_q down the field: the step rule
 *                 is eea_partition_path_batch's (the first of the eight moves onto a cell of label r that accounts for the
 *                 cost, a diagonal one between two cells of the field), until the cost is 0.  d_goal_cell[q] is the cell
 *                 where the walk ends -- a member of r -- also for a walk longer than n_steps.  Rows, headings, the repeat rule
 *                 and d_len are eea_geodesic_path_batch's; the moves are forward ones, nothing is reversed.  A robot on a
 *                 seed gets len 0, its own cell as goal, and n_steps rows of its cell's centre with the pose's heading.
 *   A robot that is unassigned after the last round, or not placed, gets goal_region = goal_cell = goal_cost = len = -1 and
 *   its pose in all rows.  EVERY element of d_goal_region, d_goal_cell, d_goal_cost [P], d_path [P][n_steps][3] and d_len [P] is
 *   overwritten.  n_steps == 0 is allowed with d_path == NULL; d_len may be NULL.
 *   max_rounds    as eea_geodesic_partition's.  0: every field is built to the end; the call waits on `stream` and reads state
 *                 words on the host every 16 tile rounds, and stops at the first idle auction round.  > 0: the call enqueues
 *                 3 + n_auction * (max_rounds + 6) launches on `stream` and neither allocates, waits nor reads; an idle auction
 *                 round leaves every tile flag 0, so its round launches exit at once.
 *   d_state       (uint32 [4], device) [0] 1 iff every field build of the call was final; [1] the tile rounds that changed
 *                 something, summed over the call; [2] the robots assigned; [3] the auction rounds that were not idle.  With
 *                 [0] == 1 the outputs are bitwise the definition above.  With [0] == 0 each output element is -1, or the pose,
 *                 or in range; nothing more is promised, and the caller must look at [0].
 *   The launches: once per call the traversability plane, one lane per robot (its cell, the byte of that cell, the outputs'
 *   unassigned state) and one lane per record (rem_r); per auction round a pass that seeds the key plane, the tile rounds of
 *   eea_geodesic_partition, a pass that unpacks the keys, one lane per robot that bids (the bidders of a region counted with
 *   integer atomics, combined per wavefront), one lane per robot that counts its rank -- the bids of the same region with a
 *   smaller K, against all P bids streamed through LDS; K is unique, so no atomics -- and, accepted, writes its outputs and
 *   walks, and one lane per record that lowers rem_r and counts the open regions and the unassigned robots for the next
 *   round's idle test.  Nothing waits inside a kernel.
 *   eea_frontier_auction_ws_bytes: host only; the bytes d_ws must hold (positive, monotone in the grid's size, in P and in
 *   max_regions).  d_ws is device memory aligned to 8 bytes; its contents mean nothing between calls.
 *   P == 0 is EEA_OK: it writes d_state = {1, 0, 0, 0} and nothing else.
 *   Before the device is selected, with no output touched -- EEA_ERR_INVALID_ARGUMENT: cfg, d_grid, d_region, d_fstate, d_pose
 *   (with P > 0), d_goal_region, d_goal_cell, d_goal_cost, d_ws or d_state null; d_regions null with max_regions > 0; d_path
 *   null with n_steps > 0; clear_sq < 0; unknown flag bits; n_auction == 0; d_ws not 8-byte aligned; the configuration errors of
 *   the geodesic calls.  EEA_ERR_UNSUPPORTED: their limits; P > 65536 (the bound of the all-pairs rank: to be lifted only with
 *   a sort); max_regions > 2^31 - 1.
 * eea_abi_version() stays 6. */
eea_status eea_frontier_auction_ws_bytes(const eea_collision_cfg* cfg, unsigned P, unsigned max_regions, size_t* bytes);
eea_status eea_frontier_auction(int device, const eea_collision_cfg* cfg, const int8_t* d_grid, const int* d_sq, int clear_sq,
                                unsigned flags, const int* d_region, const eea_frontier_region* d_regions,
                                const unsigned* d_fstate, unsigned max_regions, const double* d_pose, unsigned P,
                                unsigned n_auction, unsigned min_size, unsigned cells_per_robot, unsigned max_rounds,
                                unsigned n_steps, int* d_goal_region, int* d_goal_cell, int* d_goal_cost, double* d_path,
                                int* d_len, void* d_ws, unsigned* d_state, void* stream);

/* ---- goal paths: every robot's way to its OWN goal, one bounded window each (additive to ABI 6: detect this entry by
 * symbol) -----------------------------------------------------------------------------------------------------------------
 * No reference counterpart.  eea_geodesic_path_batch walks to the nearest source of ONE field, eea_partition_path_batch to a goal
 * inside the robot's own cell of the partition, eea_frontier_auction to the region it has just assigned.  A goal from anywhere
 * else -- the one a robot was given last tick, an operator's way-point, a rendezvous cell -- had one whole-grid
 * eea_geodesic_field per distinct goal as its only route to a path.  Here every robot's shortest path is computed inside a
 * bounded window around the robot and its goal: the work follows the distance to the goal, not the size of the map.  The result
 * is a function of the inputs alone: integers with a unique answer, way-points from the literal arithmetic of
 * eea_geodesic_path_batch.  Bit-reproducible.
 * eea_geodesic_goto_batch: d_grid, d_sq, clear_sq, blocks(v), the cell of a pose with gridBounds, traversable and the 5-7 moves
 *   without corner cutting are eea_geodesic_field's; flags takes only EEA_GEODESIC_UNKNOWN_BLOCKS.  Per robot q of d_pose [P][3]
 *   with d_mask == NULL || d_mask[q] != 0 (d_mask: int32 [P]), decided in this order:
 *   1 robot cell  c_q = (i_c, j_c): the cell of pose q.  Off the grid, or blocks(d_grid[c_q]): status EEA_GOTO_NO_ROBOT.
 *   2 goal        g = d_goal[q] (int32, a row-major index), (i_g, j_g) its row and column.  g < 0, g >= xsize * ysize or
 *                 blocks(d_grid[g]): status EEA_GOTO_NO_GOAL.
 *   3 window      rows [min(i_c, i_g) - margin, max(i_c, i_g) + margin] and columns [min(j_c, j_g) - margin, max(j_c, j_g) +
 *                 margin], computed in 64 bits, then clipped to the grid: h rows, w columns.  h * w > EEA_GOTO_MAX_CELLS:
 *                 status EEA_GOTO_WINDOW.
 *   4 field       the unique fixed point of eea_geodesic_field's rule on the cells of the window only -- a move never leaves
 *                 the window --, its one source g seeded with 0.  The unknown test and the clearance test are waived for g, as
 *                 for any source (nothing moves into a g that is not traversable), and c_q is enterable whatever those tests
 *                 say, as it is in eea_frontier_auction (a robot is where it is).
 *   5             c_q has no cost: status EEA_GOTO_CUT_OFF (inside THIS window: a larger margin may find a way).
 *   6             otherwise status EEA_GOTO_OK.
 *   An OK robot gets d_cost[q] = the cost at c_q and the forward walk from c_q down the field by eea_geodesic_path_batch's step
 *   rule: the eight moves tried in its order, the first whose target accounts for the cost taken, a diagonal one only between
 *   two cells that have a cost; way-point centres (on the whole grid's indices), the eight literal headings and the repeat rule
 *   are eea_geodesic_path_batch's.  len = the number of moves written, <= n_steps; the cost is the whole path's even when n_steps
 *   is shorter.  A robot on its goal gets cost 0, len 0 and n_steps rows of its cell's centre with the pose's heading.  Every
 *   other status gives cost = len = -1 and the pose in all rows.  EVERY element of d_cost, d_status, d_len [P] (int32) and d_path
 *   [P][n_steps][3] that belongs to a robot that is not masked out is overwritten; of a masked-out robot nothing is read and
 *   nothing written.  n_steps == 0 is allowed with d_path == NULL; d_len may be NULL.
 *   d_state       (uint32 [4], device) is overwritten with four counts over the robots that are not masked out: [0] OK, [1]
 *                 WINDOW, [2] CUT_OFF, [3] NO_ROBOT + NO_GOAL.
 *   The caller falls back to the whole-grid field for a robot with status WINDOW or CUT_OFF; the cost of an OK robot is that of
 *   the best path INSIDE the window, which is the whole grid's once the window holds such a path (it does not rise with margin).
 *   The launches: one lane group clears d_state; then one workgroup of 256 threads per robot (a launch of at most 2048
 *   workgroups strides over the robots) stages the window in LDS -- one 32-bit word per cell, a cost or "no move may enter",
 *   EEA_GOTO_MAX_CELLS of them being 64 KB, so that two workgroups share a CU --, relaxes it in place to its fixed point with one workgroup-wide OR
 *   per sweep, walks, and writes the rows; the counts are integer atomics, combined per workgroup first.  A value that cannot
 *   lie on the robot's walk (>= the cost its own cell holds) is not stored.  No workspace, no allocation, nothing read on the
 *   host, no synchronising call, nothing waits inside the kernel: asynchronous on `stream`.
 *   P == 0 is EEA_OK: it writes d_state = {0, 0, 0, 0} and nothing else.
 *   Before the device is selected, with no output touched -- EEA_ERR_INVALID_ARGUMENT: cfg, d_grid, d_cost, d_status or d_state
 *   null; d_pose or d_goal null with P > 0; d_path null with n_steps > 0; clear_sq < 0; unknown flag bits; the configuration
 *   errors of the geodesic calls.  EEA_ERR_UNSUPPORTED: their limits; P > 2^31 - 1.
 * eea_abi_version() stays 6. */
#define EEA_GOTO_MAX_CELLS 16384 /* a window's cells: one 4-byte word of LDS each, 64 KB */
enum { EEA_GOTO_OK = 0, EEA_GOTO_NO_ROBOT = 1, EEA_GOTO_NO_GOAL = 2, EEA_GOTO_WINDOW = 3, EEA_GOTO_CUT_OFF = 4 };
eea_status eea_geodesic_goto_batch(int device, const eea_collision_cfg* cfg, const int8_t* d_grid, const int* d_sq,
                                   int clear_sq, unsigned flags, const double* d_pose, const int* d_goal,
                                   const int* d_mask, unsigned P, unsigned margin, unsigned n_steps, int* d_cost,
                                   int* d_status, double* d_path, int* d_len, unsigned* d_state, void* stream);

/* ---- footprint collision: a convex polygon base, checked through the distance field ----------------------------------
 * No reference counterpart (the reference README lists "model the robot's base as a polygon for collision detection" and "use
 * a distance field for detecting obstacle cells" under "Future Improvements").  Every other collision call treats the robot
 * as a disc and reads no heading; these read all three components of a pose.  They stand beside those calls and change none.
 *
 * The footprint: n vertices (x[k], y[k]) in the body frame, in metres, counter-clockwise and strictly convex, the body origin
 * (the pose) strictly inside.  There is no padding: a caller who wants a margin passes a larger polygon.  Edge k runs from
 * vertex k to vertex k + 1 (mod n); the host derives, each operation rounded on its own,
 *   ex = x[k+1] - x[k], ey = y[k+1] - y[k], len = sqrt(ex * ex + ey * ey), (nx, ny) = (ey / len, -ex / len),
 *   h = nx * x[k] + ny * y[k];   r_in = min h_k,   r_out = max sqrt(x[k] * x[k] + y[k] * y[k]).
 *
 * The verdict (the definition; the field is an optimisation of it): a pose (px, py, th) with all three components finite
 * collides iff some in-grid cell (i, j) is occupied by checkCell's test, !(int8 / 100.0 < occupied_threshold), and its centre
 * (GridMap::grid2World, grid.cpp:126-131) lies in the closed footprint placed at the pose:
 *   cxw = j * res + res / 2.0 + xmin,  cyw = i * res + res / 2.0 + ymin,  dx = cxw - px,  dy = cyw - py,  (s, c) = sincos(th),
 *   bx = c * dx + s * dy,  by = (-s) * dx + c * dy;   inside iff nx_k * bx + ny_k * by <= h_k for every k
 * (no fused multiply-add).  A pose with a non-finite component collides with nothing.  The robot's own cell need not be on
 * the grid: a base that hangs over the map's edge collides with the in-grid cells it covers, and nothing off the grid is an
 * obstacle.  Sine and cosine are the device's, within a few ulp of libm: the verdict is pinned wherever no occupied centre
 * lies within 1e-9 m of the footprint's boundary.  Of cfg only the geometry and occupied_threshold are read; the radii are
 * neither read nor checked.
 *
 * d_sq (may be NULL): the plane eea_distance_field built for the same grid and threshold.  A pose whose own cell
 * (floor((px - xmin) / res), floor((py - ymin) / res)) -- compared as doubles, no wrap, no upper-edge step -- is on the grid
 * then reads one int: an occupied centre inside the inscribed circle is a hit, none inside the circumscribed circle is free,
 * with 0.7072 + 1e-6 cells of margin for the pose's place in its cell; only the band in between takes the test above, over
 * the cells within ceil(r_out / res) + 1 of the pose's.  The filter never contradicts the definition; without d_sq every
 * pose takes the test.  Both device calls are asynchronous on `stream`, allocate nothing and keep nothing between calls;
 * eea_abi_version() stays 6.
 * Before the device is selected, with no output touched -- EEA_ERR_INVALID_ARGUMENT: a required pointer null (cfg, fp,
 * d_grid, the poses, the output); n < 3 or n > EEA_FOOTPRINT_MAX_VERTICES; a vertex not finite; a turn not strictly left (the
 * cross product of consecutive edges <= 0); some h_k <= 0; xsize or ysize 0; resolution <= 0; T == 0 or T > 2^31 - 1.
 * EEA_ERR_UNSUPPORTED: xsize * ysize > 2^31; r_out / res > 1024. */
#define EEA_FOOTPRINT_MAX_VERTICES 16
typedef struct {
  unsigned n;
  double x[EEA_FOOTPRINT_MAX_VERTICES], y[EEA_FOOTPRINT_MAX_VERTICES];
} eea_footprint;
/* host only, needs no device: validates fp (the footprint's errors above) and returns the radii of the inscribed and the
 * circumscribed circle about the body origin; r_in and r_out may each be NULL */
eea_status eea_footprint_radii(const eea_footprint* fp, double* r_in, double* r_out);
/* d_hit [P] = 1 (collides) or 0 per pose of d_pose [P][3].  P == 0 is EEA_OK with nothing launched. */
eea_status eea_footprint_check_batch(int device, const eea_collision_cfg* cfg, const eea_footprint* fp, const int8_t* d_grid,
                                     const int* d_sq, const double* d_pose, unsigned P, int* d_hit, void* stream);
/* d_step [B] = the first colliding step of each trajectory d_traj [B][T][3] (the layout of eea_rollout_batch's output,
 * eea_control_batch's d_traj and eea_tick_io.d_traj), -1 when none collides.  B == 0 is EEA_OK with nothing launched. */
eea_status eea_footprint_traj_first(int device, const eea_collision_cfg* cfg, const eea_footprint* fp, const int8_t* d_grid,
                                    const int* d_sq, const double* d_traj, unsigned B, unsigned T, int* d_step, void* stream);

/* ---- footprint planning: the polygon base in validate_control, the dynamic window and the tick -------------------------
 * The three calls that decide a robot's motion, with the verdict above in place of the disc's collisionCheck.  They are defined
 * by composition and add no numerics: the poses of a rollout are those of eea_validate_control_batch / eea_dwa_control_batch
 * bit for bit (the same twist step, the heading wrapped), every pose is judged as eea_footprint_check_batch judges a pose, and
 * the window bounds, both objectives, the first strict minimum in loop order, found and u_opt = 0 are eea_dwa_control_batch's.
 * Sine and cosine of a pose's heading are the rollout's own; the verdict is pinned under the rule above (no occupied centre
 * within 1e-9 m of the polygon's boundary).  d_sq may be NULL; with it the outputs are the same bits.  Of the collision cfg only
 * the geometry and occupied_threshold are read.  Additive to ABI 6 (eea_abi_version() stays 6); asynchronous on `stream`, nothing
 * allocated, nothing kept between calls.  P == 0 / B == 0 is EEA_OK with nothing launched.
 * Refusals, before the device is selected and with no output touched: eea_footprint_check_batch's for cfg / fp / d_grid
 * (r_out / res > 1024 included), then eea_validate_control_batch's / eea_dwa_control_batch's for the rest (null pointers; both or
 * neither of d_vref / d_xt_ref; n_ref == 0; more than 8192 samples; a rollout that would read past its reference). */
/* validate_control (numerics.hpp:312-330): d_valid [P] = 1 when no step of the rollout of d_u [P][3] from d_x0 [P][3] collides */
eea_status eea_footprint_validate_control_batch(int device, const eea_collision_cfg* cfg, const eea_footprint* fp,
                                                const int8_t* d_grid, const int* d_sq, const double* d_x0, const double* d_u,
                                                double dt, double horizon, unsigned P, int* d_valid, void* stream);
/* DynamicWindow::control (dynamic_window.cpp:92-286), both modes as in eea_dwa_control_batch (d_vref, or d_xt_ref / n_ref /
 * dt_ref) */
eea_status eea_footprint_dwa_control_batch(int device, const eea_collision_cfg* ccfg, const eea_dwa_cfg* dcfg,
                                           const eea_footprint* fp, const int8_t* d_grid, const int* d_sq, const double* d_x0,
                                           const double* d_vb, const double* d_vref, const double* d_xt_ref, unsigned n_ref,
                                           double dt_ref, unsigned P, double* d_u_opt, int* d_found, void* stream);
/* eea_tick_batch with the footprint in steps 3 and 4; steps 1 and 2 are eea_tick_batch's, and d_valid, d_follow_dwa,
 * d_dwa_count, d_u and d_source mean what they mean there.  tick->grid_epoch is ignored (there is no inflated map to cache):
 * the caller rebuilds d_sq with eea_distance_field when the grid changes.  Refusals: eea_tick_batch's, in its order, with fp
 * and the grid's geometry checked where eea_tick_batch_fleet checks its layer. */
eea_status eea_tick_batch_footprint(eea_engine* e, unsigned B, const eea_batch_io* io, const eea_tick_io* tick,
                                    const eea_collision_cfg* ccfg, const eea_dwa_cfg* dcfg, const eea_footprint* fp,
                                    const int* d_sq, void* stream);

/* ---- body layer: polygon robots as obstacles to one another (additive to ABI 6: detect these entries by symbol) -----------
 * The fleet layer above makes the robots of a tick obstacles to one another as DISCS; the footprint calls judge a robot by
 * its polygon but know no other robot.  A body layer joins them: one footprint per layer, shared by all B robots, as
 * eea_tick_batch_footprint takes one.  No reference counterpart.
 *
 * The cell test.  T(cell, pose) is the closed test of the cell's centre against the polygon placed at the pose -- the
 * products and sums written under "footprint collision" above, in that order, no fused multiply-add -- with the sine and the
 * cosine the rollouts use.
 *
 * Obstacles.  At an update robot j is STAMPED iff it is active (d_mask == NULL or d_mask[j] != 0), its pose is finite, and its
 * box touches the grid: with fx = floor((px - xmin) / res), fy likewise, box = ceil(r_out / res) + 1, all as doubles,
 * fx + box >= 0, fx - box <= xsize - 1, fy + box >= 0, fy - box <= ysize - 1.  The body of robot j is the set of IN-GRID
 * cells c with T(c, pose_j at the update), whatever those cells hold and whatever occupied_threshold is.  Nothing off the grid
 * is an obstacle: a body that hangs over the edge is its in-grid part.
 *
 * The verdict of a pose q that belongs to robot i (d_self[q] = i; in the tick: robot r's poses belong to robot r) is the
 * footprint's verdict on a grid of robot i's own -- the grid with every cell of every OTHER stamped robot's body occupied:
 *   the static verdict, OR some in-grid cell c has T(c, q) and T(c, pose_j) for a stamped j != i.
 * A robot is never its own obstacle.  d_self == NULL or d_self[q] == -1: nobody's body is taken out.  A d_self entry outside
 * [-1, B) is the caller's error and is not checked.
 *
 * Staleness, as in the fleet layer: the others stand still at the poses of the last update for a whole rollout.  Robots whose
 * bodies share a cell at the update are in collision where they stand: every rollout of either that has not left the overlap
 * by its first step collides, validate_control rejects every twist that does not, and the dynamic window finds nothing unless
 * a sample leaves at once.  Keeping the bodies apart is the planner's job from the tick before.
 *
 * Composition.  Rollouts, window bounds, costs, the first strict minimum, found and u_opt = 0 are bit for bit those of
 * eea_footprint_validate_control_batch / eea_footprint_dwa_control_batch.  d_sq (the distance field of the STATIC grid, may be
 * NULL) never changes an output bit, and neither does any filter inside the layer.  The verdict is pinned wherever no centre
 * lies within 1e-9 m of a boundary it is tested against: the polygon at q against the occupied centres and the centres of the
 * others' bodies, and every stamped polygon against the in-grid centres.
 *
 * eea_body_layer_read (for tests and tools; synchronises; any pointer may be NULL; it also verifies the guard words the layer
 * keeps on either side of its maps in device memory and answers EEA_ERR_HIP if one was overwritten):
 *   h_cover [ysize][xsize] int: the number of stamped robots whose body holds the cell;
 *   h_near [ysize + 2 box][xsize + 2 box] int over the cells [-box, xsize + box) x [-box, ysize + box): the stamped robots whose
 *     cell (fx, fy) lies within Chebyshev distance Rn = 2 ceil(r_out / res) + 2 of this one.  near minus the pose's own robot
 *     (when stamped and within Rn) == 0 proves that no other body shares a cell with a polygon placed in this cell; it is
 *     used for nothing else;
 *   h_snapshot [B][5] double: px, py, sine, cosine of the pose the robot was stamped with and 1.0, or five zeros.
 * flags: EEA_BODY_LAYER_NO_FILTER skips near -- every pose with a non-empty box takes the exact test (so that the filter can
 * be tested on the device, as d_sq == NULL tests the field).
 *
 * An update is stream operations only (one clear, one stamp kernel, two row scans): no host read, no allocation, no
 * synchronising call; the readers on the same stream see it.  Before the first update no robot is an obstacle.
 * Refusals, before any HIP call, outputs untouched, the message naming the entry -- creation: NULL cfg / fp / out; the
 * footprint's and the grid's refusals of eea_footprint_check_batch (EEA_ERR_UNSUPPORTED: xsize * ysize > 2^31, r_out / res >
 * 1024, a near map above 2^31 cells); B == 0; unknown flag bits.  The batch entries: those of the footprint entries they extend
 * (NULL l / poses / outputs; d_grid NULL except in eea_body_collision_check_batch, where it means robots only; the dynamic
 * window's).  eea_tick_batch_bodies: eea_tick_batch_footprint's, in its order; where eea_tick_batch_fleet checks its layer: ccfg
 * must give the layer's geometry and occupied_threshold, B the layer's B, and the layer must live on the engine's device. */
#define EEA_BODY_LAYER_NO_FILTER 1u
typedef struct eea_body_layer eea_body_layer;
eea_status eea_body_layer_create(int device, const eea_collision_cfg* cfg, const eea_footprint* fp, unsigned B, unsigned flags,
                                 eea_body_layer** out);
void eea_body_layer_destroy(eea_body_layer* l);
/* d_pose [B][3], d_mask [B] (may be NULL: all active) */
eea_status eea_body_layer_update(eea_body_layer* l, const double* d_pose, const int* d_mask, void* stream);
eea_status eea_body_layer_read(const eea_body_layer* l, int* h_cover, int* h_near, double* h_snapshot);
/* box = ceil(r_out / res) + 1 of the layer (-1: NULL) */
int eea_body_layer_box(const eea_body_layer* l);
/* eea_footprint_check_batch with the layer; d_grid == NULL: robots only (d_sq is then ignored) */
eea_status eea_body_collision_check_batch(const eea_body_layer* l, const int8_t* d_grid, const int* d_sq, const double* d_pose,
                                          const int* d_self, unsigned P, int* d_hit, void* stream);
/* eea_footprint_validate_control_batch / eea_footprint_dwa_control_batch with the layer; d_self [P] as above */
eea_status eea_body_validate_control_batch(const eea_body_layer* l, const int8_t* d_grid, const int* d_sq, const double* d_x0,
                                           const double* d_u, const int* d_self, double dt, double horizon, unsigned P,
                                           int* d_valid, void* stream);
eea_status eea_body_dwa_control_batch(const eea_body_layer* l, const eea_dwa_cfg* dcfg, const int8_t* d_grid, const int* d_sq,
                                      const double* d_x0, const double* d_vb, const double* d_vref, const double* d_xt_ref,
                                      unsigned n_ref, double dt_ref, const int* d_self, unsigned P, double* d_u_opt, int* d_found,
                                      void* stream);
/* eea_tick_batch_footprint with the layer in steps 3 and 4: robot r of the tick is robot r of the layer (updated on the same
 * stream before) */
eea_status eea_tick_batch_bodies(eea_engine* e, unsigned B, const eea_batch_io* io, const eea_tick_io* tick,
                                 const eea_collision_cfg* ccfg, const eea_dwa_cfg* dcfg, const eea_body_layer* l, const int* d_sq,
                                 void* stream);

/* The collision / DWA / tick / clearance calls keep small device caches between calls (the ring offsets per radii, one
 * inflated-map and one key-map buffer per (device, stream), the span tables of fleet layers that no layer holds any more).  A long-running
 * process that changes streams or map sizes can drop them; synchronises the devices involved.  No reference counterpart. */
void eea_release_collision_caches(void);

#ifdef __cplusplus
}
#endif
#endif
