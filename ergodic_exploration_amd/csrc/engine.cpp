// C ABI (include/ergodic_amd.h) of the MI355X ergodic receding-horizon engine: argument
// checking, device-memory ownership and kernel dispatch.  All arithmetic of the hot path
// runs in the HIP kernels (control_kernel.hip, phik_kernel.hip, collision_kernel.hip); the
// host code here only prepares their inputs the way the reference's host code does
// (steps_ truncation, grid coordinates by accumulation, covariance inverse).
// This file: the entries that take an eea_engine (and the free functions of the controller's classes).  The entries that take
// a device or a layer are grid_entries.cpp; what both need is entry_util.hpp.
#include "../../include/ergodic_amd.h"

#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "entry_util.hpp"

// (of entry_util.hpp: the buffers of the engine, and what eea_set_target_gain and the ticks ask of their arguments)
using eea::as;
using eea::collision_cfg_refusal;
using eea::collision_params;
using eea::DevBuf;
using eea::dwa_window_refusal;
using eea::footprint_call_refusal;
using eea::gain_refusal;
using eea::grid_params;
using eea::horizon_steps;
using eea::named;

namespace
{
using eea::fail;

// process-wide dispatch options (eea_set_option); index = EEA_OPT_*
std::atomic<int> g_options[EEA_OPT_COUNT] = { { 0 }, { 0 }, { 0 }, { 1 }, { 0 }, { 0 }, { 0 }, { 250 } };
}  // namespace

namespace eea
{
int option(int id) { return (id >= 0 && id < EEA_OPT_COUNT) ? g_options[id].load(std::memory_order_relaxed) : 0; }
}  // namespace eea

namespace
{
using eea::fail;

// grid.hpp:61-64 of the reference (x86-64 cast semantics do not matter here: non-negative)
unsigned axis_length(double lower, double upper, double resolution)
{
  return static_cast<unsigned>(std::round((upper - lower) / resolution));
}

// Accumulated grid coordinates and the cos tables built from them (cx [K][nx], cy [ny][K]) of ONE grid and domain.  The
// coordinates 0, res, res + res, ... (ergodic_control.hpp:387-408) depend only on the resolution: one array serves both
// axes of every grid, generated once and extended when a larger grid appears -- no upload on a repeated call.  The key
// says which tables cx / cy hold: a repeated call on the same grid and domain reuses them.  When the buffers may be
// replaced or rewritten under earlier launches is the owner's business (the phi_k path and eea_records_field differ).
struct AxisTables
{
  DevBuf axis, cx, cy;
  unsigned axis_n = 0;
  unsigned nx = 0, ny = 0;  // key (0: none)
  double lx = 0.0, ly = 0.0;

  bool holds(unsigned nx_, unsigned ny_, double lx_, double ly_) const { return nx == nx_ && ny == ny_ && lx == lx_ && ly == ly_; }
  void forget() { nx = ny = 0; }
  // records the key once the launch that writes the tables is enqueued: a failure before must not leave it on tables that
  // were never written
  void remember(unsigned nx_, unsigned ny_, double lx_, double ly_)
  {
    nx = nx_;
    ny = ny_;
    lx = lx_;
    ly = ly_;
  }
  // at least n coordinates: repeated += resolution from 0, cast per element (blocking upload)
  template <typename R>
  eea_status extend_axis(unsigned n, double resolution)
  {
    if (n <= axis_n) return EEA_OK;
    unsigned count = axis_n ? 2 * axis_n : 2048;
    if (count < n) count = n;
    std::vector<R> v(count);
    double x = 0.0;
    for (unsigned i = 0; i < count; ++i) {
      v[i] = static_cast<R>(x);
      x += resolution;
    }
    axis_n = 0;
    EEA_HIP(axis.reserve(sizeof(R) * count));
    EEA_HIP(hipMemcpy(axis.p, v.data(), sizeof(R) * count, hipMemcpyHostToDevice));
    axis_n = count;
    return EEA_OK;
  }
  // one launch on s writes both tables (cx / cy hold nx * K and ny * K reals) and records the key
  template <typename R>
  eea_status launch(unsigned nx_, unsigned ny_, int K, double lx_, double ly_, hipStream_t s)
  {
    EEA_HIP(eea::launch_axis_tables<R>(as<R>(axis.p), nx_, ny_, K, static_cast<R>(eea::kPi / lx_), static_cast<R>(eea::kPi / ly_),
                                       as<R>(cx.p), as<R>(cy.p), s));
    remember(nx_, ny_, lx_, ly_);
    return EEA_OK;
  }
};

// host mailbox of the single-agent path, device-visible (zero-copy over PCIe)
struct Mailbox
{
  double pose[3];  // viewed as R[3]
  double u0[3];    // viewed as R[3]
  int status;
  int done;  // completion sequence number written by the kernel (polled by eea_control)
};
}  // namespace

struct eea_engine
{
  eea_config cfg;
  int T = 0, K = 0, K2 = 0;
  bool f32 = false;
  size_t rs = 8;  // sizeof(real)
  int chunk = 128;

  // Basis state (basis_.lx_, ly_ start at 0: ergodic_control.hpp:208): the domain of the phi_k the engine holds, written by
  // commit_phik alone
  double lx = 0.0, ly = 0.0, map_x = 0.0, map_y = 0.0;
  bool have_phik = false;
  std::vector<double> mu, sigma;  // target Gaussians, map frame
  bool have_gauss = false;

  DevBuf d_phik, d_lamdak;
  // phi grid of the last rebuild
  unsigned nx = 0, ny = 0;
  bool have_fill_grid = false;  // d_phi holds the Target::fill output of the last rebuild ...
  bool phi_is_raw = false;      // ... un-normalised: d_sum[0] is its mass (eea_get_target_grid divides)
  // ... or WILL hold it: a Gaussian rebuild computes phi_k from the per-axis factors without the grid; the grid is
  // filled when eea_get_target_grid asks for it, from the Gaussians as they were at the rebuild (Fourier frame)
  bool fill_deferred = false;
  std::vector<double> fill_gauss;  // [n][4] of the last rebuild: mean - map_pos, diag(cov_inv)
  DevBuf d_phi, d_work, d_gauss, d_sum;
  AxisTables tab;         // of the last rebuild / row tile
  bool have_lut = false;  // the entropy decode table is uploaded once
  hipEvent_t ev_done = nullptr;  // completion of a rebuild: polled (a few microseconds earlier than a blocking wait)
  // a rebuild that was only enqueued (eea_config_domain_async): control calls on OTHER streams wait for this event
  hipEvent_t ev_rebuild = nullptr;
  hipStream_t rebuild_stream = nullptr;
  bool rebuild_pending = false;
  DevBuf d_lut, d_raw, d_occ;  // occupancy targets: decode table, un-normalised sums, staged cells
  // eea_set_target_gain / eea_set_target_mi: the field (uint32 / double; when the caller passes no buffer), its value grid
  DevBuf d_gain, d_gain_val;

  // eea_records_field's OWN tables, apart from the phi_k path's: a field on another grid never evicts tab / d_work and adds no
  // wait to a rebuild
  AxisTables field;
  hipEvent_t ev_field_used = nullptr;  // behind the last field launch: its tables are rewritten in place only after it
  std::mutex field_mutex;

  // workspaces of eea_ck_records_sum (group records of both levels + the tickets of its tree), one per distinct output
  // buffer: concurrent calls on several streams must not share tickets
  struct SumWs
  {
    const void* key = nullptr;
    unsigned long last_use = 0;
    hipStream_t last_stream = nullptr;  // the stream of the last launch that used the buffers
    DevBuf ws, ctr;
  };
  std::vector<std::unique_ptr<SumWs>> sum_ws;  // (pointers: a workspace in use must not move when the list grows)
  std::mutex sum_mutex;
  unsigned long sum_clock = 0;
  // device buffers replaced while launches may still use them: freed once the event recorded behind their last launch has
  // completed (or with the engine)
  struct Retired
  {
    void* p;
    hipEvent_t done;
  };
  std::vector<Retired> retired;

  // single-agent path
  hipStream_t stream1 = nullptr;
  Mailbox* h_mail = nullptr;
  void* d_mail = nullptr;
  DevBuf d_ut1, d_traj1, d_mem1;
  void* h_stage = nullptr;  // pinned staging for mem_cols / ut transfers
  size_t h_stage_cap = 0;
  double last_pose[3] = { 0, 0, 0 };
  int mail_seq = 0;          // sequence number of the last single-agent launch
  unsigned long phik_gen = 0;  // bumped whenever phi_k / the domain changes

  // resident single-robot workgroup (EEA_OPT_RESIDENT_CONTROL): host-mapped mailbox + replay-memory buffer, its own stream
  void* h_rmail = nullptr;
  void* d_rmail = nullptr;
  void* h_rmem = nullptr;
  void* d_rmem = nullptr;
  DevBuf d_rstage;             // ResidentStage: the request's pose / column count in device memory
  hipStream_t stream_res = nullptr;
  bool res_launched = false;   // a workgroup was launched and has not been seen to leave
  bool res_one_wavefront = false;  // ... the one-wavefront form (horizons of one slot): its controls live in LDS between requests
  unsigned res_seq = 0;        // last request number
  unsigned long res_gen = 0;   // phik_gen it was launched with
};

namespace
{
template <typename R>
void to_real(const double* in, R* out, size_t n)
{
  for (size_t i = 0; i < n; ++i) out[i] = static_cast<R>(in[i]);
}

// f(float{}) or f(double{}) by the engine's precision: what a call does is written once, with R = the type of f's argument
template <typename F>
auto by_precision(const eea_engine* e, F&& f)
{
  return e->f32 ? f(float{}) : f(double{});
}

// n doubles of the caller as the engine's reals in host memory (the mirror of download_reals)
void store_reals(const eea_engine* e, const double* in, void* out, size_t n)
{
  by_precision(e, [&](auto r) { to_real(in, as<decltype(r)>(out), n); });
}

eea_status use_device(const eea_engine* e)
{
  EEA_HIP(hipSetDevice(e->cfg.device));
  return EEA_OK;
}

eea_status stage_reserve(eea_engine* e, size_t bytes)
{
  if (bytes <= e->h_stage_cap) return EEA_OK;
  // grows geometrically: the replay memory adds a column per tick until it reaches the batch size
  size_t want = e->h_stage_cap ? 2 * e->h_stage_cap : 4096;
  if (want < bytes) want = bytes;
  if (e->h_stage) (void)hipHostFree(e->h_stage);
  e->h_stage = nullptr;
  e->h_stage_cap = 0;
  EEA_HIP(hipHostMalloc(&e->h_stage, want, hipHostMallocDefault));
  e->h_stage_cap = want;
  return EEA_OK;
}

// waits for everything enqueued on `s` so far: records an event and polls it (bounded), then the ordinary wait
eea_status wait_stream_spin(eea_engine* e, hipStream_t s)
{
  if (e->ev_done == nullptr) EEA_HIP(hipEventCreateWithFlags(&e->ev_done, hipEventDisableTiming));
  EEA_HIP(hipEventRecord(e->ev_done, s));
  for (int spin = 0; spin < 200000; ++spin) {
    const hipError_t q = hipEventQuery(e->ev_done);
    if (q == hipSuccess) return EEA_OK;
    if (q != hipErrorNotReady) return fail(EEA_ERR_HIP, std::string("hipEventQuery: ") + hipGetErrorString(q));
  }
  EEA_HIP(hipStreamSynchronize(s));
  return EEA_OK;
}

template <typename R>
eea_status upload_lamdak(eea_engine* e)
{
  // basis.cpp:69-75: lamdak = 1 / (1 + sqrt(k1^2 + k2^2))^1.5, col = k2*K + k1
  std::vector<R> lam(e->K2);
  for (int k2 = 0; k2 < e->K; ++k2) {
    for (int k1 = 0; k1 < e->K; ++k1) {
      const double ss = static_cast<double>(k1 * k1 + k2 * k2);
      lam[k2 * e->K + k1] = static_cast<R>(1.0 / std::pow(1.0 + std::sqrt(ss), 1.5));
    }
  }
  EEA_HIP(e->d_lamdak.reserve(sizeof(R) * e->K2));
  EEA_HIP(e->d_phik.reserve(sizeof(R) * e->K2));
  EEA_HIP(hipMemcpy(e->d_lamdak.p, lam.data(), sizeof(R) * e->K2, hipMemcpyHostToDevice));
  EEA_HIP(hipMemset(e->d_phik.p, 0, sizeof(R) * e->K2));
  return EEA_OK;
}

// The one place a new phi_k becomes the engine's: the domain it was formed on (fill_params and engine_view read it, and
// eea_config_domain compares the next map with it) and the generation the resident single-robot workgroup restarts on.
// Called once the last launch or copy of the call that forms phi_k has been issued successfully -- a call that fails
// leaves the engine on the domain of the phi_k it still holds.
void commit_phik(eea_engine* e, double lx, double ly)
{
  e->lx = lx;
  e->ly = ly;
  e->have_phik = true;
  ++e->phik_gen;
}

// the phi_k path's coordinates (e->tab.axis): extended behind everything on the device, no synchronisation otherwise
template <typename R>
eea_status ensure_axis(eea_engine* e, unsigned n)
{
  if (n <= e->tab.axis_n) return EEA_OK;
  EEA_HIP(hipDeviceSynchronize());  // kernels of earlier rebuilds may still read the old array
  return e->tab.extend_axis<R>(n, e->cfg.resolution);
}

// The phi_k path's cos tables (e->tab) of the domain (lx, ly) on an nx x ny grid, and d_work for the streaming pass over
// that grid: one launch, reused while grid and domain stay the same.
// Returns through *stale whether the tables have to be (re)computed; the caller that fuses their computation into its own
// launch passes stale != nullptr (and records the key once that launch is enqueued), everybody else gets the separate
// table launch
template <typename R>
eea_status upload_axes_and_tables(eea_engine* e, unsigned nx, unsigned ny, double lx, double ly, hipStream_t s,
                                  bool* stale = nullptr)
{
  if (stale) *stale = false;
  AxisTables& t = e->tab;
  const eea_status st = ensure_axis<R>(e, nx > ny ? nx : ny);
  if (st != EEA_OK) return st;
  const size_t need_cx = sizeof(R) * nx * e->K, need_cy = sizeof(R) * ny * e->K;
  const size_t need_work = sizeof(R) * eea::spatial_work_elems(nx, ny, e->K);
  if (need_cx > t.cx.cap || need_cy > t.cy.cap || need_work > e->d_work.cap) {
    EEA_HIP(hipDeviceSynchronize());  // the buffers about to be replaced may still be in use
    EEA_HIP(t.cx.reserve(need_cx));
    EEA_HIP(t.cy.reserve(need_cy));
    EEA_HIP(e->d_work.reserve(need_work));
    t.forget();
  }
  if (t.holds(nx, ny, lx, ly)) return EEA_OK;
  if (stale) {
    *stale = true;
    return EEA_OK;
  }
  return t.launch<R>(nx, ny, e->K, lx, ly, s);
}

// A row tile is launched with ny = nrows and its tile geometry is recomputed from nrows; the rows-per-tile
// rule is not monotone in ny, so the partials buffer is sized for both the whole grid and the tile
template <typename R>
eea_status reserve_tile_work(eea_engine* e, unsigned nx, unsigned ny_total, unsigned nrows)
{
  size_t elems = eea::spatial_work_elems(nx, ny_total, e->K);
  const size_t tile = eea::spatial_work_elems(nx, nrows, e->K);
  if (tile > elems) elems = tile;
  EEA_HIP(e->d_work.reserve(sizeof(R) * elems));
  return EEA_OK;
}

// orders stream s behind a rebuild that was only enqueued on another stream (no-op once it has completed)
eea_status order_after_rebuild(eea_engine* e, hipStream_t s)
{
  if (!e->rebuild_pending || s == e->rebuild_stream) return EEA_OK;
  if (hipEventQuery(e->ev_rebuild) == hipSuccess) {
    e->rebuild_pending = false;
    return EEA_OK;
  }
  EEA_HIP(hipStreamWaitEvent(s, e->ev_rebuild, 0));
  return EEA_OK;
}
// host-side readers of what a rebuild writes
eea_status finish_rebuild(eea_engine* e)
{
  if (!e->rebuild_pending) return EEA_OK;
  EEA_HIP(hipEventSynchronize(e->ev_rebuild));
  e->rebuild_pending = false;
  return EEA_OK;
}

// eea_records_field: the axis tables of the domain (lx, ly) on an nx x ny grid in the field's own buffers (e->field; the
// caller holds field_mutex).  Unchanged (nx, ny, lx, ly): nothing happens here.  Otherwise one table launch on s, behind
// the last field launch of any stream; a grid larger than the buffers waits for the device before they are replaced (first
// call / change only).
template <typename R>
eea_status field_tables(eea_engine* e, unsigned nx, unsigned ny, double lx, double ly, hipStream_t s)
{
  AxisTables& f = e->field;
  if (f.holds(nx, ny, lx, ly)) return EEA_OK;
  const unsigned n = nx > ny ? nx : ny;
  const size_t need_cx = sizeof(R) * nx * e->K, need_cy = sizeof(R) * ny * e->K;
  const bool grow = n > f.axis_n || need_cx > f.cx.cap || need_cy > f.cy.cap;
  f.forget();  // (a failure below leaves no key on tables that were never written)
  if (grow) EEA_HIP(hipDeviceSynchronize());  // field kernels may still read the buffers about to be replaced
  const eea_status st = f.extend_axis<R>(n, e->cfg.resolution);
  if (st != EEA_OK) return st;
  EEA_HIP(f.cx.reserve(need_cx));
  EEA_HIP(f.cy.reserve(need_cy));
  if (e->ev_field_used == nullptr) {
    EEA_HIP(hipEventCreateWithFlags(&e->ev_field_used, hipEventDisableTiming));
  } else if (!grow) {
    EEA_HIP(hipStreamWaitEvent(s, e->ev_field_used, 0));  // a field launch of another stream may still read the old tables
  }
  return f.launch<R>(nx, ny, e->K, lx, ly, s);
}

template <typename R>
eea_status records_field_impl(eea_engine* e, int kind, unsigned n_rec, const void* d_rec, unsigned nx, unsigned ny_total,
                              unsigned row0, unsigned nrows, void* d_field, hipStream_t s)
{
  std::lock_guard<std::mutex> lock(e->field_mutex);
  const eea_status st = field_tables<R>(e, nx, ny_total, e->lx, e->ly, s);
  if (st != EEA_OK) return st;
  EEA_HIP(eea::launch_records_field<R>(kind, n_rec, as<R>(d_rec), e->K, as<R>(e->d_phik.p), as<R>(e->d_lamdak.p),
                                       as<R>(e->field.cx.p), as<R>(e->field.cy.p), nx, row0, nrows,
                                       static_cast<R>(e->lx * e->ly), as<R>(d_field), s));
  EEA_HIP(hipEventRecord(e->ev_field_used, s));
  return EEA_OK;
}

// Gaussians as Target::fill takes them, [n][4]: the mean translated into the Fourier frame (target.hpp:99) and the
// diagonal of cov_inv = inv(diagmat(sigma^2)) (target.hpp:69; 2x2 inverse), formed in double
std::vector<double> gauss_params(unsigned n, const double* mu, const double* sigma, double trans_x, double trans_y)
{
  std::vector<double> g(static_cast<size_t>(4) * n);
  for (unsigned i = 0; i < n; ++i) {
    const double a = sigma[2 * i] * sigma[2 * i], d = sigma[2 * i + 1] * sigma[2 * i + 1];
    const double det = a * d - 0.0 * 0.0;
    g[4 * i + 0] = mu[2 * i] - trans_x;
    g[4 * i + 1] = mu[2 * i + 1] - trans_y;
    g[4 * i + 2] = d / det;
    g[4 * i + 3] = a / det;
  }
  return g;
}
// ... and by value in the arguments of a launch, cast to its precision (at most kMaxGaussArgs of them)
template <typename R>
eea::GaussArgs<R> gauss_args(const std::vector<double>& g)
{
  eea::GaussArgs<R> ga;
  std::memset(&ga, 0, sizeof(ga));
  ga.n = static_cast<int>(g.size() / 4);
  for (int i = 0; i < ga.n; ++i) {
    for (int c = 0; c < 4; ++c) ga.g[i][c] = static_cast<R>(g[4 * i + c]);
  }
  return ga;
}

// The event the last launch of a rebuild is bound to: the one other streams and the getters wait for when the rebuild is
// only enqueued, none when this call waits itself
eea_status rebuild_event(eea_engine* e, bool wait, hipEvent_t* ev)
{
  *ev = nullptr;
  if (wait) return EEA_OK;
  if (e->ev_rebuild == nullptr) EEA_HIP(hipEventCreateWithFlags(&e->ev_rebuild, hipEventDisableTiming | hipEventDisableSystemFence));
  *ev = e->ev_rebuild;
  return EEA_OK;
}
// ... and behind that launch on s: wait for it, or leave it enqueued -- whatever follows on s is ordered by the stream,
// other streams wait for the event (order_after_rebuild, finish_rebuild).  Then phi_k is the engine's.
eea_status rebuild_issued(eea_engine* e, double lx, double ly, hipStream_t s, bool wait)
{
  if (wait) {
    const eea_status st = wait_stream_spin(e, s);
    if (st != EEA_OK) return st;
    e->rebuild_pending = false;
  } else {
    e->rebuild_stream = s;
    e->rebuild_pending = true;
  }
  commit_phik(e, lx, ly);
  e->have_fill_grid = true;
  e->phi_is_raw = true;
  return EEA_OK;
}

// Target::fill + Basis::spatialCoeff of the Gaussian target on the domain (lx, ly), on the device: one launch from the
// per-axis factors, or three (tables + fill, streaming pass, final sums with the normalisation folded in); ONE host
// synchronisation at the end (wait) or none (enqueue only)
template <typename R>
eea_status rebuild_phik(eea_engine* e, double lx, double ly, hipStream_t s, bool wait)
{
  // the engine's grid / table / phi_k buffers: behind a rebuild still in flight on another stream
  eea_status st = order_after_rebuild(e, s);
  if (st != EEA_OK) return st;
  // Add 1 to include the boundary (ergodic_control.hpp:383-385)
  const unsigned nx = axis_length(0.0, lx, e->cfg.resolution) + 1;
  const unsigned ny = axis_length(0.0, ly, e->cfg.resolution) + 1;
  const size_t P = static_cast<size_t>(nx) * ny;
  if (P == 0 || P > (static_cast<size_t>(1) << 31)) {
    return fail(EEA_ERR_UNSUPPORTED, "target grid size out of range");
  }
  e->nx = nx;
  e->ny = ny;
  const int ng = static_cast<int>(e->mu.size() / 2);
  e->fill_gauss = gauss_params(ng, e->mu.data(), e->sigma.data(), e->map_x, e->map_y);
  hipEvent_t ev = nullptr;
  // A sum of axis-aligned Gaussians on the rectangular grid factors per axis, and so do phi_k and the mass: ONE launch
  // of one workgroup, (nx + ny)(G + K) transcendentals, no grid (gaussian_phik_kernel).  The grid itself is filled only
  // when eea_get_target_grid asks for it.  EEA_OPT_REBUILD_IMPL = 1 forces the streaming form below (A/B, tests).
  if (ng >= 1 && ng <= eea::kMaxGaussArgs && eea::option(EEA_OPT_REBUILD_IMPL) != 1 &&
      eea::gaussian_phik_lds_bytes(nx, ny, ng, e->K, sizeof(R)) <= 160 * 1024) {
    st = ensure_axis<R>(e, nx > ny ? nx : ny);
    if (st != EEA_OK) return st;
    if (e->d_sum.cap < sizeof(R)) {
      EEA_HIP(hipDeviceSynchronize());
      EEA_HIP(e->d_sum.reserve(sizeof(R) * 64));
    }
    st = rebuild_event(e, wait, &ev);
    if (st != EEA_OK) return st;
    EEA_HIP(eea::launch_gaussian_phik<R>(as<R>(e->tab.axis.p), nx, ny, gauss_args<R>(e->fill_gauss), e->K,
                                         static_cast<R>(1.0 / lx), static_cast<R>(1.0 / ly), as<R>(e->d_phik.p),
                                         as<R>(e->d_sum.p), s, ev));
    st = rebuild_issued(e, lx, ly, s, wait);
    if (st == EEA_OK) e->fill_deferred = true;
    return st;
  }
  e->fill_deferred = false;
  const bool by_args = ng <= eea::kMaxGaussArgs;  // the Gaussians fit the kernel arguments
  bool tables_stale = false;
  st = upload_axes_and_tables<R>(e, nx, ny, lx, ly, s, by_args ? &tables_stale : nullptr);
  if (st != EEA_OK) return st;
  const size_t need_phi = sizeof(R) * P;
  const int fill_blocks_args = eea::target_fill_blocks(P);
  const int fill_blocks_buf = static_cast<int>((P + eea::kBlock - 1) / eea::kBlock);
  const size_t need_sum = sizeof(R) * (static_cast<size_t>(by_args ? fill_blocks_args : fill_blocks_buf) + 1);
  if (need_phi > e->d_phi.cap || need_sum > e->d_sum.cap) {
    EEA_HIP(hipDeviceSynchronize());
    EEA_HIP(e->d_phi.reserve(need_phi));
    EEA_HIP(e->d_sum.reserve(need_sum));
  }
  AxisTables& t = e->tab;
  R* const d_mass = as<R>(e->d_sum.p);
  R* const d_partials = d_mass + 1;
  int n_partials = 0;
  if (by_args) {
    n_partials = fill_blocks_args;
    // the fill and (when the domain changed) the two axis tables in ONE launch
    EEA_HIP(eea::launch_target_fill_args<R>(as<R>(t.axis.p), nx, ny, gauss_args<R>(e->fill_gauss), as<R>(e->d_phi.p),
                                            d_partials, e->K, static_cast<R>(eea::kPi / lx), static_cast<R>(eea::kPi / ly),
                                            tables_stale ? as<R>(t.cx.p) : nullptr, as<R>(t.cy.p), s));
    if (tables_stale) t.remember(nx, ny, lx, ly);
  } else {
    // more Gaussians than the kernel arguments hold: parameters through a device buffer (one more sync)
    const std::vector<R> g(e->fill_gauss.begin(), e->fill_gauss.end());
    EEA_HIP(e->d_gauss.reserve(sizeof(R) * g.size()));
    EEA_HIP(hipMemcpyAsync(e->d_gauss.p, g.data(), sizeof(R) * g.size(), hipMemcpyHostToDevice, s));
    EEA_HIP(hipStreamSynchronize(s));
    EEA_HIP(eea::launch_target_fill<R>(as<R>(t.axis.p), as<R>(t.axis.p), nx, ny, as<R>(e->d_gauss.p), ng, as<R>(e->d_phi.p),
                                       d_partials, &n_partials, s));
  }
  // phi_k = spatialCoeff(phi / sum(phi)) = spatialCoeff(phi) / sum(phi)  (target.cpp:87, basis.cpp:122-133)
  // enqueue-only form: the event other streams (and the getters) wait for is bound to the last launch itself
  st = rebuild_event(e, wait, &ev);
  if (st != EEA_OK) return st;
  EEA_HIP(eea::launch_spatial_coeff_normalised<R>(as<R>(e->d_phi.p), nx, ny, e->K, as<R>(t.cx.p), as<R>(t.cy.p),
                                                  as<R>(e->d_work.p), as<R>(e->d_phik.p), d_partials, n_partials, d_mass, s,
                                                  ev));
  return rebuild_issued(e, lx, ly, s, wait);
}

// Target::fill of the last Gaussian rebuild on demand (eea_get_target_grid): the un-normalised grid into d_phi; d_sum[0]
// keeps the mass the rebuild computed from the per-axis factors
template <typename R>
eea_status fill_deferred_grid(eea_engine* e)
{
  const unsigned nx = e->nx, ny = e->ny;
  const size_t P = static_cast<size_t>(nx) * ny;
  EEA_HIP(hipDeviceSynchronize());
  EEA_HIP(e->d_phi.reserve(sizeof(R) * P));
  DevBuf partials;  // (the fill's per-workgroup sums are not needed: the mass is already known)
  EEA_HIP(partials.reserve(sizeof(R) * (static_cast<size_t>(eea::target_fill_blocks(P)) + 1)));
  EEA_HIP(eea::launch_target_fill_args<R>(as<R>(e->tab.axis.p), nx, ny, gauss_args<R>(e->fill_gauss), as<R>(e->d_phi.p),
                                          as<R>(partials.p), e->K, R(0), R(0), nullptr, nullptr, nullptr));
  EEA_HIP(hipDeviceSynchronize());  // (partials goes only behind the launch)
  e->fill_deferred = false;
  return EEA_OK;
}

template <typename R>
eea_status set_target_grid_impl(eea_engine* e, unsigned nx, unsigned ny, const void* phi_vals, int on_device, double lx,
                                double ly, hipStream_t s)
{
  const size_t P = static_cast<size_t>(nx) * ny;
  e->nx = nx;
  e->ny = ny;
  e->have_fill_grid = false;
  const eea_status st = upload_axes_and_tables<R>(e, nx, ny, lx, ly, s);
  if (st != EEA_OK) return st;
  const R* d_phi = as<R>(phi_vals);
  if (!on_device) {
    EEA_HIP(e->d_phi.reserve(sizeof(R) * P));
    EEA_HIP(hipMemcpyAsync(e->d_phi.p, phi_vals, sizeof(R) * P, hipMemcpyHostToDevice, s));
    EEA_HIP(hipStreamSynchronize(s));
    d_phi = as<R>(e->d_phi.p);
  }
  EEA_HIP(eea::launch_spatial_coeff<R>(d_phi, nx, ny, e->K, as<R>(e->tab.cx.p), as<R>(e->tab.cy.p), as<R>(e->d_work.p),
                                       as<R>(e->d_phik.p), s));
  EEA_HIP(hipStreamSynchronize(s));
  commit_phik(e, lx, ly);
  return EEA_OK;
}

template <typename R>
void fill_params(const eea_engine* e, eea::ControlParams<R>& p)
{
  std::memset(&p, 0, sizeof(p));
  p.T = e->T;
  p.K = e->K;
  p.chunk = e->chunk;
  p.dt = static_cast<R>(e->cfg.dt);
  p.dt6 = static_cast<R>(e->cfg.dt / 6.0);
  p.half_dt = static_cast<R>(0.5 * e->cfg.dt);
  p.lx = static_cast<R>(e->lx);
  p.ly = static_cast<R>(e->ly);
  p.map_x = static_cast<R>(e->map_x);
  p.map_y = static_cast<R>(e->map_y);
  p.expl_weight = static_cast<R>(e->cfg.expl_weight);
  p.pi_lx = static_cast<R>(eea::kPi / e->lx);
  p.pi_ly = static_cast<R>(eea::kPi / e->ly);
  p.inv_lx = static_cast<R>(1.0 / e->lx);
  p.inv_ly = static_cast<R>(1.0 / e->ly);
  for (int i = 0; i < 9; ++i) p.Rinv[i] = static_cast<R>(e->cfg.Rinv[i]);
  for (int i = 0; i < 3; ++i) {
    p.umin[i] = static_cast<R>(e->cfg.umin[i]);
    p.umax[i] = static_cast<R>(e->cfg.umax[i]);
  }
  p.phik = static_cast<const R*>(e->d_phik.p);
  p.lamdak = static_cast<const R*>(e->d_lamdak.p);
  p.n_steps = 1;
}

// workspace of the sum written to `key` for up to B records.  One per distinct output buffer (concurrent sums on
// several streams must not share tickets), found under the engine's lock (the header allows concurrent calls with
// distinct d_sum buffers); at most kMaxSumWs of them -- a caller that passes a fresh output buffer every call recycles
// the least recently used workspace instead of growing the list.  The tickets are zeroed on the launch stream.
constexpr size_t kMaxSumWs = 32;
// (the caller holds e->sum_mutex, and keeps it across its launch: a second thread that misses with every workspace in use
// must not recycle this one between the lookup and the launch)
template <typename R>
eea_status sum_workspace(eea_engine* e, const void* key, unsigned B, hipStream_t s, eea_engine::SumWs** out)
{
  eea_engine::SumWs* w = nullptr;
  for (auto& cand : e->sum_ws) {
    if (cand->key == key) w = cand.get();
  }
  bool recycled = false;
  if (w == nullptr) {
    if (e->sum_ws.size() < kMaxSumWs) {
      e->sum_ws.emplace_back(new eea_engine::SumWs());
      w = e->sum_ws.back().get();
    } else {  // least recently used
      w = e->sum_ws.front().get();
      for (auto& cand : e->sum_ws) {
        if (cand->last_use < w->last_use) w = cand.get();
      }
      recycled = true;
    }
    w->key = key;
  }
  w->last_use = ++e->sum_clock;
  const size_t need_ws = sizeof(R) * eea::ck_sum_ws_elems(B, e->K2);
  const size_t need_ctr = sizeof(unsigned) * eea::ck_sum_tickets(B, e->K2);
  if (need_ws > w->ws.cap || need_ctr > w->ctr.cap || recycled) {
    // NO device synchronisation here (a per-pass call must not stall every stream of the device): buffers an
    // earlier launch may still use are retired behind an event on that launch's stream and freed once it has completed
    // (no device-wide sweep); a recycled workspace gets fresh buffers for the same reason.
    for (size_t i = 0; i < e->retired.size();) {
      if (e->retired[i].done != nullptr && hipEventQuery(e->retired[i].done) == hipSuccess) {
        (void)hipEventDestroy(e->retired[i].done);
        (void)hipFree(e->retired[i].p);
        e->retired[i] = e->retired.back();
        e->retired.pop_back();
      } else {
        ++i;
      }
    }
    (void)hipGetLastError();  // (hipErrorNotReady of the queries is not an error of this call)
    // Each buffer moves to the retired list individually, and the workspace forgets it the moment it has (a failed
    // record must neither leak the event nor leave w->ws.p pointing at a buffer the list will free).  last_stream is a
    // CALLER-owned handle remembered from an earlier call: if the caller has destroyed it the record fails -- the event is
    // destroyed and the buffer stays in the list without one, until eea_destroy (its last launch cannot be proven complete).
    for (DevBuf* buf : { &w->ws, &w->ctr }) {
      if (buf->p == nullptr) continue;
      hipEvent_t ev = nullptr;
      if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) ev = nullptr;
      if (ev != nullptr && hipEventRecord(ev, w->last_stream) != hipSuccess) {
        (void)hipEventDestroy(ev);
        ev = nullptr;
      }
      (void)hipGetLastError();
      e->retired.push_back({ buf->p, ev });
      (void)buf->detach();  // (ownership moved to the retired list)
    }
    EEA_HIP(w->ws.reserve(need_ws));
    EEA_HIP(w->ctr.reserve(need_ctr));
    EEA_HIP(hipMemsetAsync(w->ctr.p, 0, w->ctr.cap, s));  // the tickets reset themselves from here on
  }
  w->last_stream = s;
  *out = w;
  return EEA_OK;
}

// The kernel that runs a control call of B agents with these parameters (eea::ControlForm): the one place that reads
// EEA_OPT_CONTROL_KERNEL and EEA_OPT_AGENT_LANES.  Three kernels ship: one wavefront per agent (horizons <= 256 steps,
// K <= 16 or K = 20), several agents per wavefront (fp64 short horizons, when the batch still fills the chip) and one
// workgroup per agent (everything else).  Batches take the wavefront kernels unless EEA_OPT_CONTROL_KERNEL says otherwise.
// The single-agent call (eea_control and its resident form: one agent, latency) takes the wavefront for horizons of one
// slot (T <= 64: one step per lane, no barrier -- 3.0 / 4.9 / 4.3 us of device time at configs[0] / configs[1] / the yaml's
// T = 50 against 5.1 / 7.4 / 5.2 of the workgroup) and keeps four wavefronts per agent beyond (T = 200: 7.2 against 11.6 us;
// profiles/r05_one_agent_kernels.txt)
template <typename R>
eea::ControlForm control_form(const eea::ControlParams<R>& p, unsigned B, bool single_agent)
{
  if (eea::option(EEA_OPT_CONTROL_KERNEL) != 0) return { 0 };
  if ((single_agent && p.T > 64) || !eea::control_wave_eligible<R>(p)) return { 0 };
  if constexpr (sizeof(R) == 8) {
    const int lanes = eea::control_pack_lanes(p, B, eea::option(EEA_OPT_AGENT_LANES));
    if (lanes != 0) return { lanes };
  }
  return { 64 };
}

// the form of a batch call of B agents on this engine (eea_batch_agent_lanes, eea_batch_record_count)
eea::ControlForm batch_form(const eea_engine* e, unsigned B)
{
  return by_precision(e, [&](auto r) {
    eea::ControlParams<decltype(r)> p;
    fill_params(e, p);
    return control_form(p, B, false);
  });
}

// One control launch of B agents in the form control_form picks, reported in *form when not null.  done: the single-agent
// call's completion word (eea_control), null for batches.
template <typename R>
eea_status control_batch_impl(eea_engine* e, unsigned B, const eea_batch_io* io, bool rollout_only, hipStream_t s,
                              eea::ControlForm* form = nullptr, int* done = nullptr, long long* d_stamps = nullptr,
                              unsigned n_steps = 1, unsigned pose_step_stride = 0, unsigned u0_step_stride = 0)
{
  eea::ControlParams<R> p;
  fill_params<R>(e, p);
  p.n_steps = static_cast<int>(n_steps);
  p.pose_step_stride = pose_step_stride;
  p.u0_step_stride = u0_step_stride;
  p.pose = static_cast<const R*>(io->d_pose);
  p.ut = static_cast<R*>(io->d_ut);
  p.mem_cols = static_cast<const R*>(io->d_mem_cols);
  p.n_mem = io->d_n_mem;
  p.mem_stride = io->d_mem_cols ? io->mem_stride : 0u;
  p.u0 = static_cast<R*>(io->d_u0);
  p.traj = static_cast<R*>(io->d_traj);
  p.ck = static_cast<R*>(io->d_ck);
  p.ck_shared = static_cast<const R*>(io->d_ck_shared);
  p.ck_shared_parts = io->d_ck_shared != nullptr ? static_cast<int>(io->ck_shared_parts) : 0;
  p.rec_len = eea::ck_record_len(e->K2);
  p.rec_ready = rollout_only ? nullptr : io->d_rec_ready;
  p.rec_wave = io->rec_per_wavefront != 0 ? 1 : 0;
  p.rec_seq = io->rec_seq;
  p.ck_flag = io->d_ck_shared != nullptr ? io->d_ck_flag : nullptr;
  p.ck_flag_seq = io->ck_flag_seq;
  p.edx = static_cast<R*>(io->d_edx);
  p.bdx = static_cast<R*>(io->d_bdx);
  p.rhot = static_cast<R*>(io->d_rhot);
  p.status = io->d_status;
  p.skip = io->d_skip;
  p.done = done;
  p.done_seq = e->mail_seq;
  const int n_mem_max = rollout_only ? 0 : static_cast<int>(p.mem_stride);
  p.dbg = d_stamps;  // phase stamps: null in the product (only the A/B library's kernels read it, tools/ab/)
  p.ck_rec = rollout_only ? nullptr : static_cast<R*>(io->d_ck_rec);
  const eea::ControlForm f = control_form<R>(p, B, done != nullptr);
  if (form != nullptr) *form = f;
  if constexpr (sizeof(R) == 8) {
    if (f.lanes != 0 && f.lanes < 64) {
      EEA_HIP(eea::launch_control_pack(p, B, e->cfg.model, rollout_only, f.lanes, s));
      return EEA_OK;
    }
  }
  if (f.lanes == 64) {
    EEA_HIP(eea::launch_control_wave<R>(p, B, e->cfg.model, rollout_only, s));
    return EEA_OK;
  }
  const size_t lds = eea::control_lds_bytes<R>(p.T, p.K, n_mem_max, p.chunk);
  if (lds > 160 * 1024) {
    return fail(EEA_ERR_UNSUPPORTED, "horizon/memory/basis too large for one workgroup's 160 KiB LDS");
  }
  // the workgroup-per-agent kernel takes one step per launch: a multi-step call is that many launches on the stream
  p.n_steps = 1;
  for (unsigned n = 0; n < n_steps; ++n) {
    p.pose = static_cast<const R*>(io->d_pose) + 3 * static_cast<size_t>(n) * pose_step_stride;
    p.u0 = static_cast<R*>(io->d_u0) + 3 * static_cast<size_t>(n) * u0_step_stride;
    EEA_HIP(eea::launch_control<R>(p, B, e->cfg.model, n_mem_max, rollout_only, s));
  }
  return EEA_OK;
}

// numerics.hpp:164-179 of the reference: information entropy of one occupancy cell, p = cell / 100
// (unknown cells, p < 0, count 0.7; p == 0 or 1 count 1e-3)
double cell_entropy(double p)
{
  if (std::fabs(0.0 - p) < 1.0e-12 || std::fabs(1.0 - p) < 1.0e-12) return 1e-3;
  if (p < 0.0) return 0.7;
  return -p * std::log(p) - (1.0 - p) * std::log(1.0 - p);
}

// decode table of the occupancy path, indexed by the cell's byte (int8 two's complement)
template <typename R>
eea_status upload_entropy_table(eea_engine* e, hipStream_t s)
{
  std::vector<R> lut(256);
  for (int b = 0; b < 256; ++b) {
    const int cell = static_cast<int>(static_cast<int8_t>(static_cast<uint8_t>(b)));
    lut[b] = static_cast<R>(cell_entropy(static_cast<double>(cell) / 100.0));  // getCell: grid.cpp:176-184
  }
  EEA_HIP(e->d_raw.reserve(sizeof(R) * e->K2));
  if (e->have_lut) return EEA_OK;
  EEA_HIP(e->d_lut.reserve(sizeof(R) * 256));
  EEA_HIP(hipMemcpyAsync(e->d_lut.p, lut.data(), sizeof(R) * 256, hipMemcpyHostToDevice, s));
  EEA_HIP(hipStreamSynchronize(s));
  e->have_lut = true;
  return EEA_OK;
}

// un-normalised coefficient sums of rows [row0, row0 + nrows) of an occupancy grid on the domain (lx, ly)
template <typename R>
eea_status occupancy_rows_impl(eea_engine* e, unsigned nx, unsigned ny_total, unsigned row0, unsigned nrows, double lx,
                               double ly, const int8_t* d_occ_rows, void* d_raw_out, hipStream_t s,
                               void* d_mass_out = nullptr)
{
  eea_status st = upload_axes_and_tables<R>(e, nx, ny_total, lx, ly, s);
  if (st != EEA_OK) return st;
  st = upload_entropy_table<R>(e, s);
  if (st != EEA_OK) return st;
  st = reserve_tile_work<R>(e, nx, ny_total, nrows);
  if (st != EEA_OK) return st;
  EEA_HIP(eea::launch_spatial_coeff_cells<R>(d_occ_rows, nx, nrows, e->K, as<R>(e->tab.cx.p),
                                             as<R>(e->tab.cy.p) + static_cast<size_t>(row0) * e->K, as<R>(e->d_lut.p),
                                             as<R>(e->d_work.p), as<R>(d_raw_out), s, as<R>(d_mass_out)));
  return EEA_OK;
}

// ---- resident single-robot workgroup (control_kernel_impl.hpp control_resident_kernel) --------------------------------------
// idle time of a resident workgroup in ticks of the constant 100 MHz clock (EEA_OPT_RESIDENT_IDLE_MS, default 250 ms: a 10 Hz
// loop keeps it alive)
long long resident_idle_ticks() { return 100000LL * static_cast<long long>(eea::option(EEA_OPT_RESIDENT_IDLE_MS)); }

// tells the workgroup to leave and waits until it has (no-op when none was launched)
eea_status resident_stop(eea_engine* e)
{
  if (!e->res_launched) return EEA_OK;
  // (the two mailbox layouts differ only in the width of the reals in front of cmd / req: go through the right one)
  if (e->f32) {
    auto* m = static_cast<eea::ResidentMail<float>*>(e->h_rmail);
    __atomic_store_n(&m->cmd, 1, __ATOMIC_RELAXED);
    __atomic_store_n(&m->req, ++e->res_seq, __ATOMIC_RELEASE);
  } else {
    auto* m = static_cast<eea::ResidentMail<double>*>(e->h_rmail);
    __atomic_store_n(&m->cmd, 1, __ATOMIC_RELAXED);
    __atomic_store_n(&m->req, ++e->res_seq, __ATOMIC_RELEASE);
  }
  EEA_HIP(hipStreamSynchronize(e->stream_res));  // it leaves within microseconds (or has left already: idle)
  if (e->f32) static_cast<eea::ResidentMail<float>*>(e->h_rmail)->cmd = 0;
  else static_cast<eea::ResidentMail<double>*>(e->h_rmail)->cmd = 0;
  e->res_launched = false;
  return EEA_OK;
}

template <typename R>
eea_status resident_start(eea_engine* e)
{
  using Mail = eea::ResidentMail<R>;
  if (e->h_rmail == nullptr) {
    EEA_HIP(hipHostMalloc(&e->h_rmail, sizeof(Mail), hipHostMallocMapped));
    std::memset(e->h_rmail, 0, sizeof(Mail));
    EEA_HIP(hipHostGetDevicePointer(&e->d_rmail, e->h_rmail, 0));
    EEA_HIP(hipHostMalloc(&e->h_rmem, sizeof(R) * 3 * eea::kResidentMemCols, hipHostMallocMapped));
    std::memset(e->h_rmem, 0, sizeof(R) * 3 * eea::kResidentMemCols);
    EEA_HIP(hipHostGetDevicePointer(&e->d_rmem, e->h_rmem, 0));
    EEA_HIP(hipStreamCreateWithFlags(&e->stream_res, hipStreamNonBlocking));
    EEA_HIP(e->d_rstage.reserve(sizeof(eea::ResidentStage<R>)));
  }
  EEA_HIP(hipStreamSynchronize(e->stream_res));  // (an earlier workgroup that left by itself has completed)
  eea_status st = finish_rebuild(e);             // phi_k of an enqueued rebuild is complete before the workgroup reads it
  if (st != EEA_OK) return st;
  EEA_HIP(hipStreamSynchronize(e->stream1));     // ... and so is everything else the launch path left behind (d_ut1)
  Mail* const hm = static_cast<Mail*>(e->h_rmail);
  Mail* const dm = static_cast<Mail*>(e->d_rmail);
  eea::ControlParams<R> p;
  fill_params<R>(e, p);
  p.pose = dm->pose;   // (the workgroup points these two at its device-memory stage per request)
  p.n_mem = &dm->n_mem;
  p.ut = static_cast<R*>(e->d_ut1.p);
  p.u0 = dm->u0;
  p.status = &dm->status;
  p.mem_cols = static_cast<const R*>(e->d_rmem);
  p.mem_stride = static_cast<unsigned>(eea::kResidentMemCols);
  p.rec_len = eea::ck_record_len(e->K2);
  p.done = &dm->done;  // (the workgroup announces the answer itself and ignores it)
  // fp64 horizons of one slot: ONE wavefront (the kernel the launch path takes at these shapes), otherwise the workgroup
  bool one_wavefront = false;
  if constexpr (sizeof(R) == 8) one_wavefront = control_form<R>(p, 1, true).lanes == 64 && eea::control_wave_resident_eligible(p);
  const size_t lds = eea::control_lds_bytes<R>(p.T, p.K, eea::kResidentMemCols, p.chunk);
  if (!one_wavefront && lds > 160 * 1024) return EEA_ERR_UNSUPPORTED;  // (no message: the caller takes the launch path)
  hm->alive = 1;
  hm->cmd = 0;
  __atomic_thread_fence(__ATOMIC_SEQ_CST);
  if constexpr (sizeof(R) == 8) {
    if (one_wavefront) {
      p.res_mail = e->d_rmail;
      p.res_first = e->res_seq;
      p.res_idle = resident_idle_ticks();
      EEA_HIP(eea::launch_control_wave_resident(p, e->cfg.model, e->stream_res));
    }
  }
  if (!one_wavefront) {
    EEA_HIP(eea::launch_control_resident<R>(p, e->cfg.model, eea::kResidentMemCols, e->d_rmail, e->d_rstage.p, e->res_seq,
                                            resident_idle_ticks(), e->stream_res));
  }
  e->res_one_wavefront = one_wavefront;
  e->res_launched = true;
  e->res_gen = e->phik_gen;
  return EEA_OK;
}

// eea_control through the resident workgroup: post the request in the mailbox, poll the answer
template <typename R>
eea_status control_resident(eea_engine* e, const double x[3], const double* h_mem_cols, unsigned n_mem, double u_out[3])
{
  using Mail = eea::ResidentMail<R>;
  eea_status st = EEA_OK;
  if (e->res_launched && e->res_gen != e->phik_gen) {  // the domain / phi_k changed: the launch parameters are stale
    st = resident_stop(e);
    if (st != EEA_OK) return st;
  }
  Mail* hm = static_cast<Mail*>(e->h_rmail);
  if (!e->res_launched || __atomic_load_n(&hm->alive, __ATOMIC_ACQUIRE) == 0) {
    e->res_launched = false;
    st = resident_start<R>(e);
    if (st != EEA_OK) return st;
    hm = static_cast<Mail*>(e->h_rmail);
  }
  to_real<R>(x, hm->pose, 3);
  hm->map_x = static_cast<R>(e->map_x);
  hm->map_y = static_cast<R>(e->map_y);
  hm->n_mem = static_cast<int>(n_mem);
  if (n_mem > 0) to_real<R>(h_mem_cols, static_cast<R*>(e->h_rmem), 3 * static_cast<size_t>(n_mem));
  hm->status = 0;
  const unsigned seq = ++e->res_seq;
  __atomic_store_n(&hm->req, seq, __ATOMIC_RELEASE);
  // the answer (bounded: ~2 s of polling), or the news that the workgroup left before it saw the request
  bool relaunched = false;
  for (long spin = 0;; ++spin) {
    if (__atomic_load_n(&hm->done, __ATOMIC_ACQUIRE) == static_cast<int>(seq)) break;
    if (__atomic_load_n(&hm->alive, __ATOMIC_ACQUIRE) == 0 &&
        __atomic_load_n(&hm->done, __ATOMIC_ACQUIRE) != static_cast<int>(seq)) {
      if (relaunched) return fail(EEA_ERR_HIP, "the resident control workgroup left twice without answering");
      // It announced that it is leaving around the time of this request.  It may still be SERVING it (a request that lands
      // between "alive = 0" and its last look at the mailbox is served, and then it leaves -- it never polls again): wait
      // until it has left, then look at the answer once more.  Only a request that is still unanswered then gets a new
      // workgroup, which starts from the request before this one and sees it at once.  (Relaunching without this wait served
      // such a request twice: the warm start shifted twice, u0 rewritten under the host's read -- ADVICE r05.)
      EEA_HIP(hipStreamSynchronize(e->stream_res));
      if (__atomic_load_n(&hm->done, __ATOMIC_ACQUIRE) == static_cast<int>(seq)) {
        e->res_launched = false;  // answered by the leaving workgroup; the next call starts another one
        break;
      }
      e->res_launched = false;
      --e->res_seq;
      st = resident_start<R>(e);
      ++e->res_seq;
      if (st != EEA_OK) return st;
      relaunched = true;
    }
    if (spin > 400000000L) return fail(EEA_ERR_TIMEOUT, "the resident control workgroup does not answer");
  }
  if (hm->status == EEA_ERR_INVALID_TWIST) return fail(EEA_ERR_INVALID_TWIST, "Invalid twist y-velocity must be 0.");
  for (int i = 0; i < 3; ++i) u_out[i] = static_cast<double>(hm->u0[i]);
  return EEA_OK;
}

// Prologue of the entries that launch on the engine: refuses a null engine, then the call's own arguments (bad_args: what is
// wrong with them, null when nothing is), then selects the engine's device.
eea_status enter_launch(const eea_engine* e, const char* bad_args = nullptr)
{
  if (e == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null engine");
  if (bad_args != nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, bad_args);
  return use_device(e);
}

// Prologue of the entries that write the engine's grid / table / phi_k buffers: the same, but a rebuild that was only
// enqueued owns those buffers and is waited for first (a failed wait is reported before the arguments are).
eea_status enter_target(eea_engine* e, const char* bad_args)
{
  if (e == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null engine");
  if (finish_rebuild(e) != EEA_OK) return EEA_ERR_HIP;
  return enter_launch(e, bad_args);
}
}  // namespace

eea_status eea::control_batch(eea_engine* e, unsigned B, const eea_batch_io* io, void* stream, ControlForm* form,
                              unsigned n_steps, unsigned pose_step_stride, unsigned u0_step_stride)
{
  // (its refusals are of three kinds, in this order, and all come before the device is touched: no shared prologue)
  if (e == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null engine");
  if (io == nullptr || io->d_pose == nullptr || io->d_ut == nullptr || io->d_u0 == nullptr) {
    return fail(EEA_ERR_INVALID_ARGUMENT, "d_pose, d_ut and d_u0 are required");
  }
  if (n_steps == 0 || n_steps > (1u << 20)) return fail(EEA_ERR_INVALID_ARGUMENT, "n_steps must be in 1 .. 2^20");
  if ((pose_step_stride != 0 && pose_step_stride < B) || (u0_step_stride != 0 && u0_step_stride < B)) {
    return fail(EEA_ERR_INVALID_ARGUMENT, "a step stride is 0 (the same row every step) or >= B agents");
  }
  if (n_steps > 1 && (io->d_rec_ready != nullptr || io->d_ck_flag != nullptr)) {
    // a step of the launch would wait, inside the kernel, for an exchange the host can only enqueue after this call: that
    // needs truly concurrent hardware queues (streams may share one) -- the device-bound exchange is one step per launch
    return fail(EEA_ERR_UNSUPPORTED, "the device-bound exchange (d_rec_ready / d_ck_flag) takes one step per launch");
  }
  if (!e->have_phik) return fail(EEA_ERR_NO_TARGET, "no phi_k: call eea_config_domain or eea_set_target_grid first");
  hipStream_t s = static_cast<hipStream_t>(stream);
  // the device, and behind a phi_k rebuild that was only enqueued on another stream (eea_config_domain_async)
  const eea_status st = engine_enter(e, s);
  if (st != EEA_OK) return st;
  return by_precision(e, [&](auto r) {
    return control_batch_impl<decltype(r)>(e, B, io, false, s, form, nullptr, nullptr, n_steps, pose_step_stride, u0_step_stride);
  });
}

void eea::engine_view(const eea_engine* e, EngineView* v)
{
  v->device = e->cfg.device;
  v->K = e->K;
  v->f32 = e->f32;
  v->have_phik = e->have_phik;
  v->lx = e->lx;
  v->ly = e->ly;
  v->map_x = e->map_x;
  v->map_y = e->map_y;
  v->d_phik = e->d_phik.p;
  v->d_lamdak = e->d_lamdak.p;
}

eea_status eea::engine_enter(eea_engine* e, hipStream_t s)
{
  const eea_status st = use_device(e);
  return st != EEA_OK ? st : order_after_rebuild(e, s);
}

extern "C" {

const char* eea_last_error(void) { return eea::g_last_error.c_str(); }

eea_status eea_set_option(int option, int value)
{
  bool ok = false;
  switch (option) {
    case EEA_OPT_CONTROL_KERNEL: ok = value == 0 || value == 1; break;
    case EEA_OPT_WORKGROUP_THREADS: ok = value == 0 || value == 64 || value == 128 || value == 256; break;
    case EEA_OPT_COLLISION_IMPL: ok = value >= 0 && value <= 2; break;
    case EEA_OPT_MAILBOX_POLL: ok = value == 0 || value == 1; break;
    case EEA_OPT_REBUILD_IMPL: ok = value == 0 || value == 1; break;
    case EEA_OPT_AGENT_LANES: ok = value == 0 || value == 8 || value == 16 || value == 32 || value == 64; break;
    case EEA_OPT_RESIDENT_CONTROL: ok = value == 0 || value == 1; break;
    case EEA_OPT_RESIDENT_IDLE_MS: ok = value >= 1 && value <= 60000; break;
    default: return fail(EEA_ERR_INVALID_ARGUMENT, "unknown option");
  }
  if (!ok) return fail(EEA_ERR_INVALID_ARGUMENT, "option value out of range");
  g_options[option].store(value, std::memory_order_relaxed);
  return EEA_OK;
}
int eea_get_option(int option) { return eea::option(option); }
unsigned eea_abi_version(void) { return EEA_ABI_VERSION; }

eea_status eea_create(const eea_config* cfg, eea_engine** out)
{
  if (cfg == nullptr || out == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  *out = nullptr;
  if (cfg->model != EEA_MODEL_OMNI && cfg->model != EEA_MODEL_SIMPLE_CART) {
    return fail(EEA_ERR_INVALID_ARGUMENT,
                "model must be Omni or SimpleCart (Cart/Mecanum cannot run under ErgodicControl)");
  }
  if (cfg->precision != EEA_PREC_F64 && cfg->precision != EEA_PREC_F32) {
    return fail(EEA_ERR_INVALID_ARGUMENT, "unknown precision");
  }
  // steps_ = static_cast<unsigned>(std::abs(horizon / dt))  (ergodic_control.hpp:199)
  const double ratio = std::abs(cfg->horizon / cfg->dt);
  if (!(ratio < 1.0e6)) return fail(EEA_ERR_INVALID_ARGUMENT, "horizon / dt out of range");
  const unsigned steps = static_cast<unsigned>(ratio);
  if (steps == 1) {
    return fail(EEA_ERR_INVALID_ARGUMENT,
                "Need at least two steps in forward simulation. Increase the horizon or decrease "
                "the time step.");
  }
  if (steps == 0) return fail(EEA_ERR_INVALID_ARGUMENT, "horizon shorter than one time step");
  if (cfg->num_basis == 0 || cfg->num_basis > static_cast<unsigned>(eea::kMaxBasis)) {
    return fail(EEA_ERR_UNSUPPORTED, "num_basis must be in [1, 32]");
  }
  int ndev = 0;
  EEA_HIP(hipGetDeviceCount(&ndev));
  if (cfg->device < 0 || cfg->device >= ndev) return fail(EEA_ERR_HIP, "no such HIP device");
  EEA_HIP(hipSetDevice(cfg->device));

  eea_engine* e = new eea_engine();
  e->cfg = *cfg;
  e->T = static_cast<int>(steps);
  e->K = static_cast<int>(cfg->num_basis);
  e->K2 = e->K * e->K;
  e->f32 = cfg->precision == EEA_PREC_F32;
  e->rs = e->f32 ? 4 : 8;
  const eea_status st = by_precision(e, [&](auto r) { return upload_lamdak<decltype(r)>(e); });
  if (st != EEA_OK) {
    eea_destroy(e);
    return st;
  }
  hipError_t err = hipStreamCreateWithFlags(&e->stream1, hipStreamNonBlocking);
  if (err == hipSuccess) {
    err = hipHostMalloc(reinterpret_cast<void**>(&e->h_mail), sizeof(Mailbox),
                        hipHostMallocMapped | hipHostMallocCoherent);
  }
  if (err == hipSuccess) {
    std::memset(e->h_mail, 0, sizeof(Mailbox));
    err = hipHostGetDevicePointer(&e->d_mail, e->h_mail, 0);
  }
  if (err == hipSuccess) err = e->d_ut1.reserve(e->rs * 3 * e->T);
  if (err == hipSuccess) err = hipMemset(e->d_ut1.p, 0, e->rs * 3 * e->T);  // ut_ starts at zero (:201)
  if (err == hipSuccess) err = e->d_traj1.reserve(e->rs * 3 * e->T);
  if (err != hipSuccess) {
    const std::string msg = std::string("engine allocation: ") + hipGetErrorString(err);
    eea_destroy(e);
    return fail(EEA_ERR_HIP, msg);
  }
  *out = e;
  return EEA_OK;
}

void eea_destroy(eea_engine* e)
{
  if (e == nullptr) return;
  (void)hipSetDevice(e->cfg.device);
  (void)resident_stop(e);  // the resident single-robot workgroup leaves before anything it reads is freed
  (void)finish_rebuild(e);
  if (e->stream1) {
    (void)hipStreamSynchronize(e->stream1);
    (void)hipStreamDestroy(e->stream1);
  }
  if (e->ev_field_used) (void)hipEventDestroy(e->ev_field_used);
  for (auto& r : e->retired) {
    if (r.done != nullptr) (void)hipEventDestroy(r.done);
    (void)hipFree(r.p);
  }
  if (e->ev_done) (void)hipEventDestroy(e->ev_done);
  if (e->ev_rebuild) (void)hipEventDestroy(e->ev_rebuild);
  if (e->h_mail) (void)hipHostFree(e->h_mail);
  if (e->h_stage) (void)hipHostFree(e->h_stage);
  if (e->h_rmail) (void)hipHostFree(e->h_rmail);
  if (e->h_rmem) (void)hipHostFree(e->h_rmem);
  if (e->stream_res) (void)hipStreamDestroy(e->stream_res);
  delete e;  // every DevBuf of the engine and of its sum workspaces
}

unsigned eea_steps(const eea_engine* e) { return e ? static_cast<unsigned>(e->T) : 0u; }
unsigned eea_batch_agent_lanes(const eea_engine* e, unsigned B) { return e ? batch_form(e, B).lanes : 0u; }
unsigned eea_batch_record_count(const eea_engine* e, unsigned B) { return e ? batch_form(e, B).records(B) : 0u; }
unsigned eea_num_modes(const eea_engine* e) { return e ? static_cast<unsigned>(e->K2) : 0u; }
size_t eea_real_size(const eea_engine* e) { return e ? e->rs : 0; }
unsigned eea_ck_record_len(const eea_engine* e) { return e ? static_cast<unsigned>(eea::ck_record_len(e->K2)) : 0u; }
double eea_time_step(const eea_engine* e) { return e ? e->cfg.dt : 0.0; }

eea_status eea_set_target_gaussians(eea_engine* e, unsigned n, const double* mu, const double* sigma)
{
  if (e == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null engine");
  if (n > 0 && (mu == nullptr || sigma == nullptr)) return fail(EEA_ERR_INVALID_ARGUMENT, "null target");
  e->mu.assign(mu, mu + 2 * static_cast<size_t>(n));
  e->sigma.assign(sigma, sigma + 2 * static_cast<size_t>(n));
  e->have_gauss = true;
  return EEA_OK;
}

eea_status eea_set_target_grid(eea_engine* e, unsigned nx, unsigned ny, const void* phi_vals,
                               int on_device, double lx, double ly, void* stream)
{
  // (the arguments are judged here, without touching e, and reported by the prologue in its order: null engine first, then a
  // failed wait for an enqueued rebuild, then this message, then the device -- the same at every entry below)
  const bool ok = phi_vals != nullptr && nx != 0 && ny != 0 && lx > 0.0 && ly > 0.0;
  const eea_status st = enter_target(e, ok ? nullptr : "bad target grid");
  if (st != EEA_OK) return st;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return by_precision(e, [&](auto r) { return set_target_grid_impl<decltype(r)>(e, nx, ny, phi_vals, on_device, lx, ly, s); });
}

eea_status eea_spatial_coeff_rows(eea_engine* e, unsigned nx, unsigned ny_total, unsigned row0,
                                  unsigned nrows, const void* d_phi_rows, double lx, double ly,
                                  void* d_phik_partial, void* stream)
{
  const bool ok = d_phi_rows != nullptr && d_phik_partial != nullptr && nx != 0 && ny_total != 0 && nrows != 0 &&
                  row0 + nrows <= ny_total && lx > 0.0 && ly > 0.0;
  const eea_status st0 = enter_target(e, ok ? nullptr : "bad grid tile");
  if (st0 != EEA_OK) return st0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return by_precision(e, [&](auto r) {
    using R = decltype(r);
    // the tables are built for the tile's domain; the engine's own domain is not involved
    eea_status st = upload_axes_and_tables<R>(e, nx, ny_total, lx, ly, s);
    if (st != EEA_OK) return st;
    st = reserve_tile_work<R>(e, nx, ny_total, nrows);
    if (st != EEA_OK) return st;
    EEA_HIP(eea::launch_spatial_coeff<R>(as<R>(d_phi_rows), nx, nrows, e->K, as<R>(e->tab.cx.p),
                                         as<R>(e->tab.cy.p) + static_cast<size_t>(row0) * e->K, as<R>(e->d_work.p),
                                         as<R>(d_phik_partial), s));
    return EEA_OK;
  });
}

eea_status eea_set_target_occupancy(eea_engine* e, unsigned nx, unsigned ny, const int8_t* occ,
                                    int on_device, double lx, double ly, void* stream)
{
  const bool ok = occ != nullptr && nx != 0 && ny != 0 && lx > 0.0 && ly > 0.0;
  eea_status st = enter_target(e, ok ? nullptr : "bad occupancy grid");
  if (st != EEA_OK) return st;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t P = static_cast<size_t>(nx) * ny;
  const int8_t* d_occ = occ;
  if (!on_device) {
    EEA_HIP(e->d_occ.reserve(P));
    EEA_HIP(hipMemcpyAsync(e->d_occ.p, occ, P, hipMemcpyHostToDevice, s));
    EEA_HIP(hipStreamSynchronize(s));
    d_occ = static_cast<const int8_t*>(e->d_occ.p);
  }
  e->nx = nx;
  e->ny = ny;
  e->have_fill_grid = false;
  EEA_HIP(e->d_raw.reserve(e->rs * e->K2));
  // the whole grid on this engine: the reduction launch normalises by mode (0, 0)'s sum itself (phi_k / sum(phi), target.cpp:87) --
  // two launches, the same bits as sums -> launch_normalise_by_first (which the row-tiled multi-rank form still uses, behind its
  // all-reduce); the normaliser goes to d_raw[0]
  st = by_precision(e, [&](auto r) {
    return occupancy_rows_impl<decltype(r)>(e, nx, ny, 0, ny, lx, ly, d_occ, e->d_phik.p, s, e->d_raw.p);
  });
  if (st != EEA_OK) return st;
  EEA_HIP(hipStreamSynchronize(s));
  commit_phik(e, lx, ly);
  return EEA_OK;
}

eea_status eea_spatial_coeff_occupancy_rows(eea_engine* e, unsigned nx, unsigned ny_total, unsigned row0,
                                            unsigned nrows, const int8_t* d_occ_rows, double lx, double ly,
                                            void* d_sums_partial, void* stream)
{
  const bool ok = d_occ_rows != nullptr && d_sums_partial != nullptr && nx != 0 && ny_total != 0 && nrows != 0 &&
                  row0 + nrows <= ny_total && lx > 0.0 && ly > 0.0;
  const eea_status st = enter_target(e, ok ? nullptr : "bad occupancy tile");
  if (st != EEA_OK) return st;
  hipStream_t s = static_cast<hipStream_t>(stream);
  // (the tables are built for the tile's domain; the engine's own domain is not involved)
  return by_precision(e, [&](auto r) {
    return occupancy_rows_impl<decltype(r)>(e, nx, ny_total, row0, nrows, lx, ly, d_occ_rows, d_sums_partial, s);
  });
}

eea_status eea_set_phik(eea_engine* e, const void* phik, int on_device, double lx, double ly)
{
  const bool ok = phik != nullptr && lx > 0.0 && ly > 0.0;
  const eea_status st = enter_target(e, ok ? nullptr : "bad phi_k");
  if (st != EEA_OK) return st;
  EEA_HIP(hipMemcpy(e->d_phik.p, phik, e->rs * e->K2, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
  commit_phik(e, lx, ly);
  return EEA_OK;
}

eea_status eea_set_phik_from_sums(eea_engine* e, const void* d_sums, double lx, double ly, void* stream)
{
  const bool ok = d_sums != nullptr && lx > 0.0 && ly > 0.0;
  const eea_status st0 = enter_target(e, ok ? nullptr : "bad sums");
  if (st0 != EEA_OK) return st0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const eea_status st = by_precision(e, [&](auto r) {
    using R = decltype(r);
    EEA_HIP(eea::launch_normalise_by_first<R>(as<R>(d_sums), e->K2, as<R>(e->d_phik.p), s));
    return EEA_OK;
  });
  if (st != EEA_OK) return st;
  commit_phik(e, lx, ly);
  return EEA_OK;
}

static eea_status config_domain_impl(eea_engine* e, double xmin, double xmax, double ymin, double ymax, int* rebuilt,
                                     void* stream, bool wait)
{
  if (e == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null engine");
  if (rebuilt) *rebuilt = 0;
  // translation from map to fourier domain is refreshed on every call (:366-367)
  e->map_x = xmin;
  e->map_y = ymin;
  const double mx = xmax - xmin, my = ymax - ymin;
  // almost_equal, numerics.hpp:68-71
  if (std::fabs(mx - e->lx) < 1.0e-12 && std::fabs(my - e->ly) < 1.0e-12) return EEA_OK;
  if (!e->have_gauss) return fail(EEA_ERR_NO_TARGET, "configTarget before setTarget");
  eea_status st = use_device(e);
  if (st != EEA_OK) return st;
  hipStream_t s = static_cast<hipStream_t>(stream);
  // the reference throws out of the controller when this fails; the new extent becomes the engine's only with its phi_k
  // (left behind by a failed rebuild, the next call would take the almost_equal early return with a stale phi_k)
  st = by_precision(e, [&](auto r) { return rebuild_phik<decltype(r)>(e, mx, my, s, wait); });
  if (st != EEA_OK) return st;
  if (rebuilt) *rebuilt = 1;
  return st;
}

eea_status eea_config_domain(eea_engine* e, double xmin, double xmax, double ymin, double ymax,
                             int* rebuilt, void* stream)
{
  return config_domain_impl(e, xmin, xmax, ymin, ymax, rebuilt, stream, true);
}

eea_status eea_config_domain_async(eea_engine* e, double xmin, double xmax, double ymin, double ymax,
                                   int* rebuilt, void* stream)
{
  return config_domain_impl(e, xmin, xmax, ymin, ymax, rebuilt, stream, false);
}

static eea_status download_reals(eea_engine* e, const void* d, size_t n, double* out)
{
  eea_status st = use_device(e);
  if (st != EEA_OK) return st;
  if (e->f32) {
    std::vector<float> tmp(n);
    EEA_HIP(hipMemcpy(tmp.data(), d, sizeof(float) * n, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) out[i] = tmp[i];
  } else {
    EEA_HIP(hipMemcpy(out, d, sizeof(double) * n, hipMemcpyDeviceToHost));
  }
  return EEA_OK;
}

eea_status eea_get_phik(eea_engine* e, double* h_phik)
{
  if (e == nullptr || h_phik == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  if (finish_rebuild(e) != EEA_OK) return EEA_ERR_HIP;
  return download_reals(e, e->d_phik.p, e->K2, h_phik);
}

eea_status eea_get_lamdak(eea_engine* e, double* h_lamdak)
{
  if (e == nullptr || h_lamdak == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  return download_reals(e, e->d_lamdak.p, e->K2, h_lamdak);
}

eea_status eea_target_grid_size(const eea_engine* e, unsigned* nx, unsigned* ny)
{
  if (e == nullptr || nx == nullptr || ny == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  *nx = e->nx;
  *ny = e->ny;
  return EEA_OK;
}

eea_status eea_records_field(eea_engine* e, int kind, unsigned n_rec, const void* d_rec, unsigned nx, unsigned ny_total,
                             unsigned row0, unsigned nrows, void* d_field, void* stream)
{
  // every argument check comes before the engine is read and before any HIP call
  if (e == nullptr || d_rec == nullptr || d_field == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  if (n_rec == 0 || nx == 0 || ny_total == 0 || nrows == 0) {
    return fail(EEA_ERR_INVALID_ARGUMENT, "n_rec, nx, ny_total and nrows must be positive");
  }
  if (row0 > ny_total || nrows > ny_total - row0) return fail(EEA_ERR_INVALID_ARGUMENT, "row0 + nrows > ny_total");
  if (kind != EEA_FIELD_DENSITY && kind != EEA_FIELD_DEFICIT && kind != EEA_FIELD_POTENTIAL) {
    return fail(EEA_ERR_INVALID_ARGUMENT, "unknown field kind");
  }
  if (static_cast<unsigned long long>(nx) * ny_total > (1ull << 31)) {
    return fail(EEA_ERR_UNSUPPORTED, "field grid: nx * ny_total <= 2^31");
  }
  // (the axis tables are indexed with int: (nx + ny_total) * K < 2^31 for every K <= 32)
  if (static_cast<unsigned long long>(nx) + ny_total > (1ull << 26) - 1) {
    return fail(EEA_ERR_UNSUPPORTED, "field grid: nx + ny_total < 2^26");
  }
  if (!e->have_phik) return fail(EEA_ERR_NO_TARGET, "no phi_k: call eea_config_domain or eea_set_target_grid first");
  if (reinterpret_cast<uintptr_t>(d_field) % e->rs != 0 || reinterpret_cast<uintptr_t>(d_rec) % e->rs != 0) {
    return fail(EEA_ERR_INVALID_ARGUMENT, "d_rec / d_field are not aligned to the engine's real");
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  const eea_status st = eea::engine_enter(e, s);  // the device, and behind a rebuild that was only enqueued on another stream
  if (st != EEA_OK) return st;
  return by_precision(e, [&](auto r) {
    return records_field_impl<decltype(r)>(e, kind, n_rec, d_rec, nx, ny_total, row0, nrows, d_field, s);
  });
}

eea_status eea_get_target_grid(eea_engine* e, double* h_phi_vals)
{
  if (e == nullptr || h_phi_vals == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  if (e->nx == 0 || !e->have_fill_grid || (e->d_phi.p == nullptr && !e->fill_deferred)) {
    return fail(EEA_ERR_NO_TARGET, "no Target::fill grid on the device (explicit / occupancy targets are not kept)");
  }
  if (finish_rebuild(e) != EEA_OK) return EEA_ERR_HIP;
  const size_t P = static_cast<size_t>(e->nx) * e->ny;
  if (e->fill_deferred) {  // the Gaussian rebuild never needed the grid: fill it now (un-normalised; the mass is in d_sum[0])
    const eea_status stf = by_precision(e, [&](auto r) { return fill_deferred_grid<decltype(r)>(e); });
    if (stf != EEA_OK) return stf;
  }
  eea_status st = download_reals(e, e->d_phi.p, P, h_phi_vals);
  if (st != EEA_OK || !e->phi_is_raw) return st;
  // the device keeps the un-normalised grid and its mass; phi_vals / sum(phi_vals) as target.cpp:87 forms it
  double mass = 0.0;
  st = download_reals(e, e->d_sum.p, 1, &mass);
  if (st != EEA_OK) return st;
  if (e->f32) {
    const float m = static_cast<float>(mass);
    for (size_t i = 0; i < P; ++i) h_phi_vals[i] = static_cast<double>(static_cast<float>(h_phi_vals[i]) / m);
  } else {
    for (size_t i = 0; i < P; ++i) h_phi_vals[i] = h_phi_vals[i] / mass;
  }
  return EEA_OK;
}

eea_status eea_control_batch(eea_engine* e, unsigned B, const eea_batch_io* io, void* stream)
{
  return eea::control_batch(e, B, io, stream, nullptr);
}

eea_status eea_control_batch_steps(eea_engine* e, unsigned B, const eea_batch_io* io, unsigned n_steps,
                                   unsigned pose_step_stride, unsigned u0_step_stride, void* stream)
{
  return eea::control_batch(e, B, io, stream, nullptr, n_steps, pose_step_stride, u0_step_stride);
}

static eea_status records_sum_impl(eea_engine* e, unsigned B, const void* d_ck_rec, void* d_sum, void* stream,
                                   const unsigned* d_ready, unsigned seq, unsigned* d_flag)
{
  const bool ok = d_ck_rec != nullptr && d_sum != nullptr && B != 0;
  const eea_status st0 = enter_launch(e, ok ? nullptr : "d_ck_rec, d_sum and B > 0 are required");
  if (st0 != EEA_OK) return st0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  std::lock_guard<std::mutex> lock(e->sum_mutex);  // across the launch: the workspace must not be recycled under it
  return by_precision(e, [&](auto r) {
    using R = decltype(r);
    eea_engine::SumWs* w = nullptr;
    const eea_status st = sum_workspace<R>(e, d_sum, B, s, &w);
    if (st != EEA_OK) return st;
    EEA_HIP(eea::launch_ck_records_sum<R>(as<R>(d_ck_rec), B, e->K2, as<R>(w->ws.p), static_cast<unsigned*>(w->ctr.p),
                                          as<R>(d_sum), s, d_ready, seq, d_flag));
    return EEA_OK;
  });
}

eea_status eea_ck_records_sum(eea_engine* e, unsigned B, const void* d_ck_rec, void* d_sum, void* stream)
{
  return records_sum_impl(e, B, d_ck_rec, d_sum, stream, nullptr, 0u, nullptr);
}

eea_status eea_ck_records_sum_ws_bytes(const eea_engine* e, unsigned B, size_t* ws_bytes, size_t* ticket_bytes)
{
  if (e == nullptr || B == 0) return fail(EEA_ERR_INVALID_ARGUMENT, "null engine / B == 0");
  if (ws_bytes) *ws_bytes = e->rs * eea::ck_sum_ws_elems(B, e->K2);
  if (ticket_bytes) *ticket_bytes = sizeof(unsigned) * eea::ck_sum_tickets(B, e->K2);
  return EEA_OK;
}

// the plain record sum with a caller-owned workspace: no allocation, no cache look-up, nothing but the launch (capturable)
eea_status eea_ck_records_sum_ws(eea_engine* e, unsigned B, const void* d_ck_rec, void* d_sum, void* d_ws, void* d_tickets,
                                 void* stream)
{
  const bool ok = d_ck_rec != nullptr && d_sum != nullptr && d_ws != nullptr && d_tickets != nullptr && B != 0;
  const eea_status st = enter_launch(e, ok ? nullptr : "d_ck_rec, d_sum, d_ws, d_tickets and B > 0 are required");
  if (st != EEA_OK) return st;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return by_precision(e, [&](auto r) {
    using R = decltype(r);
    EEA_HIP(eea::launch_ck_records_sum<R>(as<R>(d_ck_rec), B, e->K2, as<R>(d_ws), static_cast<unsigned*>(d_tickets), as<R>(d_sum),
                                          s, nullptr, 0u, nullptr));
    return EEA_OK;
  });
}

eea_status eea_ck_records_sum_bound(eea_engine* e, unsigned B, const void* d_ck_rec, const unsigned* d_rec_ready, unsigned seq,
                                    void* d_sum, unsigned* d_flag, void* stream)
{
  if (d_rec_ready == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "d_rec_ready is required (eea_batch_io::d_rec_ready of the producing calls)");
  return records_sum_impl(e, B, d_ck_rec, d_sum, stream, d_rec_ready, seq, d_flag);
}

eea_status eea_publish_record(eea_engine* e, const void* d_src, void* d_pub, unsigned* d_flag, unsigned seq, void* stream)
{
  const bool ok = d_src != nullptr && d_pub != nullptr && d_flag != nullptr;
  const eea_status st = enter_launch(e, ok ? nullptr : "null argument");
  if (st != EEA_OK) return st;
  const int n = eea::ck_record_len(e->K2);
  hipStream_t s = static_cast<hipStream_t>(stream);
  return by_precision(e, [&](auto r) {
    using R = decltype(r);
    EEA_HIP(eea::launch_publish_record<R>(as<R>(d_src), n, as<R>(d_pub), d_flag, seq, s));
    return EEA_OK;
  });
}

eea_status eea_rollout_batch(eea_engine* e, unsigned B, const void* d_pose, const void* d_ut,
                             void* d_traj, int* d_status, void* stream)
{
  const bool ok = d_pose != nullptr && d_ut != nullptr && d_traj != nullptr;
  const eea_status st = enter_launch(e, ok ? nullptr : "d_pose, d_ut and d_traj are required");
  if (st != EEA_OK) return st;
  eea_batch_io io;
  std::memset(&io, 0, sizeof(io));
  io.d_pose = d_pose;
  io.d_ut = const_cast<void*>(d_ut);  // rollout_only never writes ut
  io.d_traj = d_traj;
  io.d_status = d_status;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return by_precision(e, [&](auto r) { return control_batch_impl<decltype(r)>(e, B, &io, true, s); });
}

eea_status eea_control(eea_engine* e, double xmin, double xmax, double ymin, double ymax,
                       const double x[3], const double* h_mem_cols, unsigned n_mem, double u_out[3])
{
  const char* bad = nullptr;
  if (x == nullptr || u_out == nullptr) bad = "null argument";
  else if (n_mem > 0 && h_mem_cols == nullptr) bad = "null mem_cols";
  eea_status st = enter_launch(e, bad);
  if (st != EEA_OK) return st;
  // pose_ = x; configTarget(grid)  (:227-230): enqueued on the same stream as the control kernel, no host wait
  st = eea_config_domain_async(e, xmin, xmax, ymin, ymax, nullptr, e->stream1);
  if (st != EEA_OK) return st;
  if (!e->have_phik) return fail(EEA_ERR_NO_TARGET, "no target set");
  for (int i = 0; i < 3; ++i) e->last_pose[i] = x[i];
  // one robot, one control() per tick without a launch per call (EEA_OPT_RESIDENT_CONTROL); a replay-memory sample beyond
  // the mapped buffer takes the launch path
  if (eea::option(EEA_OPT_RESIDENT_CONTROL) != 0 && n_mem <= static_cast<unsigned>(eea::kResidentMemCols)) {
    st = by_precision(e, [&](auto r) { return control_resident<decltype(r)>(e, x, h_mem_cols, n_mem, u_out); });
    if (st != EEA_ERR_UNSUPPORTED) return st;  // (UNSUPPORTED: the shape does not fit a resident workgroup -- launch path)
  } else {
    st = resident_stop(e);  // (the option was switched off, or this call does not fit: the launch path owns d_ut1 now)
    if (st != EEA_OK) return st;
  }

  eea_batch_io io;
  std::memset(&io, 0, sizeof(io));
  if (n_mem > 0) {
    const size_t bytes = e->rs * 3 * n_mem;
    st = stage_reserve(e, bytes);
    if (st != EEA_OK) return st;
    {
      size_t want = 4096;  // power-of-two steps: the replay memory grows by one column per tick
      while (want < bytes) want *= 2;
      EEA_HIP(e->d_mem1.reserve(want));
    }
    store_reals(e, h_mem_cols, e->h_stage, 3 * static_cast<size_t>(n_mem));
    EEA_HIP(hipMemcpyAsync(e->d_mem1.p, e->h_stage, bytes, hipMemcpyHostToDevice, e->stream1));
    io.d_mem_cols = e->d_mem1.p;
    io.mem_stride = n_mem;  // d_n_mem == NULL: every reserved column is valid
  }
  store_reals(e, x, e->h_mail->pose, 3);
  e->h_mail->status = 0;
  Mailbox* const dm = static_cast<Mailbox*>(e->d_mail);
  io.d_pose = dm->pose;
  io.d_u0 = dm->u0;
  io.d_status = &dm->status;
  io.d_ut = e->d_ut1.p;
  e->mail_seq = (e->mail_seq % 1000000) + 1;
  st = by_precision(e, [&](auto r) { return control_batch_impl<decltype(r)>(e, 1, &io, false, e->stream1, nullptr, &dm->done); });
  if (st != EEA_OK) return st;
  // the kernel publishes u0 / status and then the sequence number with a system-scope release: poll it
  // (a few microseconds earlier than the stream's completion signal); bounded, then the ordinary wait
  const bool poll = eea::option(EEA_OPT_MAILBOX_POLL) != 0;
  bool seen = false;
  if (poll) {
    const volatile int* const flag = &e->h_mail->done;
    for (int spin = 0; spin < 200000; ++spin) {
      if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == e->mail_seq) {
        seen = true;
        break;
      }
    }
  }
  if (!seen) EEA_HIP(hipStreamSynchronize(e->stream1));
  if (e->h_mail->status == EEA_ERR_INVALID_TWIST) {
    return fail(EEA_ERR_INVALID_TWIST, "Invalid twist y-velocity must be 0.");
  }
  by_precision(e, [&](auto r) {
    for (int i = 0; i < 3; ++i) u_out[i] = as<decltype(r)>(e->h_mail->u0)[i];
  });
  return EEA_OK;
}

eea_status eea_resident_stop(eea_engine* e)
{
  const eea_status st = enter_launch(e);
  if (st != EEA_OK) return st;
  return resident_stop(e);
}

eea_status eea_opt_traj(eea_engine* e, double* h_traj)
{
  if (e == nullptr || h_traj == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  eea_status st = use_device(e);
  if (st != EEA_OK) return st;
  store_reals(e, e->last_pose, e->h_mail->pose, 3);
  e->h_mail->status = 0;
  Mailbox* const dm = static_cast<Mailbox*>(e->d_mail);
  st = eea_rollout_batch(e, 1, dm->pose, e->d_ut1.p, e->d_traj1.p, &dm->status, e->stream1);
  if (st != EEA_OK) return st;
  EEA_HIP(hipStreamSynchronize(e->stream1));
  if (e->h_mail->status == EEA_ERR_INVALID_TWIST) {
    return fail(EEA_ERR_INVALID_TWIST, "Invalid twist y-velocity must be 0.");
  }
  return download_reals(e, e->d_traj1.p, 3 * static_cast<size_t>(e->T), h_traj);
}

eea_status eea_get_ut(eea_engine* e, double* h_ut)
{
  if (e == nullptr || h_ut == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  EEA_HIP(hipStreamSynchronize(e->stream1));
  return download_reals(e, e->d_ut1.p, 3 * static_cast<size_t>(e->T), h_ut);
}

eea_status eea_set_ut(eea_engine* e, const double* h_ut)
{
  if (e == nullptr || h_ut == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  eea_status st = use_device(e);
  if (st != EEA_OK) return st;
  const size_t n = 3 * static_cast<size_t>(e->T);
  if (e->res_launched && e->res_one_wavefront) {  // its warm start is in LDS: the next call starts another one from d_ut1
    st = resident_stop(e);
    if (st != EEA_OK) return st;
  }
  EEA_HIP(hipStreamSynchronize(e->stream1));
  const void* src = h_ut;  // fp64: straight from the caller, as download_reals copies straight to it
  std::vector<float> narrowed;
  if (e->f32) {
    narrowed.resize(n);
    store_reals(e, h_ut, narrowed.data(), n);
    src = narrowed.data();
  }
  EEA_HIP(hipMemcpy(e->d_ut1.p, src, e->rs * n, hipMemcpyHostToDevice));
  return EEA_OK;
}

// ---- Basis free functions ------------------------------------------------------------------
static eea_status basis_points(int device, double lx, double ly, unsigned K, const double* xs,
                               const double* ys, const double* ws, unsigned P, double scale,
                               double* out)
{
  if (K == 0 || K > static_cast<unsigned>(eea::kMaxBasis)) return fail(EEA_ERR_UNSUPPORTED, "num_basis must be in [1, 32]");
  EEA_HIP(hipSetDevice(device));
  const size_t K2 = static_cast<size_t>(K) * K;
  DevBuf dx, dy, dw, dwork, dout;
  EEA_HIP(dx.reserve(sizeof(double) * (P ? P : 1)));
  EEA_HIP(dy.reserve(sizeof(double) * (P ? P : 1)));
  if (ws) EEA_HIP(dw.reserve(sizeof(double) * (P ? P : 1)));
  EEA_HIP(dwork.reserve(sizeof(double) * eea::point_work_elems(P, K)));
  EEA_HIP(dout.reserve(sizeof(double) * K2));
  if (P) {
    EEA_HIP(hipMemcpy(dx.p, xs, sizeof(double) * P, hipMemcpyHostToDevice));
    EEA_HIP(hipMemcpy(dy.p, ys, sizeof(double) * P, hipMemcpyHostToDevice));
    if (ws) EEA_HIP(hipMemcpy(dw.p, ws, sizeof(double) * P, hipMemcpyHostToDevice));
  }
  EEA_HIP(eea::launch_point_coeff<double>(as<double>(dx.p), as<double>(dy.p), ws ? as<double>(dw.p) : nullptr, P, K,
                                          eea::kPi / lx, eea::kPi / ly, scale, as<double>(dwork.p), as<double>(dout.p),
                                          nullptr));
  EEA_HIP(hipMemcpy(out, dout.p, sizeof(double) * K2, hipMemcpyDeviceToHost));
  return EEA_OK;
}

eea_status eea_basis_traj_coeff(int device, double lx, double ly, unsigned num_basis,
                                const double* h_xt, unsigned rows, unsigned n, double* h_ck)
{
  if (h_xt == nullptr || h_ck == nullptr || rows < 2 || n == 0) return fail(EEA_ERR_INVALID_ARGUMENT, "bad trajectory");
  std::vector<double> xs(n), ys(n);
  for (unsigned i = 0; i < n; ++i) {
    xs[i] = h_xt[static_cast<size_t>(rows) * i];
    ys[i] = h_xt[static_cast<size_t>(rows) * i + 1];
  }
  return basis_points(device, lx, ly, num_basis, xs.data(), ys.data(), nullptr, n, 1.0 / static_cast<double>(n), h_ck);
}

eea_status eea_basis_spatial_coeff(int device, double lx, double ly, unsigned num_basis,
                                   const double* h_phi_vals, const double* h_phi_grid, unsigned P,
                                   double* h_phik)
{
  if (h_phi_vals == nullptr || h_phi_grid == nullptr || h_phik == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  std::vector<double> xs(P), ys(P);
  for (unsigned i = 0; i < P; ++i) {
    xs[i] = h_phi_grid[2 * static_cast<size_t>(i)];
    ys[i] = h_phi_grid[2 * static_cast<size_t>(i) + 1];
  }
  return basis_points(device, lx, ly, num_basis, xs.data(), ys.data(), h_phi_vals, P, 1.0, h_phik);
}

eea_status eea_rk4_rollout(int device, int model, double dt, double horizon, const double x0[3],
                           const double* h_ut, double* h_xt)
{
  if (x0 == nullptr || h_ut == nullptr || h_xt == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  if (model != EEA_MODEL_OMNI && model != EEA_MODEL_SIMPLE_CART) {
    return fail(EEA_ERR_INVALID_ARGUMENT, "device rollout needs a body-twist model (Omni / SimpleCart)");
  }
  const double ratio = std::abs(horizon / dt);
  if (!(ratio < 1.0e6)) return fail(EEA_ERR_INVALID_ARGUMENT, "horizon / dt out of range");
  const unsigned steps = static_cast<unsigned>(ratio);  // integrator.hpp:141
  if (steps == 0) return EEA_OK;
  EEA_HIP(hipSetDevice(device));
  DevBuf dpose, dut, dtraj, dstat;
  EEA_HIP(dpose.reserve(sizeof(double) * 3));
  EEA_HIP(dut.reserve(sizeof(double) * 3 * steps));
  EEA_HIP(dtraj.reserve(sizeof(double) * 3 * steps));
  EEA_HIP(dstat.reserve(sizeof(int)));
  EEA_HIP(hipMemcpy(dpose.p, x0, sizeof(double) * 3, hipMemcpyHostToDevice));
  EEA_HIP(hipMemcpy(dut.p, h_ut, sizeof(double) * 3 * steps, hipMemcpyHostToDevice));
  eea::ControlParams<double> p;
  std::memset(&p, 0, sizeof(p));
  p.T = static_cast<int>(steps);
  p.K = 1;
  p.n_steps = 1;
  p.chunk = 64;
  p.dt = dt;
  p.dt6 = dt / 6.0;
  p.half_dt = 0.5 * dt;
  p.lx = p.ly = 1.0;
  p.inv_lx = p.inv_ly = 1.0;
  p.pose = as<double>(dpose.p);
  p.ut = as<double>(dut.p);
  p.traj = as<double>(dtraj.p);
  p.status = static_cast<int*>(dstat.p);
  if (eea::control_lds_bytes<double>(p.T, p.K, 0, p.chunk) > 160 * 1024) {
    return fail(EEA_ERR_HIP, std::string("rk4 rollout: ") + hipGetErrorString(hipErrorInvalidValue));
  }
  EEA_HIP(eea::launch_control<double>(p, 1, model, 0, true, nullptr));
  int status = 0;
  EEA_HIP(hipMemcpy(&status, dstat.p, sizeof(int), hipMemcpyDeviceToHost));
  if (status == 0) EEA_HIP(hipMemcpy(h_xt, dtraj.p, sizeof(double) * 3 * steps, hipMemcpyDeviceToHost));
  if (status == EEA_ERR_INVALID_TWIST) return fail(EEA_ERR_INVALID_TWIST, "Invalid twist y-velocity must be 0.");
  return EEA_OK;
}

eea_status eea_target_fill(int device, unsigned n_gauss, const double* mu, const double* sigma,
                           const double trans[2], const double* h_phi_grid, unsigned P,
                           double* h_phi_vals)
{
  if (trans == nullptr || h_phi_grid == nullptr || h_phi_vals == nullptr || (n_gauss > 0 && (mu == nullptr || sigma == nullptr))) {
    return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  }
  if (P == 0) return EEA_OK;
  EEA_HIP(hipSetDevice(device));
  std::vector<double> xs(P), ys(P);
  for (unsigned i = 0; i < P; ++i) {
    xs[i] = h_phi_grid[2 * static_cast<size_t>(i)];
    ys[i] = h_phi_grid[2 * static_cast<size_t>(i) + 1];
  }
  std::vector<double> g = gauss_params(n_gauss, mu, sigma, trans[0], trans[1]);
  if (g.empty()) g.assign(4, 0.0);  // (no Gaussian: the kernel reads none of it)
  const int blocks = static_cast<int>((P + eea::kBlock - 1) / eea::kBlock);
  DevBuf dx, dy, dg, dphi, dsum;
  EEA_HIP(dx.reserve(sizeof(double) * P));
  EEA_HIP(dy.reserve(sizeof(double) * P));
  EEA_HIP(dg.reserve(sizeof(double) * g.size()));
  EEA_HIP(dphi.reserve(sizeof(double) * P));
  EEA_HIP(dsum.reserve(sizeof(double) * (static_cast<size_t>(blocks) + 1)));
  EEA_HIP(hipMemcpy(dx.p, xs.data(), sizeof(double) * P, hipMemcpyHostToDevice));
  EEA_HIP(hipMemcpy(dy.p, ys.data(), sizeof(double) * P, hipMemcpyHostToDevice));
  EEA_HIP(hipMemcpy(dg.p, g.data(), sizeof(double) * g.size(), hipMemcpyHostToDevice));
  int n_partials = 0;
  double* const d_mass = as<double>(dsum.p);
  double* const d_partials = d_mass + 1;
  EEA_HIP(eea::launch_target_fill_points<double>(as<double>(dx.p), as<double>(dy.p), P, as<double>(dg.p),
                                                 static_cast<int>(n_gauss), as<double>(dphi.p), d_partials, &n_partials,
                                                 nullptr));
  EEA_HIP(eea::launch_reduce_sum<double>(d_partials, n_partials, d_mass, nullptr));
  EEA_HIP(eea::launch_scale_by_inv<double>(as<double>(dphi.p), P, d_mass, nullptr));
  EEA_HIP(hipMemcpy(h_phi_vals, dphi.p, sizeof(double) * P, hipMemcpyDeviceToHost));
  return EEA_OK;
}

}  // extern "C"

// What eea_set_target_gain and eea_set_target_mi share behind the checks of their field's arguments: the refusals of the target
// (floor, domain, 2^31 cells), the engine's workspaces and bookkeeping, and field -> value grid -> the launches of
// eea_spatial_coeff_rows (whole grid) and eea_set_phik_from_sums: the same bits.  field_and_values(real, field, d_values, s)
// enqueues the field into `field` -- d_field, or the engine's workspace when that is null -- and its value grid into d_values.
template <typename Cell, typename FieldAndValues>
static eea_status target_from_field(eea_engine* e, const eea::CollisionParams& c, const char* what, double floor, double lx,
                                    double ly, Cell* d_field, void* stream, FieldAndValues field_and_values)
{
  if (!(floor >= 0.0) || !std::isfinite(floor)) return fail(EEA_ERR_INVALID_ARGUMENT, "floor must be finite and >= 0");
  if (!(lx > 0.0 && ly > 0.0)) return fail(EEA_ERR_INVALID_ARGUMENT, std::string("bad ") + what + " target domain");
  const size_t P = static_cast<size_t>(c.xsize) * c.ysize;
  if (P > (static_cast<size_t>(1) << 31)) {
    return fail(EEA_ERR_UNSUPPORTED, std::string("a ") + what + " target of more than 2^31 cells");
  }
  eea_status st = enter_target(e, nullptr);
  if (st != EEA_OK) return st;
  hipStream_t s = static_cast<hipStream_t>(stream);
  // the engine's workspaces: a first call, or a growing one, waits for the device before it replaces them
  const size_t need_field = d_field != nullptr ? 0 : sizeof(Cell) * P, need_val = e->rs * P, need_raw = e->rs * e->K2;
  if (need_field > e->d_gain.cap || need_val > e->d_gain_val.cap || need_raw > e->d_raw.cap) {
    EEA_HIP(hipDeviceSynchronize());
    EEA_HIP(e->d_gain.reserve(need_field));
    EEA_HIP(e->d_gain_val.reserve(need_val));
    EEA_HIP(e->d_raw.reserve(need_raw));
  }
  Cell* const field = d_field != nullptr ? d_field : static_cast<Cell*>(e->d_gain.p);
  e->nx = c.xsize;
  e->ny = c.ysize;
  e->have_fill_grid = false;
  st = by_precision(e, [&](auto r) {
    using R = decltype(r);
    eea_status st2 = upload_axes_and_tables<R>(e, c.xsize, c.ysize, lx, ly, s);
    if (st2 != EEA_OK) return st2;
    st2 = reserve_tile_work<R>(e, c.xsize, c.ysize, c.ysize);
    if (st2 != EEA_OK) return st2;
    st2 = field_and_values(r, field, e->d_gain_val.p, s);
    if (st2 != EEA_OK) return st2;
    EEA_HIP(eea::launch_spatial_coeff<R>(as<R>(e->d_gain_val.p), c.xsize, c.ysize, e->K, as<R>(e->tab.cx.p), as<R>(e->tab.cy.p),
                                         as<R>(e->d_work.p), as<R>(e->d_raw.p), s));
    EEA_HIP(eea::launch_normalise_by_first<R>(as<R>(e->d_raw.p), e->K2, as<R>(e->d_phik.p), s));
    return EEA_OK;
  });
  if (st != EEA_OK) return st;
  commit_phik(e, lx, ly);
  return EEA_OK;
}

extern "C" {

eea_status eea_set_target_gain(eea_engine* e, const eea_collision_cfg* cfg, unsigned range_cells, unsigned stride,
                               const int8_t* d_known, double floor, double lx, double ly, unsigned* d_gain, void* stream)
{
  if (e == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null engine");
  if (cfg == nullptr || d_known == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  const eea_status st = gain_refusal(cfg, range_cells, stride);
  if (st != EEA_OK) return st;
  const eea::CollisionParams c = grid_params(cfg);
  return target_from_field(e, c, "gain", floor, lx, ly, d_gain, stream, [&](auto r, unsigned* gain, void* d_values, hipStream_t s) {
    using R = decltype(r);
    EEA_HIP(eea::launch_gain_field(c, range_cells, stride, d_known, gain, s));
    EEA_HIP(eea::launch_gain_values<R>(c, stride, d_known, gain, floor, as<R>(d_values), s));
    return EEA_OK;
  });
}

eea_status eea_set_target_mi(eea_engine* e, const eea_collision_cfg* cfg, unsigned range_cells, unsigned stride, double p_unknown,
                             const int8_t* d_known, double floor, double lx, double ly, double* d_mi, void* stream)
{
  if (e == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null engine");
  if (cfg == nullptr || d_known == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  eea_status st = gain_refusal(cfg, range_cells, stride);
  if (st == EEA_OK) st = eea::p_unknown_refusal(p_unknown);
  if (st != EEA_OK) return st;
  const eea::CollisionParams c = grid_params(cfg);
  return target_from_field(e, c, "mutual-information", floor, lx, ly, d_mi, stream,
                           [&](auto r, double* mi, void* d_values, hipStream_t s) {
                             using R = decltype(r);
                             EEA_HIP(eea::launch_mi_field(c, range_cells, stride, p_unknown, d_known, mi, s));
                             EEA_HIP(eea::launch_mi_values<R>(c, stride, d_known, mi, floor, as<R>(d_values), s));
                             return EEA_OK;
                           });
}

// the target of a field the caller already has (kind 0: the gain count, 1: the mutual information), on the candidates that
// d_geo reaches: no field launch, the value grid of geodesic_kernel.hip, then the launches the two entries above share
eea_status eea_set_target_reachable(eea_engine* e, const eea_collision_cfg* cfg, int kind, const void* d_field, unsigned stride,
                                    const int8_t* d_known, const int* d_geo, double floor, double lx, double ly, void* stream)
{
  if (e == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null engine");
  const eea_status st = eea::reachable_refusal(cfg, kind, d_field, stride, d_known, d_geo);
  if (st != EEA_OK) return st;
  const eea::CollisionParams c = grid_params(cfg);
  // (the field is the caller's and read only: no workspace is taken for it)
  return target_from_field(e, c, "reachable", floor, lx, ly, static_cast<const char*>(d_field), stream,
                           [&](auto r, const char*, void* d_values, hipStream_t s) {
                             using R = decltype(r);
                             EEA_HIP(eea::launch_reachable_values<R>(c, kind, d_field, stride, d_known, d_geo, floor, as<R>(d_values), s));
                             return EEA_OK;
                           });
}

}  // extern "C"

// ---- the fleet tick: one iteration of Exploration<ModelT>::control's loop body for B robots (exploration.hpp:220-279) ----
// See ergodic_amd.h.  The four entries differ in their obstacle model -- what a pose collides with in steps 3 and 4 -- and each
// states its own below, top to bottom in the order a caller meets its refusals: tick_arguments_refusal (what every tick asks
// of its arguments), the model's own refusals and its CollisionParams, then tick_run with the launch of steps 3 and 4.
// A tick refuses, returns for B == 0 and builds its parameter blocks before the device is touched.
static eea_status tick_arguments_refusal(const char* entry, const eea_engine* e, const eea_batch_io* io, const eea_tick_io* tick,
                                         const eea_dwa_cfg* dcfg)
{
  if (e == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null engine");
  if (io == nullptr || tick == nullptr || dcfg == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null argument");
  if (e->f32) return fail(EEA_ERR_UNSUPPORTED, std::string(entry) + " takes fp64 engines (poses and twists are doubles)");
  if (io->d_pose == nullptr || io->d_ut == nullptr || tick->d_follow_dwa == nullptr || tick->d_dwa_count == nullptr ||
      tick->d_u == nullptr || tick->d_vb == nullptr || tick->d_grid == nullptr || tick->d_traj == nullptr ||
      tick->d_valid == nullptr || tick->d_skip == nullptr) {
    return fail(EEA_ERR_INVALID_ARGUMENT, "null tick buffer");
  }
  if (io->d_rec_ready != nullptr || io->d_ck_flag != nullptr) {
    return fail(EEA_ERR_UNSUPPORTED, std::string(entry) + " does not take the device-bound exchange buffers");
  }
  return EEA_OK;
}

// The rest of a tick whose arguments and obstacle model were accepted: the window's refusals, the target, the device, steps 1
// and 2, and launch_plan(d, tail...) for steps 3 and 4 -- tail: the arguments every planning launcher ends in (common.hpp:
// from d_x0 to the stream)
template <typename LaunchPlan>
static eea_status tick_run(eea_engine* e, unsigned B, const eea_batch_io* io, const eea_tick_io* tick, const eea_dwa_cfg* dcfg,
                           void* stream, LaunchPlan&& launch_plan)
{
  // the dynamic window tracks optTraj(): T columns every cfg.dt (before step 1: a refused tick leaves follow_dwa / i alone)
  eea::DwaParams d;
  eea_status st = dwa_window_refusal(dcfg, nullptr, tick->d_traj, static_cast<unsigned>(e->T), e->cfg.dt, d);
  if (st != EEA_OK) return st;
  if (!e->have_phik) return fail(EEA_ERR_NO_TARGET, "no target set");
  st = use_device(e);
  if (st != EEA_OK) return st;
  hipStream_t s = static_cast<hipStream_t>(stream);
  // 1. followers count a step (exploration.hpp:223-228); d_skip = who follows a DWA twist this tick
  EEA_HIP(eea::launch_tick_begin(tick->d_follow_dwa, tick->d_dwa_count, tick->d_skip, d.steps, B, s));
  // 2. control() of everybody else (:230-236), the twist straight into d_u; then optTraj() of the updated controls (:257)
  eea_batch_io cio = *io;
  cio.d_u0 = tick->d_u;
  cio.d_skip = tick->d_skip;
  cio.d_traj = nullptr;
  st = control_batch_impl<double>(e, B, &cio, false, s);
  if (st != EEA_OK) return st;
  eea_batch_io rio{};
  rio.d_pose = io->d_pose;
  rio.d_ut = io->d_ut;
  rio.d_traj = tick->d_traj;
  rio.d_skip = tick->d_skip;
  st = control_batch_impl<double>(e, B, &rio, true, s);
  if (st != EEA_OK) return st;
  // 3. validate_control (:238, numerics.hpp:312-330); 4. the dynamic window where the twist was rejected (:240-277), u /
  // follow_dwa / i updated in place
  EEA_HIP(launch_plan(d, static_cast<const double*>(io->d_pose), tick->d_vb, tick->d_traj, static_cast<unsigned>(e->T), e->cfg.dt,
                      tick->val_dt, horizon_steps(tick->val_horizon, tick->val_dt), tick->d_valid, tick->d_follow_dwa,
                      tick->d_dwa_count, tick->d_u, tick->d_source, B, s));
  return EEA_OK;
}

extern "C" {

// the disc on the static map: Collision::Collision's checks, one inflated map for both steps
eea_status eea_tick_batch(eea_engine* e, unsigned B, const eea_batch_io* io, const eea_tick_io* tick,
                          const eea_collision_cfg* ccfg, const eea_dwa_cfg* dcfg, void* stream)
{
  eea_status st = tick_arguments_refusal("eea_tick_batch", e, io, tick, dcfg);
  if (st != EEA_OK || B == 0) return st;
  st = collision_cfg_refusal(ccfg);
  if (st != EEA_OK) return st;
  const eea::CollisionParams c = collision_params(ccfg);
  return tick_run(e, B, io, tick, dcfg, stream, [&](const eea::DwaParams& d, auto... tail) {
    return eea::launch_validate_and_dwa_fleet(c, d, nullptr, tick->d_grid, tick->grid_epoch, tail...);
  });
}

// ... and the other robots' discs: the layer is the tick's in B, configuration and device (B == 0 is not a layer's)
eea_status eea_tick_batch_fleet(eea_engine* e, unsigned B, const eea_batch_io* io, const eea_tick_io* tick,
                                const eea_collision_cfg* ccfg, const eea_dwa_cfg* dcfg, const eea_fleet_layer* l, void* stream)
{
  eea_status st = tick_arguments_refusal("eea_tick_batch_fleet", e, io, tick, dcfg);
  if (st != EEA_OK) return st;
  if (l == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null fleet layer");
  st = collision_cfg_refusal(ccfg);
  if (st != EEA_OK) return st;
  const eea::CollisionParams c = collision_params(ccfg);
  if (B != l->v.B) return fail(EEA_ERR_INVALID_ARGUMENT, "the tick's B is not the fleet layer's");
  if (!eea::same_params(c, l->c)) return fail(EEA_ERR_INVALID_ARGUMENT, "the tick's collision configuration is not the fleet layer's");
  if (l->device != e->cfg.device) return fail(EEA_ERR_INVALID_ARGUMENT, "the fleet layer lives on another device than the engine");
  return tick_run(e, B, io, tick, dcfg, stream, [&](const eea::DwaParams& d, auto... tail) {
    return eea::launch_validate_and_dwa_fleet(c, d, &l->v, tick->d_grid, tick->grid_epoch, tail...);
  });
}

// the polygon base on the static map: the footprint, the grid's geometry and the cell limits, as eea_footprint_check_batch
// asks them.  The radii are neither read nor checked, and tick->grid_epoch is not read: no inflated map
eea_status eea_tick_batch_footprint(eea_engine* e, unsigned B, const eea_batch_io* io, const eea_tick_io* tick,
                                    const eea_collision_cfg* ccfg, const eea_dwa_cfg* dcfg, const eea_footprint* fp,
                                    const int* d_sq, void* stream)
{
  eea_status st = tick_arguments_refusal("eea_tick_batch_footprint", e, io, tick, dcfg);
  if (st != EEA_OK) return st;
  eea::FootprintArgs f;
  st = footprint_call_refusal(ccfg, fp, tick->d_grid, io->d_pose, tick->d_valid, f);
  if (st != EEA_OK || B == 0) return st;
  const eea::CollisionParams c = grid_params(ccfg);
  return tick_run(e, B, io, tick, dcfg, stream, [&](const eea::DwaParams& d, auto... tail) {
    return eea::launch_footprint_validate_and_dwa_fleet(c, d, f, nullptr, tick->d_grid, d_sq, tail...);
  });
}

// ... and the other robots' polygons: the footprint is the layer's, and the layer is the tick's in B, grid and device
eea_status eea_tick_batch_bodies(eea_engine* e, unsigned B, const eea_batch_io* io, const eea_tick_io* tick,
                                 const eea_collision_cfg* ccfg, const eea_dwa_cfg* dcfg, const eea_body_layer* l, const int* d_sq,
                                 void* stream)
{
  static const char* const entry = "eea_tick_batch_bodies";
  eea_status st = tick_arguments_refusal(entry, e, io, tick, dcfg);
  if (st != EEA_OK) return st;
  if (l == nullptr) return named(entry, fail(EEA_ERR_INVALID_ARGUMENT, "null body layer"));
  eea::FootprintArgs f;
  st = footprint_call_refusal(ccfg, &l->fp, tick->d_grid, io->d_pose, tick->d_valid, f);
  if (st != EEA_OK) return st;
  const eea::CollisionParams c = grid_params(ccfg);
  if (B != l->v.B) return named(entry, fail(EEA_ERR_INVALID_ARGUMENT, "the tick's B is not the body layer's"));
  if (!eea::same_params(c, l->c)) {
    return named(entry, fail(EEA_ERR_INVALID_ARGUMENT, "the tick's grid geometry or occupied_threshold is not the body layer's"));
  }
  if (l->device != e->cfg.device) return named(entry, fail(EEA_ERR_INVALID_ARGUMENT, "the body layer lives on another device than the engine"));
  return tick_run(e, B, io, tick, dcfg, stream, [&](const eea::DwaParams& d, auto... tail) {
    return eea::launch_footprint_validate_and_dwa_fleet(c, d, f, &l->v, tick->d_grid, d_sq, tail...);
  });
}

}  // extern "C"

// the A/B library (make AB=1; tools/ab/) adds its diagnostic entry point here; the product does not
#ifdef EEA_AB_BUILD
#include "../../tools/ab/engine_ab.inc"
#endif
