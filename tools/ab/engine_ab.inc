// Included at the end of csrc/engine.cpp by the A/B library only (make AB=1): the diagnostic entry point declared in
// tools/ab/ergodic_amd_ab.h.  Same as eea_control_batch with the kernels' phase stamps switched on (p.dbg).
#include "../../tools/ab/ergodic_amd_ab.h"

namespace eea
{
// tools/ab/control_kernel_timing.hip: the workgroup-per-agent kernel with phase stamps (K = 10 and 30, fp64)
hipError_t launch_control_timing(const ControlParams<double>& p, unsigned B, int model, int n_mem_max,
                                 hipStream_t stream);
}  // namespace eea

extern "C" eea_status eea_debug_phase_timing(eea_engine* e, unsigned B, const eea_batch_io* io, void* stream,
                                             long long* d_stamps)
{
  if (e == nullptr) return fail(EEA_ERR_INVALID_ARGUMENT, "null engine");
  if (io == nullptr || io->d_pose == nullptr || io->d_ut == nullptr || io->d_u0 == nullptr || d_stamps == nullptr) {
    return fail(EEA_ERR_INVALID_ARGUMENT, "d_pose, d_ut, d_u0 and d_stamps are required");
  }
  if (!e->have_phik) return fail(EEA_ERR_NO_TARGET, "no phi_k");
  eea_status st = use_device(e);
  if (st != EEA_OK) return st;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (e->f32) return control_batch_impl<float>(e, B, io, false, s, nullptr, nullptr, d_stamps);  // wavefront-per-agent kernel only
  eea::ControlParams<double> p;
  fill_params<double>(e, p);
  p.pose = static_cast<const double*>(io->d_pose);
  p.ut = static_cast<double*>(io->d_ut);
  p.u0 = static_cast<double*>(io->d_u0);
  p.ck = static_cast<double*>(io->d_ck);
  p.dbg = d_stamps;  // (no packed form with stamps: the wavefront kernel or the workgroup)
  if (control_form<double>(p, B, false).lanes == 64) return control_batch_impl<double>(e, B, io, false, s, nullptr, nullptr, d_stamps);
  // [agent][4 waves][16] stamps of the workgroup-per-agent kernel's instrumented build
  if (eea::control_lds_bytes<double>(p.T, p.K, 0, p.chunk) > 160 * 1024) {
    return fail(EEA_ERR_UNSUPPORTED, "horizon/basis too large for one workgroup's 160 KiB LDS");
  }
  EEA_HIP(eea::launch_control_timing(p, B, e->cfg.model, 0, s));
  return EEA_OK;
}
