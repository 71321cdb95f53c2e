// Error plumbing shared by the translation units behind include/ergodic_amd.h: the thread-local message
// of eea_last_error() and the status helpers; and the entries one unit calls in another.  Internal to libergodic_amd.so.
#pragma once

#include <hip/hip_runtime.h>

#include <string>

#include "../../include/ergodic_amd.h"

namespace eea
{
inline thread_local std::string g_last_error;

inline eea_status fail(eea_status st, const std::string& msg)
{
  g_last_error = msg;
  return st;
}

// eea_control_batch[_steps] that also reports the form of the launch it made (common.hpp ControlForm) in *form when not
// null (engine.cpp)
struct ControlForm;
eea_status control_batch(eea_engine* e, unsigned B, const eea_batch_io* io, void* stream, ControlForm* form,
                         unsigned n_steps = 1, unsigned pose_step_stride = 0, unsigned u0_step_stride = 0);

// What coverage_kernel.hip reads of an engine (engine.cpp) and of a replay memory (replay_kernel.hip): the structs stay
// private to their units.  engine_view / replay_view make no HIP call; engine_enter selects the engine's device and orders
// `s` behind a phi_k rebuild that was only enqueued on another stream, as the control calls do.
struct EngineView
{
  int device = 0, K = 0;
  bool f32 = false, have_phik = false;
  double lx = 0.0, ly = 0.0, map_x = 0.0, map_y = 0.0;
  const void *d_phik = nullptr, *d_lamdak = nullptr;  // [K^2] reals
};
struct ReplayView
{
  int device = 0;
  unsigned B = 0, capacity = 0;
  size_t real_size = 8;
  const void* d_store = nullptr;      // [B][capacity][3] reals
  const unsigned* d_count = nullptr;  // [B]
};
void engine_view(const eea_engine* e, EngineView* v);
eea_status engine_enter(eea_engine* e, hipStream_t s);
void replay_view(const eea_replay* r, ReplayView* v);
}  // namespace eea

#define EEA_HIP(expr)                                                                         \
  do {                                                                                        \
    const hipError_t err__ = (expr);                                                          \
    if (err__ != hipSuccess) {                                                                \
      return eea::fail(EEA_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(err__));    \
    }                                                                                         \
  } while (0)
