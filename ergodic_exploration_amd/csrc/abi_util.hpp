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
}  // namespace eea

#define EEA_HIP(expr)                                                                         \
  do {                                                                                        \
    const hipError_t err__ = (expr);                                                          \
    if (err__ != hipSuccess) {                                                                \
      return eea::fail(EEA_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(err__));    \
    }                                                                                         \
  } while (0)
