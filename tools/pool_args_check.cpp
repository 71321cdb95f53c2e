// Host-side check of eea_replay_pool_sample's argument handling and of the life of a replay memory whose creation fails,
// meant to be built with the host sanitizers and run on a machine WITHOUT a GPU:
//   hipcc --offload-arch=gfx950 -std=c++17 -g -Xarch_host -fsanitize=address,undefined \
//         ergodic_exploration_amd/csrc/replay_kernel.hip tools/pool_args_check.cpp -o pool_args_check && ./pool_args_check
// Every call here returns before any kernel launch: the argument errors before any HIP call at all, eea_replay_create at its
// first HIP call when there is no device (its failure path frees what it holds -- the pool offsets among it -- through
// eea_replay_destroy).  With a device present the memory is created and destroyed, nothing is launched either.
#include <cstdio>

#include "../include/ergodic_amd.h"

static int failures = 0;
static void expect(bool ok, const char* what)
{
  if (!ok) {
    std::printf("FAILED: %s\n", what);
    ++failures;
  }
}

int main()
{
  double cols[2 * 4 * 3];
  int n_mem[2] = {-1, -1};
  for (double& c : cols) c = -7.0;
  alignas(16) unsigned char not_a_memory[256] = {};  // never looked into: every error below is found before the handle is used
  eea_replay* fake = reinterpret_cast<eea_replay*>(not_a_memory);
  expect(eea_replay_pool_sample(nullptr, 0, 4, 0, 0, cols, n_mem, 4, nullptr) == EEA_ERR_INVALID_ARGUMENT, "null memory");
  expect(eea_replay_pool_sample(fake, 0, 4, 0, 0, nullptr, n_mem, 4, nullptr) == EEA_ERR_INVALID_ARGUMENT, "null columns");
  expect(eea_replay_pool_sample(fake, 0, 4, 0, 0, cols, nullptr, 4, nullptr) == EEA_ERR_INVALID_ARGUMENT, "null n_mem");
  expect(eea_replay_pool_sample(fake, 0, 0, 0, 0, cols, n_mem, 4, nullptr) == EEA_ERR_INVALID_ARGUMENT, "n_cols == 0");
  expect(eea_replay_pool_sample(fake, 0, 0, 1, 1, cols, n_mem, 4, nullptr) == EEA_ERR_INVALID_ARGUMENT, "n_cols == 0, accumulate");
  expect(eea_replay_pool_sample(fake, 0, 5, 0, 0, cols, n_mem, 4, nullptr) == EEA_ERR_INVALID_ARGUMENT, "mem_stride < n_cols");
  expect(eea_replay_pool_sample(fake, 0, 4, 0, 0, cols, n_mem, 0, nullptr) == EEA_ERR_INVALID_ARGUMENT, "mem_stride == 0");
  expect(eea_replay_pool_sample(fake, 0, 4, 0, 1, cols, n_mem, 0, nullptr) == EEA_ERR_INVALID_ARGUMENT, "mem_stride == 0, accumulate");
  for (double c : cols) expect(c == -7.0, "columns untouched");
  expect(n_mem[0] == -1 && n_mem[1] == -1, "n_mem untouched");
  for (unsigned char c : not_a_memory) expect(c == 0, "handle untouched");

  eea_replay* r = nullptr;
  expect(eea_replay_create(0, 0, 8, 4, 1, 0, 8, &r) == EEA_ERR_INVALID_ARGUMENT && r == nullptr, "create: no robots");
  const eea_status st = eea_replay_create(0, 3, 8, 4, 1, 0, 8, &r);  // no device: EEA_ERR_HIP and everything freed again
  expect((st == EEA_OK) == (r != nullptr), "create: a handle exactly when it succeeded");
  eea_replay_destroy(r);
  eea_replay_destroy(nullptr);
  std::printf(failures == 0 ? "pool_args_check: ok\n" : "pool_args_check: %d failures\n", failures);
  return failures == 0 ? 0 : 1;
}
