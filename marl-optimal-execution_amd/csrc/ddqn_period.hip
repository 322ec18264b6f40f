// ddqn_period.hip — the DDQN execution learner's per-period bookkeeping in one launch
// (libmxa_ddqn.so, include/mxa_ddqn.h, with ddqn_qnet.hip; mxabides/ddqn.py run_episode, fused path).
//
// After each ABIDESEnv.step of every env the learner loop (ddqlearning_execution_agent.py:275-299,
// 409-446) needs: the transition mask, the reward of the step's fills (compute_reward, BUY), the
// next discretised state, the per-env step count, the replay append in env order, the masked
// reward row and the next alive mask.  In PyTorch that is ~45 small elementwise kernels per period,
// each a few microseconds on a 4096-env batch; here it is one workgroup of 1024 lanes walking the
// envs in blocks of 1024 with one block-wide prefix count for the replay positions.  Every float
// operation is the PyTorch path's, in the same order (built with -ffp-contract=off), so the outputs
// are bitwise the same (tests/test_gpu_ddqn.py compares the two paths), and both equal the plain
// float64 references of oracle/ddqn_ref.py exactly (tests/test_gpu_ddqn_kernels.py).
//
// The two state-carrying kernels are written once over the state's source (ddqn_period_kernels.h):
// here Grid2, ExecutionTask's two grids; ddqn_features.hip instantiates them for a list of features.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ddqn_period_kernels.h"

namespace {

// the state of one observation row on ExecutionTask's two grids
struct Grid2 {
  static constexpr int W = 2;
  const double *g0, *g1;
  int n0, n1;
  double nh, q0;
  __device__ int width() const { return 2; }
  __device__ void eval(const double* o, float* out) const { state_of(o, g0, n0, g1, n1, nh, q0, out); }
};

// ExecutionTask.actions (ddqn_device.h action_of) of every env
__global__ __launch_bounds__(256) void ddqn_actions_kernel(int n, int obs_w, const double* obs, const int64_t* a,
                                                           const double* table, double q0, double* act) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  action_of(table + 3 * a[i], obs + (size_t)i * obs_w, q0, act + 3 * i);
}

}  // namespace

extern "C" {

// ExecutionTask.actions for every env in one launch: act [n][3] f64 from a [n] and table [k][3]
int mxa_ddqn_actions(hipStream_t stream, int n, int obs_w, const double* obs, const int64_t* a, const double* table,
                     double q0, double* act) {
  if (n < 0 || obs_w < 2) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  hipLaunchKernelGGL(ddqn_actions_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, n, obs_w, obs, a, table, q0,
                     act);
  return (int)hipGetLastError();
}

// one period's bookkeeping (see PeriodArgs); 0 on success, else the hipError_t of the launch.
// train with n > cap could put two rows on one ring position, the winner unspecified: refused
int mxa_ddqn_period(hipStream_t stream, int n, int obs_w, int st_w, int train, const double* obs, const double* st,
                    const double* prev, const double* arrival, const int32_t* flags, const uint8_t* alive,
                    uint8_t* alive_next, uint8_t* live, const float* s, const int64_t* a, float* s2, double* r_row,
                    int64_t* env_steps, const double* g0, int n0, const double* g1, int n1, double nh, double q0,
                    double rscale, float* ring_s, float* ring_s2, int64_t* ring_a, float* ring_r, int64_t cap,
                    int64_t* n_dev, int64_t* stored) {
  if (n < 0 || cap <= 0 || obs_w < 2 || st_w < 3 || (train && n > cap)) return (int)hipErrorInvalidValue;
  PeriodArgs p{n, obs_w, st_w, train, obs, st, prev, arrival, flags, alive, alive_next, live, s, a, s2, r_row,
               env_steps, rscale, ring_s, ring_s2, ring_r, ring_a, cap, n_dev, stored};
  hipLaunchKernelGGL(ddqn_period_kernel<Grid2>, dim3(1), dim3(1024), 0, stream, p, Grid2{g0, g1, n0, n1, nh, q0});
  return (int)hipGetLastError();
}

// ExecutionTask.state for every env in one launch
int mxa_ddqn_state(hipStream_t stream, int n, int obs_w, const double* obs, const double* g0, int n0, const double* g1,
                   int n1, double nh, double q0, float* s) {
  if (n < 0 || obs_w < 2) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  hipLaunchKernelGGL(ddqn_state_kernel<Grid2>, dim3((n + 255) / 256), dim3(256), 0, stream, n, obs_w, obs,
                     Grid2{g0, g1, n0, n1, nh, q0}, s);
  return (int)hipGetLastError();
}

}  // extern "C"
