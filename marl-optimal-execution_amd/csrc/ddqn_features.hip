// ddqn_features.hip — the DDQN learner's per-period kernels for a state of N features
// (libmxa_ddqn_features.so, include/mxa_ddqn_features.h, mxa_state_spec.h; mxabides/ddqn.py
// ExecutionTask(features=...)): ddqn_period.hip's kernels (ddqn_period_kernels.h) instantiated with
// the state of a spec, the rows of s, s2 and the replay ring n_feat wide.  A library of its own:
// libmxa_ddqn.so's exports stay those of its two headers.  Built with -ffp-contract=off like
// ddqn_period.hip, so the default spec's 2 * (o / nh) + (-1.0) has state_of's bits.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ddqn_period_kernels.h"

namespace {

struct Spec {
  static constexpr int W = MXA_STATE_MAX_FEATURES;
  mxa_state_spec sp;
  __device__ int width() const { return sp.n_feat; }
  __device__ void eval(const double* o, float* out) const { state_of_spec(o, sp, out); }
};

}  // namespace

extern "C" {

// ExecutionTask(features=...).state for every env in one launch
int mxa_ddqn_state_spec(hipStream_t stream, int n, int obs_w, const double* obs, const mxa_state_spec* spec, float* s) {
  if (n < 0 || obs_w < 1 || mxa_state_spec_refusal(spec, obs_w)) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  hipLaunchKernelGGL(ddqn_state_kernel<Spec>, dim3((n + 255) / 256), dim3(256), 0, stream, n, obs_w, obs, Spec{*spec},
                     s);
  return (int)hipGetLastError();
}

// mxa_ddqn_period with the state of a spec; the same guards, and the spec's
int mxa_ddqn_period_spec(hipStream_t stream, int n, int obs_w, int st_w, int train, const double* obs,
                         const double* st, const double* prev, const double* arrival, const int32_t* flags,
                         const uint8_t* alive, uint8_t* alive_next, uint8_t* live, const float* s, const int64_t* a,
                         float* s2, double* r_row, int64_t* env_steps, const mxa_state_spec* spec, double q0,
                         double rscale, float* ring_s, float* ring_s2, int64_t* ring_a, float* ring_r, int64_t cap,
                         int64_t* n_dev, int64_t* stored) {
  (void)q0;
  if (n < 0 || cap <= 0 || obs_w < 2 || st_w < 3 || (train && n > cap)) return (int)hipErrorInvalidValue;
  if (mxa_state_spec_refusal(spec, obs_w)) return (int)hipErrorInvalidValue;
  PeriodArgs p{n, obs_w, st_w, train, obs, st, prev, arrival, flags, alive, alive_next, live, s, a, s2, r_row,
               env_steps, rscale, ring_s, ring_s2, ring_r, ring_a, cap, n_dev, stored};
  hipLaunchKernelGGL(ddqn_period_kernel<Spec>, dim3(1), dim3(1024), 0, stream, p, Spec{*spec});
  return (int)hipGetLastError();
}

}  // extern "C"
