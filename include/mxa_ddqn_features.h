/* mxa_ddqn_features.h - libmxa_ddqn_features.so: the per-period kernels of include/mxa_ddqn.h for a
 * state of N features (include/mxa_state_spec.h), the state given as a spec, so a learner can see the
 * market columns of the observation row (marl-optimal-execution_amd/csrc/ddqn_features.hip on the
 * kernels of ddqn_period_kernels.h; mxabides/ddqn.py ExecutionTask(features=...), features_lib()).
 * The library is built beside libmxa_ddqn.so (build_lib.build_ddqn), whose own exports stay those of
 * mxa_ddqn.h and mxa_ddqn_train.h.  The conventions are include/mxa_ddqn.h's: `stream`
 * is a hipStream_t, pointers are device pointers unless said otherwise, every export returns 0 or a
 * hipError_t.  `spec` is a HOST struct read during the call; its `grid` is a device pointer that the
 * launched kernel reads.  A spec that mxa_state_spec_refusal(spec, obs_w) refuses returns
 * hipErrorInvalidValue before any HIP call, and nothing is written. */
#ifndef MXA_DDQN_FEATURES_H
#define MXA_DDQN_FEATURES_H
#include <stdint.h>

#include "mxa_state_spec.h"
#ifdef __cplusplus
extern "C" {
#endif
/* the spec's state of every env: s [n][n_feat] f32 from obs [n][obs_w] f64.  n < 0, obs_w < 1 or a
 * refused spec: hipErrorInvalidValue; n == 0 returns 0.  With the default spec the rows are
 * mxa_ddqn_state's bit for bit. */
int mxa_ddqn_state_spec(void* stream, int n, int obs_w, const double* obs, const mxa_state_spec* spec, float* s);
/* mxa_ddqn_period with the spec's state: `spec` stands where g0, n0, g1, n1 and nh stood, and the
 * rows of s, s2, ring_s and ring_s2 are n_feat wide (ring_s / ring_s2 [cap + 1][n_feat] f32).
 * Everything else is mxa_ddqn_period's: the same outputs in the same order, the same 1024-lane walk
 * with one block-wide prefix count for the ring positions, the same preconditions (n >= 0, cap > 0,
 * obs_w >= 2, st_w >= 3, with train set n <= cap), and a refused spec besides.  q0 is unread (the
 * quantity's divisor is the spec's); rscale = 1e4 / q0 as before. */
int mxa_ddqn_period_spec(void* stream, int n, int obs_w, int st_w, int train, const double* obs, const double* st,
                         const double* prev, const double* arrival, const int32_t* flags, const uint8_t* alive,
                         uint8_t* alive_next, uint8_t* live, const float* s, const int64_t* a, float* s2,
                         double* r_row, int64_t* env_steps, const mxa_state_spec* spec, double q0, double rscale,
                         float* ring_s, float* ring_s2, int64_t* ring_a, float* ring_r, int64_t cap, int64_t* n_dev,
                         int64_t* stored);
#ifdef __cplusplus
}
#endif
#endif
