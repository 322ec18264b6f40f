// ddqn_device.h — ExecutionTask's state and action vector on the device, one restatement shared
// by the kernels of libmxa_ddqn.so (ddqn_period.hip, ddqn_qnet.hip; mxabides/ddqn.py).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/mxa_state_spec.h"

// torch.bucketize(x, bd, right=True): searchsorted's upper bound, NaN sorting last
__device__ inline int64_t upper_bound(double x, const double* bd, int n) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (!(bd[mid] > x)) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// ExecutionTask.state: discretize([2 * rem_t / nh - 1, 2 * rem_q / q0 - 1]) with true divisions,
// as the reference's numpy (ddqlearning_execution_agent.py:307-308): the reciprocal form lands
// one bin higher at 73 of the quantities 0..100000 (multiples of 250 from 50250 up)
__device__ inline void state_of(const double* o, const double* g0, int n0, const double* g1, int n1, double nh,
                                double q0, float* out) {
  const double tr = 2.0 * (o[0] / nh) - 1.0;
  const double qr = 2.0 * (o[1] / q0) - 1.0;
  out[0] = (float)upper_bound(tr, g0, n0);
  out[1] = (float)upper_bound(qr, g1, n1);
}

// One feature of a state spec (include/mxa_state_spec.h) on the observation row o: the scaled column,
// binned on the feature's own split points, or passed through where it has none.  With
// -ffp-contract=off the default spec's 2.0 * (o / nh) + (-1.0) is state_of's 2.0 * (o / nh) - 1.0.
// O: a pointer to the row in any address space (the step kernel's observation lives in LDS)
template <class O>
__device__ inline float state_feature(O o, const mxa_state_spec& sp, int f) {
  const double x = sp.mul[f] * (o[sp.col[f]] / sp.div[f]) + sp.add[f];
  const int n = sp.goff[f + 1] - sp.goff[f];
  return n > 0 ? (float)upper_bound(x, sp.grid + sp.goff[f], n) : (float)x;
}

// ExecutionTask(features=...).state of one env: out[f] for f < n_feat (out holds
// MXA_STATE_MAX_FEATURES; the constant trip count keeps it in registers)
__device__ inline void state_of_spec(const double* o, const mxa_state_spec& sp, float* out) {
#pragma unroll
  for (int f = 0; f < MXA_STATE_MAX_FEATURES; f++)
    if (f < sp.n_feat) out[f] = state_feature(o, sp, f);
}

// ExecutionTask.actions of one env: the action table's row t, or on the horizon's last step
// (remaining time o[0] == 1) the whole remaining quantity at allocation (1, 0).  PyTorch on the
// device divides a tensor by a Python scalar as a multiplication by the scalar's reciprocal (the
// true-division kernel's CPU-scalar case), which rounds differently from x / b.  Only this quantity
// share is computed so (the engine places rint(q0 * x) shares, the same integer either way); the
// state divides truly, see state_of
__device__ inline void action_of(const double* t, const double* o, double q0, double* act) {
  const bool last = o[0] == 1.0;
  act[0] = last ? o[1] * (1.0 / q0) : t[0];
  act[1] = last ? 1.0 : t[1];
  act[2] = last ? 0.0 : t[2];
}
