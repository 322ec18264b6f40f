/* mxa_policy_features.h - the closed-loop step with a state of N features: the part of the C-ABI of
 * include/mxa.h (which includes this file) that runs mxa_step_policy with the learner's state given as
 * a spec (include/mxa_state_spec.h), so the policy inside the step kernel can see the market columns
 * of the observation row.  Same conventions: 0 or a negative MXA_E* code, mxa_last_error(h) has the
 * message. */
#ifndef MXA_POLICY_FEATURES_H
#define MXA_POLICY_FEATURES_H
#include <stdint.h>

#include "mxa_state_spec.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct mxa_handle mxa_handle;
typedef struct mxa_policy mxa_policy;

/* k periods of every env in one launch with the epsilon-greedy Q-network policy evaluated in place:
 * the contract of mxa_step_policy (include/mxa.h), word for word, with three differences.  The state
 * x the network reads is the spec's state of the env's own stored observation (x [n_feat] f32, feature
 * f on lane f of the env's wave); p->grid0, grid1, n0, n1 and nh are unread; and p->dims[0] must
 * equal spec->n_feat.  Bit for bit the sequence mxa_ddqn_state_spec (include/mxa_ddqn_features.h),
 * mxa_qnet_act, mxa_step_device, mxa_write_rl_state per period.  `spec` is a HOST struct read during
 * the call; its `grid` is a DEVICE pointer, which the caller keeps alive until the launch has run.
 * The outputs, first_zero and the stream are mxa_step_policy's.
 * MXA_EINVAL with a message, before any HIP call: what mxa_step_policy refuses (but for the grids and
 * dims[0] != 2), a spec that mxa_state_spec_refusal(spec, 9) refuses (a null one included), and
 * p->dims[0] != spec->n_feat. */
int mxa_step_policy_spec(mxa_handle* h, int32_t k, int32_t first_zero, const mxa_policy* p, const mxa_state_spec* spec,
                         double* d_obs, int32_t* d_flags, int64_t* d_a, double* d_act, double* d_state);

#ifdef __cplusplus
}
#endif
#endif
