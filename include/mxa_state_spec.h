/* mxa_state_spec.h - the DDQN learner's state as a list of features of the observation row: the one
 * definition shared by libmxa.so (include/mxa_policy_features.h, the policy inside the step kernel)
 * and libmxa_ddqn_features.so (include/mxa_ddqn_features.h, the per-period kernels).
 *
 * Feature f reads one observation column, scales it, and either bins it on its own split points or
 * passes it through:
 *   x_f = mul[f] * (obs[col[f]] / div[f]) + add[f]     (f64; a true division, no contraction)
 *   n_f = goff[f + 1] - goff[f]
 *   state[f] = n_f > 0 ? (float)upper_bound(x_f, grid + goff[f], n_f) : (float)x_f
 * upper_bound is the number of split points <= x_f with NaN sorting last: np.digitize on increasing
 * points, torch.bucketize(right=True).  A feature without split points gives the network x_f itself,
 * a continuous input.
 *
 * The default spec, (col 0, mul 2, div nh, add -1) and (col 1, mul 2, div q0, add -1) on
 * ExecutionTask's two 199-point grids, gives the states of mxa_ddqn_state bit for bit:
 * 2 * (o / nh) + (-1.0) and 2 * (o / nh) - 1.0 are the same IEEE operation. */
#ifndef MXA_STATE_SPEC_H
#define MXA_STATE_SPEC_H
#include <math.h>
#include <stdint.h>

#define MXA_STATE_MAX_FEATURES 8
#define MXA_STATE_MAX_POINTS (1 << 20) /* split points of all features together */

typedef struct mxa_state_spec {
  int32_t n_feat;                /* 1..8 */
  int32_t col[8];                /* observation column of feature f */
  double mul[8], div[8], add[8]; /* x_f = mul * (obs[col] / div) + add: a true division, no contraction */
  const double* grid;            /* DEVICE: every feature's split points, concatenated, increasing per feature */
  int32_t goff[9];               /* feature f's points are grid[goff[f] .. goff[f+1]) ; goff[0] == 0 */
} mxa_state_spec;

/* What both libraries refuse, on the host and before any HIP call: null when the spec is usable on
 * observation rows of obs_w columns, else the reason.  Refused: a null spec, n_feat outside 1..8, a
 * column < 0 or >= obs_w, a zero or non-finite div, a non-finite mul or add, goff[0] != 0, a
 * decreasing goff, more than MXA_STATE_MAX_POINTS points, a null grid with points to read.  (That
 * each feature's points increase is the caller's to keep: they live on the device.) */
static inline const char* mxa_state_spec_refusal(const mxa_state_spec* sp, int32_t obs_w) {
  if (!sp) return "null state spec";
  if (sp->n_feat < 1 || sp->n_feat > MXA_STATE_MAX_FEATURES) return "n_feat outside 1..8";
  if (sp->goff[0] != 0) return "goff[0] != 0";
  for (int f = 0; f < sp->n_feat; f++) {
    if (sp->col[f] < 0 || sp->col[f] >= obs_w) return "a feature's column outside the observation row";
    if (!isfinite(sp->div[f]) || sp->div[f] == 0.0) return "a zero or non-finite div";
    if (!isfinite(sp->mul[f]) || !isfinite(sp->add[f])) return "a non-finite mul or add";
    if (sp->goff[f + 1] < sp->goff[f]) return "a decreasing goff";
    if (sp->goff[f + 1] > MXA_STATE_MAX_POINTS) return "more than 1 << 20 split points";
  }
  if (sp->goff[sp->n_feat] > 0 && !sp->grid) return "a null grid with split points to read";
  return 0;
}
#endif
