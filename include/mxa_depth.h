/* mxa_depth.h - L2 book depth of libmxa handles: the part of the C-ABI of include/mxa.h (which
 * includes this file) that writes the top price levels of every env's book in one kernel launch.
 * Same conventions: 0 or a negative MXA_E* code, mxa_last_error(h) has the message. */
#ifndef MXA_DEPTH_H
#define MXA_DEPTH_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct mxa_handle mxa_handle;

/* Book depth: OrderBook.getInsideBids(depth) / getInsideAsks(depth) (util/OrderBook.py:377-398) of
 * every env of a handle at once.
 *   d_depth [n_envs][2][levels][2] int64 in DEVICE memory: side 0 is bids, side 1 is asks; row i of a
 *   side is (price, total shares) of its i-th best level (bids descending, asks ascending), the
 *   total being the sum of the quantities of every order resting at that price, which is what the
 *   reference's loop returns.  Totals are 64-bit: a replay level can exceed 2^32 shares.
 *   d_counts [n_envs][2] int32 = min(levels, non-empty levels on the side); may be NULL.
 * Rows from the count on are written as (0, 0), so the caller's buffer need not be cleared, and the
 * call writes nothing outside the two arrays.
 * mxa_write_depth is one kernel launch, asynchronous on the handle's stream like mxa_write_records:
 * it sees the books as the last launch queued before it leaves them and returns without
 * synchronising.  mxa_read_depth is the same into HOST arrays under the readers' contract of mxa.h:
 * a stream-ordered temporary (freed on every return path) and a copy on the handle's stream, the way
 * mxa_read_counters works, and then it synchronises.
 * Every handle kind holds one exchange book, so both work on all of them: Kernel.runner handles
 * (mxa_create, _hist, _params, _config), GymKernel handles (rmsc03 + DummyRL, the replay), the replay
 * runner and the TWAP handles.  An env that has finished, errored or never run reports the book that
 * stands in its block; a freshly reset env has counts 0.
 * MXA_EINVAL, with a message in mxa_last_error and before any HIP call: null handle, null d_depth /
 * depth, levels < 1, or levels > 1 << 20 (the widest ladder the replay layout allows). */
int mxa_write_depth(mxa_handle* h, int32_t levels, int64_t* d_depth, int32_t* d_counts);
int mxa_read_depth(mxa_handle* h, int32_t levels, int64_t* depth, int32_t* counts);

#ifdef __cplusplus
}
#endif
#endif
