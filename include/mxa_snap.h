/* mxa_snap.h - env-state snapshots of libmxa handles: the part of the C-ABI of include/mxa.h
 * (which includes this file) that saves, restores and forks envs on the device.  Same
 * conventions: 0 or a negative MXA_E* code, mxa_last_error(h) has the message. */
#ifndef MXA_SNAP_H
#define MXA_SNAP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct mxa_handle mxa_handle;

/* Env-state snapshots: save, restore and fork envs on the device, mid-episode (a stepping
 * simulator's set-state call; the reference has none: its ABIDESEnv only resets from 09:30).
 * Between launches an env's whole state is its env block, the seed word of mxa_write_records and
 * its rows of the book-update log.  A snapshot is n_slots slots of device memory on the handle's
 * device; one slot holds one env: the block (mxa_env_bytes, trace ring included), a 256-byte
 * trailer with the seed word, and, when the handle had a book-update log at create, the log's
 * capacity in records.
 *   slot_of_env [n_envs] (host): -1 = the env takes no part; NULL = the identity map (needs
 *   n_slots >= n_envs).  save copies env e into slot slot_of_env[e] (two envs naming one slot:
 *   MXA_EINVAL); restore copies slot slot_of_env[e] into env e, and many envs may name one slot
 *   (a fork).  Slots and envs are independent: a 2-slot bank can feed 4,096 envs.
 * Either call is one kernel launch on the handle's stream whatever the map and returns after the
 * stream is synchronised, like mxa_reset (mxa_last_kernel_ms: the copy kernel's time).  A restored
 * env is the saved one byte for byte (header,
 * agents, RNG streams and windows, queue, book, order-id counters, the GymKernel step's sticky
 * observation), its seed word and its log records (max of the run's and the kernelStopping pass's
 * counts, capped at the capacity) included; an env with -1 keeps every byte.  After a restore the
 * handle's stop time and exchange-log switch are written again as after mxa_reset, so the current
 * mxa_set_stop_time holds for restored envs, and the handle counts as started (mxa_set_exchange_log).
 * mxa_finalize's results are no part of a snapshot (finalize again); the seeds of the next
 * mxa_reset and the market-maker options are untouched.
 * MXA_EINVAL, with a message in mxa_last_error (of the handle; of NULL when the handle is the null
 * argument) and before any HIP call: null arguments, n_slots <= 0,
 * a map entry < -1 or >= n_slots, a NULL map with too few slots, two envs saving to one slot,
 * restoring a slot never saved, a snapshot created by another handle, a handle whose env bytes,
 * log capacity (mxa_set_book_log reallocates the log) or exchange-log switch differ from those at
 * create.  MXA_EHIP: the allocation failed.  Destroy a snapshot before or after its handle.
 * mxa_snapshot_info: out4 = (slots, bytes per slot, slots filled, 1 if a slot carries log rows). */
typedef struct mxa_snapshot mxa_snapshot;
int mxa_snapshot_create(mxa_handle* h, int32_t n_slots, mxa_snapshot** out);
int mxa_snapshot_save(mxa_handle* h, mxa_snapshot* s, const int32_t* slot_of_env);
int mxa_snapshot_restore(mxa_handle* h, const mxa_snapshot* s, const int32_t* slot_of_env);
int mxa_snapshot_info(const mxa_snapshot* s, int64_t* out4);
void mxa_snapshot_destroy(mxa_snapshot* s);

#ifdef __cplusplus
}
#endif
#endif
