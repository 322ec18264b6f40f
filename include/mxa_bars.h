/* mxa_bars.h - time bars from the book-update log: the part of the C-ABI of include/mxa.h (which
 * includes this file) that replays every env's record stream (mxa_book_rec, mxa_set_book_log) on the
 * device into quotes, trade OHLC, volume and counts on a time grid, one kernel launch for all envs.
 * Same conventions: 0 or a negative MXA_E* code, mxa_last_error(h) has the message. */
#ifndef MXA_BARS_H
#define MXA_BARS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct mxa_handle mxa_handle;

#define MXA_BAR_WORDS 12
#define MXA_BAR_STATUS_WORDS 4
#define MXA_BAR_MAX_LEVELS 1024 /* live price levels per side the replay holds */

/* The replay is the one of mxabides.booklog.rows_from_records, at price-level granularity, which is
 * exact: executeOrder (OrderBook.py:172-240) fills an incoming order from the best opposite level
 * while its price crosses, each level giving min(remaining, level volume) at the level's price.
 *   d_bars [n_envs][n_bars][12] int64 in DEVICE memory, 16-byte aligned.  Bar i covers
 *   [t0 + i * dt, t0 + (i + 1) * dt) in ns since the simulated midnight:
 *     0-3   best bid price, its total shares, best ask price, its total shares: the book as it
 *           stands after the last book-changing record with t below the bar's end (cancellations and
 *           modifies count); (0, 0) for an empty side
 *     4-7   open, high, low, close over the bar's fills in order (a fill: one level's
 *           min(remaining, level volume) at that level's price); 0 without a trade
 *     8     shares executed          9   sum of price * shares (VWAP = word 9 / word 8)
 *     10    limit orders that executed at all (the orders with a LAST_TRADE row)
 *     11    book-changing records in the bar: limit, cancel and modify
 *   A bar without records carries the quotes forward with zeros in words 4-11; bars before the first
 *   record are all 0.  Records with t < t0 change the book and count in no bar; the replay stops at
 *   the first book-changing record with t >= t0 + n_bars * dt.  The bar index never goes back: a
 *   record earlier than its predecessor lands in the open bar.
 *   d_status [n_envs][4] int32, may be NULL: code, records consumed (every kind, up to where the
 *   replay stopped: the index of the record it stopped at, else all of them), peak live bid levels,
 *   peak live ask levels.  Codes:
 *     0 ok
 *     1 the env's log overflowed (count > capacity): the bars are those of the first `capacity` records
 *     2 a side would need more than level_cap live levels
 *     3 the stream contradicts itself: a cancel or modify of a level that is not there, or one that
 *       takes more than the level holds
 *   On 2 or 3 the replay stops at that record: the bars before the one the record falls in keep their
 *   rows, that bar and every later one are zero rows.
 * Record classes (mxabides.booklog.book_mask): prices in [-2^31, -2^31 + 2] (f_log) and in
 * [MXA_BL_EV_RX, MXA_BL_EV_END) (the exchange's log) are skipped, and so is the record after an
 * order-carrying code (RX + 11, RX + 12, every NT code) whatever it holds.  Of the others price < 0
 * with bit 30 of -price set is modifyOrder (side bit 29, price the low 29 bits, the level's volume
 * changes by qty and the level stays), any other price < 0 a cancellation (qty > 0: the bid side; the
 * level loses |qty| and disappears at 0), price >= 0 a limit order.
 *
 * mxa_write_bars is one kernel launch, asynchronous on the handle's stream like mxa_write_depth: it
 * reads each env's record count from the env header on the device, so between two launches
 * mid-episode it sees the records so far, and it returns without synchronising.  mxa_read_bars is the
 * same into HOST arrays under the readers' contract of mxa.h (a stream-ordered temporary, freed on every
 * return path, a copy, one synchronise).  Both work on every
 * handle that carries a book-update log: Kernel.runner handles, the replay runner and the TWAP
 * handles.  level_cap is MXA_BAR_MAX_LEVELS on the replay handles, else the book capacity rounded up
 * to 64 and capped at MXA_BAR_MAX_LEVELS (live levels never exceed resting orders).
 * mxa_bars_from_records is the kernel on caller-given DEVICE arrays, asynchronous on `stream` (a
 * hipStream_t; null: the default stream) of the current device: env e's records start at
 * d_rec + e * rec_stride, their count is d_count[e] and their capacity rec_stride.
 * MXA_EINVAL, with a message in mxa_last_error and before any HIP call: null handle, a GymKernel
 * handle, a handle without a book-update log, dt_ns <= 0, n_bars < 1 or > 1 << 24, t0_ns < 0,
 * t0 + n_bars * dt beyond int64, null or misaligned d_bars / bars; _from_records: n_envs < 1,
 * rec_stride < 1, level_cap < 1 or > MXA_BAR_MAX_LEVELS, null records or counts. */
int mxa_write_bars(mxa_handle* h, int64_t t0_ns, int64_t dt_ns, int32_t n_bars, int64_t* d_bars, int32_t* d_status);
int mxa_read_bars(mxa_handle* h, int64_t t0_ns, int64_t dt_ns, int32_t n_bars, int64_t* bars, int32_t* status);
int mxa_bars_from_records(void* stream, int32_t n_envs, const mxa_book_rec* d_rec, int64_t rec_stride,
                          const int32_t* d_count, int32_t level_cap, int64_t t0_ns, int64_t dt_ns, int32_t n_bars,
                          int64_t* d_bars, int32_t* d_status);

#ifdef __cplusplus
}
#endif
#endif
