// mxa_bars_kernels.h — time bars of every env from its book-update log in one launch
// (include/mxa_bars.h): the argument checks and the size, grid and bar-index arithmetic in plain C++
// (no HIP types: a CPU program can call them), and the replay kernel.  The replay is
// mxabides.booklog.rows_from_records' (executeOrder, OrderBook.py:172-240, at price-level
// granularity: each level gives min(remaining, level volume) at its price), with the quotes, the
// fills and the counts folded into bars [n_envs][n_bars][12] int64 instead of book_log rows.
#ifndef MXA_BARS_KERNELS_H
#define MXA_BARS_KERNELS_H
#include <cstdint>

namespace mxa_bars {

constexpr int32_t WORDS = 12;          // int64 words of a bar (MXA_BAR_WORDS)
constexpr int32_t STATUS_WORDS = 4;    // int32 words of an env's status (MXA_BAR_STATUS_WORDS)
constexpr int32_t MAX_LEVELS = 1024;   // live levels per side the LDS table holds (MXA_BAR_MAX_LEVELS)
constexpr int32_t MAX_BARS = 1 << 24;
constexpr int32_t BAR_BYTES = WORDS * 8;
constexpr int32_t PIECES = BAR_BYTES / 16;  // a bar is written as six 16-byte stores
constexpr int32_t REC_BYTES = 16;           // mxa_book_rec
constexpr int WAVE = 64;
constexpr int MAX_GRID_Y = 65535;
constexpr int CHUNKS = 4;  // record chunks of 64 in flight before the first one is consumed
enum { ST_OK = 0, ST_LOG_OVERFLOW = 1, ST_LEVELS = 2, ST_STREAM = 3 };
// record classes (mxabides.booklog.book_mask; include/mxa.h MXA_BL_*)
constexpr int32_t FLOG_HI = -2147483647 - 1 + 2;  // prices up to here are f_log records
constexpr int32_t EV_RX = -2147483647 - 1 + 256, EV_NT = EV_RX + 256, EV_PLACE = EV_RX + 512, EV_END = EV_RX + 768;
constexpr int32_t K_LIMIT = 11, K_CANCEL = 12;  // the RX codes that carry an order
constexpr int32_t MODIFY = 1 << 30;

// what mxa_write_bars / mxa_read_bars refuse about the handle, before any HIP call: NULL when it is
// good, else what is wrong with it
inline const char* check_handle(bool have_handle, bool gym, bool have_log) {
  if (!have_handle) return "null handle";
  if (gym) return "a GymKernel handle carries no book-update log";
  if (!have_log) return "no book-update log (mxa_set_book_log first)";
  return nullptr;
}
// the grid and the output array (every entry point)
inline const char* check_grid(int64_t t0, int64_t dt, int32_t n_bars, bool have_bars, bool aligned) {
  if (dt <= 0) return "dt_ns <= 0";
  if (n_bars < 1) return "n_bars < 1";
  if (n_bars > MAX_BARS) return "n_bars > 1 << 24";
  if (t0 < 0) return "t0_ns < 0";
  if (dt > (INT64_MAX - t0) / n_bars) return "t0 + n_bars * dt beyond int64";
  if (!have_bars) return "null bars array";
  if (!aligned) return "bars array not 16-byte aligned";
  return nullptr;
}
// the caller's record arrays (mxa_bars_from_records)
inline const char* check_records(int32_t n_envs, bool have_rec, int64_t rec_stride, bool have_count, int32_t level_cap) {
  if (n_envs < 1) return "n_envs < 1";
  if (rec_stride < 1) return "rec_stride < 1";
  if (level_cap < 1) return "level_cap < 1";
  if (level_cap > MAX_LEVELS) return "level_cap > 1024";
  if (!have_rec) return "null records";
  if (!have_count) return "null counts";
  return nullptr;
}

// 64-bit throughout: 4,096 envs x 23,400 bars x 96 B is 9.2 GB
constexpr int64_t bars_bytes(int64_t n_envs, int32_t n_bars) { return n_envs * (int64_t)n_bars * BAR_BYTES; }
constexpr int64_t status_bytes(int64_t n_envs) { return n_envs * STATUS_WORDS * (int64_t)sizeof(int32_t); }
// first word of (env, bar)
constexpr int64_t word_of(int64_t env, int64_t bar, int32_t n_bars) { return (env * n_bars + bar) * WORDS; }
// the grid's end (check_grid has shown that it fits)
constexpr int64_t end_ns(int64_t t0, int64_t dt, int32_t n_bars) { return t0 + (int64_t)n_bars * dt; }
// the bar a time falls in: -1 before t0, n_bars and up at or past the end
constexpr int64_t bar_index(int64_t t, int64_t t0, int64_t dt) { return t < t0 ? -1 : (t - t0) / dt; }

// the level table: slots per side (whole rows of 64, lane l owning l, l + 64, ...) and its dynamic LDS
// (an int64 volume and an int32 price a slot, both sides)
constexpr int32_t slots(int32_t level_cap) { return (level_cap + WAVE - 1) / WAVE * WAVE; }
constexpr int64_t lds_bytes(int32_t level_cap) { return (int64_t)slots(level_cap) * 2 * 12; }
// a handle's level_cap: live levels never exceed resting orders
constexpr int32_t handle_level_cap(bool replay, int32_t ocap) {
  return replay || ocap > MAX_LEVELS ? MAX_LEVELS : ocap < 1 ? WAVE : slots(ocap);
}

// the grid: one wave per env in blockIdx.y, grid-strided above 65,535
constexpr int grid_y(int64_t n_envs) { return n_envs < 1 ? 0 : n_envs > MAX_GRID_Y ? MAX_GRID_Y : (int)n_envs; }

}  // namespace mxa_bars

#ifdef __HIPCC__
namespace mxa_bars {

constexpr int32_t FREE = -1;  // price of a free slot (a level's price is >= 0)

__device__ __forceinline__ int32_t uni(int32_t v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int64_t uni64(int64_t v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(uint64_t)v);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)v >> 32));
  return (int64_t)((uint64_t)hi << 32 | lo);
}
__device__ __forceinline__ void put16(int64_t* p, int64_t a, int64_t b) {
  longlong2 v;
  v.x = a;
  v.y = b;
  *(longlong2*)p = v;
}

// The book of one env.  The table is in LDS, unsorted: vol[side * S + slot], px[side * S + slot]
// (FREE: no level).  Everything else is the same in every lane: per side the live levels, the slots
// below `hi` that were ever taken since the side was last empty (the rows a search walks), the peak,
// and the best level's price, slot and volume (the table's copy of that volume is kept current).
struct Book {
  int64_t* vol;
  int32_t* px;
  int32_t S, cap, lane;
  int32_t n[2], hi[2], peak[2], bp[2], bs[2];
  int64_t bv[2];
};
// words 4-11 of the open bar
struct Acc {
  int32_t open, high, low, close, execs, recs;
  int64_t shares, notional;
};
// words 0-3: the inside quotes, (0, 0) for an empty side
struct Quotes {
  int64_t bid, bid_vol, ask, ask_vol;
};

__device__ __forceinline__ void set_vol(Book& B, int side, int32_t slot, int64_t v) {
  if (B.lane == 0) B.vol[side * B.S + slot] = v;
  __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ void set_px(Book& B, int side, int32_t slot, int32_t p) {
  if (B.lane == 0) B.px[side * B.S + slot] = p;
  __builtin_amdgcn_wave_barrier();
}

// the slot of `price` on a side or -1, by compare and ballot over the rows in use; free_slot: the
// lowest free slot below cap (the row after them when they are full), -1 when there is none
template <int SD>
__device__ __forceinline__ int32_t find(const Book& B, int32_t price, int32_t& free_slot) {
  free_slot = -1;
  const int32_t rows = (B.hi[SD] + WAVE - 1) / WAVE;
  for (int32_t j = 0; j < rows; j++) {
    const int32_t s = j * WAVE + B.lane;
    const int32_t p = B.px[SD * B.S + s];
    const uint64_t eq = __ballot(p == price);
    if (eq) return j * WAVE + (int32_t)__builtin_ctzll(eq);
    if (free_slot < 0) {
      const uint64_t fr = __ballot(p == FREE && s < B.cap);
      if (fr) free_slot = j * WAVE + (int32_t)__builtin_ctzll(fr);
    }
  }
  if (free_slot < 0 && rows * WAVE < B.cap) free_slot = rows * WAVE;
  return -1;
}

// the side's best level from the table: every lane's best (order-preserving key, slot) over its
// slots, a 6-step xor butterfly of maxima (no atomics: the same bits every time)
template <int SD>
__device__ __forceinline__ void find_best(Book& B) {
  if (B.n[SD] == 0) {
    B.hi[SD] = 0;  // every slot is free again
    return;
  }
  int64_t key = INT64_MIN;
  const int32_t rows = (B.hi[SD] + WAVE - 1) / WAVE;
  for (int32_t j = 0; j < rows; j++) {
    const int32_t s = j * WAVE + B.lane;
    const int32_t p = B.px[SD * B.S + s];
    // bids: the price; asks: its complement, so the best level is the maximum on both sides
    const int64_t k = (int64_t)(SD == 0 ? p : ~p) * 65536 + s;
    key = p != FREE && k > key ? k : key;
  }
#pragma unroll
  for (int off = WAVE / 2; off > 0; off >>= 1) {
    const int64_t o = __shfl_xor(key, off, WAVE);
    key = o > key ? o : key;
  }
  key = uni64(key);
  const int32_t slot = (int32_t)(key & 0xFFFF), k = (int32_t)(key >> 16);
  B.bs[SD] = slot;
  B.bp[SD] = SD == 0 ? k : ~k;
  B.bv[SD] = uni64(B.vol[SD * B.S + slot]);
}

template <int SD>
__device__ __forceinline__ void remove_best(Book& B) {
  set_px(B, SD, B.bs[SD], FREE);
  B.n[SD]--;
  find_best<SD>(B);
}

// a level's volume changes by delta (a cancellation: delta < 0 and the level goes at 0; modifyOrder:
// the level stays); ST_STREAM when the level is not there or holds less
template <int SD>
__device__ __forceinline__ int change(Book& B, int32_t price, int64_t delta, bool remove_at_zero) {
  if (B.n[SD] > 0 && B.bp[SD] == price) {
    const int64_t v = B.bv[SD] + delta;
    if (v < 0) return ST_STREAM;
    if (v == 0 && remove_at_zero) {
      remove_best<SD>(B);
    } else {
      B.bv[SD] = v;
      set_vol(B, SD, B.bs[SD], v);
    }
    return ST_OK;
  }
  int32_t fr;
  const int32_t slot = find<SD>(B, price, fr);
  if (slot < 0) return ST_STREAM;
  const int64_t v = uni64(B.vol[SD * B.S + slot]) + delta;
  if (v < 0) return ST_STREAM;
  if (v == 0 && remove_at_zero) {
    set_px(B, SD, slot, FREE);
    B.n[SD]--;
  } else {
    set_vol(B, SD, slot, v);
  }
  return ST_OK;
}

// a limit order of q shares resting on side OWN: matched best-first against the other side while the
// price crosses, the remainder rests; ST_LEVELS when the remainder would be level cap + 1
template <int OWN>
__device__ __forceinline__ int limit(Book& B, Acc& A, int32_t price, int64_t q) {
  constexpr int OPP = 1 - OWN;
  bool traded = false;
  while (q > 0 && B.n[OPP] > 0 && (OWN == 0 ? B.bp[OPP] <= price : B.bp[OPP] >= price)) {
    const int64_t v = B.bv[OPP], c = q >= v ? v : q;
    const int32_t p = B.bp[OPP];
    q -= c;
    if (c > 0) {
      if (A.shares == 0) A.open = A.high = A.low = p;
      A.high = p > A.high ? p : A.high;
      A.low = p < A.low ? p : A.low;
      A.close = p;
      A.shares += c;
      A.notional += (int64_t)p * c;
      traded = true;
    }
    if (c == v) {
      remove_best<OPP>(B);
    } else {
      B.bv[OPP] = v - c;
      set_vol(B, OPP, B.bs[OPP], v - c);
    }
  }
  A.execs += traded ? 1 : 0;
  if (q == 0) return ST_OK;
  if (B.n[OWN] > 0 && B.bp[OWN] == price) {
    B.bv[OWN] += q;
    set_vol(B, OWN, B.bs[OWN], B.bv[OWN]);
    return ST_OK;
  }
  int32_t fr;
  const int32_t slot = find<OWN>(B, price, fr);
  if (slot >= 0) {
    set_vol(B, OWN, slot, uni64(B.vol[OWN * B.S + slot]) + q);
    return ST_OK;
  }
  if (B.n[OWN] >= B.cap || fr < 0 || fr >= B.cap) return ST_LEVELS;
  set_px(B, OWN, fr, price);
  set_vol(B, OWN, fr, q);
  const bool better = B.n[OWN] == 0 || (OWN == 0 ? price > B.bp[OWN] : price < B.bp[OWN]);
  B.n[OWN]++;
  B.hi[OWN] = fr + 1 > B.hi[OWN] ? fr + 1 : B.hi[OWN];
  B.peak[OWN] = B.n[OWN] > B.peak[OWN] ? B.n[OWN] : B.peak[OWN];
  if (better) {
    B.bp[OWN] = price;
    B.bs[OWN] = fr;
    B.bv[OWN] = q;
  }
  return ST_OK;
}

// one book-changing record
__device__ __forceinline__ int apply(Book& B, Acc& A, int32_t p, int32_t q) {
  if (p >= 0) return q > 0 ? limit<0>(B, A, p, (int64_t)q) : limit<1>(B, A, p, -(int64_t)q);
  const int32_t np = -p;  // p is above the f_log prices, so this fits
  if (np & MODIFY) {
    const int32_t price = np & ((1 << 29) - 1);
    return (np >> 29) & 1 ? change<1>(B, price, (int64_t)q, false) : change<0>(B, price, (int64_t)q, false);
  }
  return q > 0 ? change<0>(B, np, -(int64_t)q, true) : change<1>(B, np, (int64_t)q, true);
}

// bar `bar` of the env whose bars start at `out`: the quotes and the open bar's words, lanes 0-5 one
// 16-byte store each
__device__ __forceinline__ void put_bar(int64_t* out, int64_t bar, const Quotes qt, const Acc& A, int lane) {
  const int64_t a = lane == 0 ? qt.bid : lane == 1 ? qt.ask : lane == 2 ? A.open : lane == 3 ? A.low : lane == 4 ? A.shares : A.execs;
  const int64_t b = lane == 0 ? qt.bid_vol : lane == 1 ? qt.ask_vol : lane == 2 ? A.high : lane == 3 ? A.close : lane == 4 ? A.notional : A.recs;
  if (lane < PIECES) put16(out + bar * WORDS + lane * 2, a, b);
}
// bars [from, to) without a record: the quotes carried forward, zeros after them; the 16-byte pieces of
// the run side by side over the lanes (at most 2^24 bars x 6 pieces: 32-bit piece indices)
__device__ __forceinline__ void put_run(int64_t* out, int64_t from, int64_t to, const Quotes qt, int lane) {
  if (to <= from) return;
  const uint32_t total = (uint32_t)(to - from) * PIECES;
  int64_t* base = out + from * WORDS;
  for (uint32_t i = lane; i < total; i += WAVE) {
    const uint32_t pc = i % PIECES;
    const int64_t a = pc == 0 ? qt.bid : qt.ask, b = pc == 0 ? qt.bid_vol : qt.ask_vol;
    put16(base + (int64_t)i * 2, pc < 2 ? a : 0, pc < 2 ? b : 0);
  }
}
__device__ __forceinline__ Quotes quotes(const Book& B) {
  Quotes q;
  q.bid = B.n[0] > 0 ? B.bp[0] : 0;
  q.bid_vol = B.n[0] > 0 ? B.bv[0] : 0;
  q.ask = B.n[1] > 0 ? B.bp[1] : 0;
  q.ask_vol = B.n[1] > 0 ? B.bv[1] : 0;
  return q;
}

}  // namespace mxa_bars

// One wave per env (blockIdx.y, grid-strided).  Env e's records start at rec_base + e * rec_stride
// bytes, rec_cap of them at most; their count is the larger of the int32 words at cnt0 and cnt1
// + e * cnt_stride bytes (a handle: EnvHdr::blog_n and blog_fin in the env block; caller-given counts:
// both the same word).  The lanes load 64 records with one 16-byte load each, CHUNKS chunks ahead of
// the one being consumed (one wave hides no latency by itself), classify them side by side (the
// "record after an order-carrying code" rule is the ballot shifted by one lane, its top bit carried
// into the next chunk) and the wave walks the book-changing ones of the ballot mask serially, their
// words read with readlane.  Every branch of the walk is on wave-uniform values.
__global__ __launch_bounds__(mxa_bars::WAVE) void mxa_bars_kernel(const char* rec_base, int64_t rec_stride, int64_t rec_cap,
                                                                    const char* cnt0, const char* cnt1, int64_t cnt_stride,
                                                                    int n_envs, int32_t level_cap, int64_t t0, int64_t dt,
                                                                    int32_t n_bars, int64_t* bars, int32_t* status) {
  using namespace mxa_bars;
  extern __shared__ int64_t mxa_bars_lds[];
  const int lane = threadIdx.x;
  Book B;
  B.S = slots(level_cap);
  B.cap = level_cap;
  B.lane = lane;
  B.vol = mxa_bars_lds;
  B.px = (int32_t*)(mxa_bars_lds + 2 * B.S);
  const int64_t end = end_ns(t0, dt, n_bars);
  for (int env = blockIdx.y; env < n_envs; env += gridDim.y) {
    for (int32_t s = lane; s < 2 * B.S; s += WAVE) B.px[s] = FREE;
    __builtin_amdgcn_wave_barrier();
    for (int sd = 0; sd < 2; sd++) B.n[sd] = B.hi[sd] = B.peak[sd] = B.bp[sd] = B.bs[sd] = 0, B.bv[sd] = 0;
    Acc A = Acc{0, 0, 0, 0, 0, 0, 0, 0};
    int64_t* out = bars + word_of(env, 0, n_bars);
    const int4* rec = (const int4*)(rec_base + (int64_t)env * rec_stride);
    const int32_t c0 = uni(*(const int32_t*)(cnt0 + (int64_t)env * cnt_stride));
    const int32_t c1 = uni(*(const int32_t*)(cnt1 + (int64_t)env * cnt_stride));
    const int64_t count = c0 > c1 ? c0 : c1;
    const int64_t n = count < 0 ? 0 : count > rec_cap ? rec_cap : count;
    auto load = [&](int64_t i) { return i < n ? rec[i] : make_int4(0, 0, 0, 0); };
    int4 r[CHUNKS];
#pragma unroll
    for (int u = 0; u < CHUNKS; u++) r[u] = load((int64_t)u * WAVE + lane);
    int64_t open_bar = -1, bar_end = t0, consumed = n;  // bar_end: the end of the open bar (t0: none is open)
    int code = ST_OK;
    uint64_t carry = 0;  // the last record of the chunk before carried an order
    bool go = true;
    for (int64_t base = 0; go && base < n; base += CHUNKS * WAVE) {
#pragma unroll
      for (int u = 0; u < CHUNKS; u++) {
        const int64_t cb = base + (int64_t)u * WAVE;
        if (!go || cb >= n) break;
        const int4 cur = r[u];
        r[u] = load(cb + CHUNKS * WAVE + lane);
        const bool valid = cb + lane < n;
        const int32_t pr = cur.z;
        const bool code_rec = pr >= EV_RX && pr < EV_END;
        const uint64_t ho = __ballot(valid && (pr == EV_RX + K_LIMIT || pr == EV_RX + K_CANCEL || (pr >= EV_NT && pr < EV_PLACE)));
        uint64_t m = __ballot(valid && pr > FLOG_HI && !code_rec) & ~(ho << 1 | carry);
        carry = ho >> 63;
        while (m) {
          const int l = (int)__builtin_ctzll(m);
          m &= m - 1;
          const int64_t t = (int64_t)((uint64_t)(uint32_t)__builtin_amdgcn_readlane(cur.y, l) << 32 |
                                      (uint32_t)__builtin_amdgcn_readlane(cur.x, l));
          const int32_t p = __builtin_amdgcn_readlane(cur.z, l), q = __builtin_amdgcn_readlane(cur.w, l);
          if (t >= end) {
            consumed = cb + l;
            go = false;
            break;
          }
          if (t >= bar_end) {  // a later bar opens (t >= t0 here): the open one and the empty ones before it close
            const int64_t idx = (t - t0) / dt;
            const Quotes qt = quotes(B);
            if (open_bar >= 0) put_bar(out, open_bar, qt, A, lane);
            put_run(out, open_bar + 1, idx, qt, lane);
            open_bar = idx;
            bar_end = t0 + (idx + 1) * dt;
            A = Acc{0, 0, 0, 0, 0, 0, 0, 0};
          }
          code = apply(B, A, p, q);
          if (code != ST_OK) {
            consumed = cb + l;
            go = false;
            break;
          }
          A.recs++;
        }
      }
    }
    if (code == ST_OK) {
      const Quotes qt = quotes(B);
      if (open_bar >= 0) put_bar(out, open_bar, qt, A, lane);
      put_run(out, open_bar + 1, n_bars, qt, lane);
      code = count > rec_cap ? ST_LOG_OVERFLOW : ST_OK;
    } else {  // nothing is invented: the bar the record falls in and every later one are zero rows
      put_run(out, open_bar < 0 ? 0 : open_bar, n_bars, Quotes{0, 0, 0, 0}, lane);
    }
    if (status && lane < STATUS_WORDS)
      status[(int64_t)env * STATUS_WORDS + lane] = lane == 0 ? code : lane == 1 ? (int32_t)consumed : lane == 2 ? B.peak[0] : B.peak[1];
  }
}
#endif  // __HIPCC__

#endif
