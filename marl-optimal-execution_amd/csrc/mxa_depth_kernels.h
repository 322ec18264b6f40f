// mxa_depth_kernels.h — L2 book depth of every env in one launch (include/mxa_depth.h;
// OrderBook.getInsideBids / getInsideAsks, OrderBook.py:377-398): the argument check and the size
// and grid arithmetic in plain C++ (no HIP types: a CPU program can call them), and the two kernels,
// one per book format.  Both formats are at rest in the env block between launches:
//   the slot book   SavedOrder[ocap] at Layout::off_book, unsorted, a free slot has meta < 0 (every
//                   handle without the replay ladder)
//   the ladder      RpHdr::best / nlev in the block's header copy, the per-level order counts at
//                   RpLayout::off_lvc (int32 [2][P]) and quantities at off_lvq (int64 [2][P])
// Output: depth [n_envs][2][levels][2] int64, side 0 bids / 1 asks, row i = (price, total shares) of
// the i-th best level, rows from the count on (0, 0); counts [n_envs][2] int32 (may be NULL).
#ifndef MXA_DEPTH_KERNELS_H
#define MXA_DEPTH_KERNELS_H
#include <cstdint>

namespace mxa_depth {

constexpr int32_t MAX_LEVELS = 1 << 20;  // the widest ladder the replay layout allows
constexpr int32_t MAX_OCAP = 1024;       // 16 book slots per lane: what the slot kernel's LDS holds
constexpr int32_t ROW_BYTES = 16;        // (price, total) int64
constexpr int WAVE = 64;
constexpr int MAX_GRID_Y = 65535;
constexpr int STRIDES = 4;  // ladder kernel: count loads of 4 x 64 levels in flight before the first ballot

// everything mxa_write_depth / mxa_read_depth refuse, before any HIP call: NULL when the arguments
// are good, else what is wrong with them
inline const char* check_args(bool have_handle, bool have_depth, int32_t levels) {
  if (!have_handle) return "null handle";
  if (levels < 1) return "levels < 1";
  if (levels > MAX_LEVELS) return "levels > 1 << 20";
  if (!have_depth) return "null depth array";
  return nullptr;
}

// 64-bit throughout: 65,536 envs x 2^20 levels is 2^41 bytes
constexpr int64_t rows(int64_t n_envs, int32_t levels) { return n_envs * 2 * (int64_t)levels; }
constexpr int64_t depth_bytes(int64_t n_envs, int32_t levels) { return rows(n_envs, levels) * ROW_BYTES; }
constexpr int64_t counts_bytes(int64_t n_envs) { return n_envs * 2 * (int64_t)sizeof(int32_t); }
// first row of (env, side)
constexpr int64_t row_of(int64_t env, int side, int32_t levels) { return (env * 2 + side) * (int64_t)levels; }

// the grid: envs in blockIdx.y, grid-strided above 65,535; the ladder kernel has the side in blockIdx.x
constexpr int grid_y(int64_t n_envs) { return n_envs < 1 ? 0 : n_envs > MAX_GRID_Y ? MAX_GRID_Y : (int)n_envs; }
// envs the block with blockIdx.y = y walks
constexpr int64_t envs_of_block(int64_t n_envs, int y) {
  const int g = grid_y(n_envs);
  return g == 0 || y >= g ? 0 : (n_envs - y + g - 1) / g;
}
// slot kernel: book slots per lane (the last ones partly past ocap), and whether the LDS holds them
constexpr int slots_per_lane(int32_t ocap) { return (ocap + WAVE - 1) / WAVE; }
constexpr bool ocap_ok(int32_t ocap) { return ocap > 0 && ocap <= MAX_OCAP; }
// ladder kernel: levels one round trip covers
constexpr int round_levels() { return STRIDES * WAVE; }

}  // namespace mxa_depth

#ifdef __HIPCC__
namespace mxa_depth {
// one output row; a lane stores it whole (one 16-byte store)
struct alignas(16) Row {
  int64_t price, qty;
};
__device__ __forceinline__ void put_row(Row* p, int64_t price, int64_t qty) {
  longlong2 v;
  v.x = price;
  v.y = qty;
  *(longlong2*)p = v;
}
// a value that is the same in every lane, said to the compiler (the branch on it is a scalar one)
__device__ __forceinline__ int64_t uniform64(int64_t v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(uint64_t)v);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)v >> 32));
  return (int64_t)((uint64_t)hi << 32 | lo);
}
// rows [from, levels) of one side as (0, 0), lanes side by side
__device__ __forceinline__ void zero_rows(Row* out, int64_t from, int64_t levels, int lane) {
  for (int64_t r = from + lane; r < levels; r += WAVE) put_row(out + r, 0, 0);
}
}  // namespace mxa_depth

// The slot book: one wave per env (blockIdx.y, grid-strided).  The lanes load the (price, qty, oid,
// meta) quads of the slots side by side, four 16-byte loads in flight, and keep (price, qty, side) of
// slot j * 64 + lane in LDS (8 bytes a slot, 8 KiB: a dynamic slot index in registers would go to
// scratch).  A lane reads back only what it wrote, so there is no barrier.  Per side, level by level:
// every lane finds the best order-preserving key among its slots' prices strictly worse than the last
// level taken, and the quantity it holds at that key; a 6-step xor butterfly of (key, 64-bit sum)
// merges them (equal keys add, else the better key wins: commutative and associative, no atomics, so
// the same bits every time and the same value in every lane).  Lane i & 63 keeps level i's row and the
// wave stores up to 64 rows side by side, the (0, 0) rows past the count the same way.
__global__ __launch_bounds__(mxa_depth::WAVE) void mxa_depth_slots_kernel(const char* env_base, uint64_t env_stride,
                                                                            uint32_t off_book, int32_t ocap, int n_envs,
                                                                            int32_t levels, mxa_depth::Row* depth,
                                                                            int32_t* counts) {
  using namespace mxa_depth;
  __shared__ uint2 slot[MAX_OCAP];  // x: price; y: 0xFFFFFFFF free, else is_buy << 31 | qty
  const int lane = threadIdx.x;
  const int nj = slots_per_lane(ocap);
  constexpr int64_t NONE = INT64_MIN;
  for (int env = blockIdx.y; env < n_envs; env += gridDim.y) {
    const char* book = env_base + (size_t)env * env_stride + off_book;
    for (int j0 = 0; j0 < nj; j0 += 4) {
      int4 v[4];
#pragma unroll
      for (int u = 0; u < 4; u++) {  // a slot past ocap loads the last one again and counts as free
        const int s = (j0 + u) * WAVE + lane;
        v[u] = *(const int4*)(book + (size_t)(s < ocap ? s : ocap - 1) * sizeof(SavedOrder));
      }
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int s = (j0 + u) * WAVE + lane;
        if (j0 + u < nj) {
          const bool live = s < ocap && v[u].w >= 0;
          slot[s] = make_uint2((uint32_t)v[u].x, live ? ((uint32_t)(v[u].w & 1) << 31 | ((uint32_t)v[u].y & 0x7FFFFFFFu))
                                                      : 0xFFFFFFFFu);
        }
      }
    }
    for (int side = 0; side < 2; side++) {
      Row* out = depth + row_of(env, side, levels);
      const uint32_t want = side == 0 ? 1u : 0u;  // bids are the buy orders
      int64_t last = INT64_MAX;                   // key of the last level taken
      int32_t count = 0;
      bool more = true;
      for (int32_t base = 0; base < levels; base += WAVE) {
        const int n = levels - base < WAVE ? levels - base : WAVE;
        int64_t my_p = 0, my_q = 0;
        for (int i = 0; more && i < n; i++) {
          int64_t key = NONE, sum = 0;
          for (int j = 0; j < nj; j++) {
            const uint2 e = slot[j * WAVE + lane];
            // bids: the price; asks: its complement, so the best level is the maximum on both sides
            const int64_t k = side == 0 ? (int64_t)(int32_t)e.x : ~(int64_t)(int32_t)e.x;
            if (e.y != 0xFFFFFFFFu && (e.y >> 31) == want && k < last) {
              const int64_t q = (int64_t)(e.y & 0x7FFFFFFFu);
              sum = k > key ? q : k == key ? sum + q : sum;
              key = k > key ? k : key;
            }
          }
#pragma unroll
          for (int off = WAVE / 2; off > 0; off >>= 1) {
            const int64_t ok = __shfl_xor(key, off, WAVE), os = __shfl_xor(sum, off, WAVE);
            sum = ok > key ? os : ok == key ? sum + os : sum;
            key = ok > key ? ok : key;
          }
          key = uniform64(key);
          if (key == NONE) {
            more = false;
            break;
          }
          if (lane == i) {
            my_p = side == 0 ? key : ~key;
            my_q = sum;
          }
          last = key;
          count++;
        }
        if (lane < n) put_row(out + base + lane, my_p, my_q);
      }
      if (counts && lane == 0) counts[(size_t)env * 2 + side] = count;
    }
  }
}

// The replay ladder: one wave per (env, side) (blockIdx.x the side, blockIdx.y the envs,
// grid-strided).  From RpHdr::best toward worse prices, as lvl_next walks: the order counts of
// 4 x 64 levels are loaded before the first ballot (one wave hides no latency by itself), lanes side
// by side; per 64 levels the non-empty ones are balloted and ranked by the mask's prefix popcount, and
// a ranked lane loads its level's quantity and stores its row at rank.  Stops at min(levels, nlev)
// rows or at the ladder's end.  The FIFO lists are not walked.
__global__ __launch_bounds__(mxa_depth::WAVE) void mxa_depth_ladder_kernel(const char* env_base, uint64_t env_stride,
                                                                             uint64_t off_rh, uint64_t off_lvc,
                                                                             uint64_t off_lvq, int32_t pmin, int32_t P,
                                                                             int n_envs, int32_t levels,
                                                                             mxa_depth::Row* depth, int32_t* counts) {
  using namespace mxa_depth;
  const int lane = threadIdx.x;
  const int side = blockIdx.x;
  for (int env = blockIdx.y; env < n_envs; env += gridDim.y) {
    const char* e = env_base + (size_t)env * env_stride;
    const RpHdr* rh = (const RpHdr*)(e + off_rh);
    const int32_t* cnt = (const int32_t*)(e + off_lvc) + (size_t)side * (size_t)P;
    const int64_t* qty = (const int64_t*)(e + off_lvq) + (size_t)side * (size_t)P;
    Row* out = depth + row_of(env, side, levels);
    const int32_t best = __builtin_amdgcn_readfirstlane(rh->best[side]);
    const int32_t nlev = __builtin_amdgcn_readfirstlane(rh->nlev[side]);
    const int32_t target = best < 0 || best >= P || nlev < 0 ? 0 : nlev < levels ? nlev : levels;
    int32_t done = 0;
    for (int32_t pos = best; done < target && pos >= 0 && pos < P; pos += side == 0 ? -round_levels() : round_levels()) {
      int32_t x[STRIDES], c[STRIDES];
#pragma unroll
      for (int u = 0; u < STRIDES; u++) {  // a level past either end loads `best` again and counts as empty
        x[u] = side == 0 ? pos - (u * WAVE + lane) : pos + (u * WAVE + lane);
        const bool in = x[u] >= 0 && x[u] < P;
        c[u] = cnt[in ? x[u] : best];
        c[u] = in ? c[u] : 0;
      }
#pragma unroll
      for (int u = 0; u < STRIDES; u++) {
        const uint64_t m = __ballot(c[u] > 0);
        const int32_t rank = done + __popcll(m & ((1ull << lane) - 1));
        if (c[u] > 0 && rank < target) put_row(out + rank, (int64_t)pmin + x[u], qty[x[u]]);
        done += __popcll(m);
      }
    }
    const int32_t count = done < target ? done : target;
    zero_rows(out, count, levels, lane);
    if (counts && lane == 0) counts[(size_t)env * 2 + side] = count;
  }
}
#endif  // __HIPCC__

#endif
