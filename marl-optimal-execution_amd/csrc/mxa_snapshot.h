// mxa_snapshot.h — env-state snapshots (include/mxa_snap.h): the slot arithmetic and the
// map checks in plain C++ (no HIP types: a CPU program can call them), and the one copy kernel that
// serves save and restore.
//
// Between launches an env's whole state is its env block (mxa_layout.h holds offsets only), its
// d_built seed word and its rows of the book-update log.  A slot holds the three back to back:
//   [0, env_stride)              the env block, trace ring included
//   [env_stride, +256)           the trailer: word 0 is the d_built seed word
//   [env_stride + 256, ...)      log_cap 16-byte book-update records (handles with a log only)
// every piece a multiple of 256 bytes, so every 16-byte lane access is aligned.
#ifndef MXA_SNAPSHOT_H
#define MXA_SNAPSHOT_H
#include <cstdint>
#include <vector>

namespace mxa_snap {

constexpr int64_t TRAILER_BYTES = 256;
constexpr int64_t LOG_REC_BYTES = 16;  // sizeof(BlRec)

constexpr int64_t align256(int64_t x) { return (x + 255) / 256 * 256; }
// where a slot's log rows start / what one slot takes (log_cap 0: a handle without a book-update log)
constexpr int64_t log_offset(int64_t env_stride) { return env_stride + TRAILER_BYTES; }
constexpr int64_t slot_bytes(int64_t env_stride, int32_t log_cap) {
  return log_offset(env_stride) + align256((int64_t)log_cap * LOG_REC_BYTES);
}
// 0 for a stride the copy cannot take: the kernel has no tail path below 256 bytes
constexpr bool stride_ok(int64_t env_stride) { return env_stride > 0 && env_stride % 256 == 0; }

// slot_of_env [n_envs] (-1: the env takes no part; NULL: the identity map) against a snapshot of
// n_slots slots of which filled[s] != 0 have been saved.  save: two envs naming one slot is refused;
// restore: many envs may name one slot (a fork), each named slot must have been saved.
// Returns NULL when the map is good, else what is wrong with it.
inline const char* check_map(const int32_t* slot_of_env, int32_t n_envs, int32_t n_slots, bool save,
                             const uint8_t* filled) {
  if (n_envs <= 0 || n_slots <= 0 || !filled) return "bad arguments";
  if (!slot_of_env) {
    if (n_slots < n_envs) return "the identity map (NULL) needs n_slots >= n_envs";
    if (!save)
      for (int32_t e = 0; e < n_envs; e++)
        if (!filled[e]) return "restoring a slot that was never saved";
    return nullptr;
  }
  for (int32_t e = 0; e < n_envs; e++)
    if (slot_of_env[e] < -1 || slot_of_env[e] >= n_slots) return "a map entry outside -1 .. n_slots - 1";
  if (save) {
    std::vector<uint8_t> taken((size_t)n_slots, 0);
    for (int32_t e = 0; e < n_envs; e++) {
      const int32_t s = slot_of_env[e];
      if (s < 0) continue;
      if (taken[s]) return "two envs saving to one slot";
      taken[s] = 1;
    }
  } else {
    for (int32_t e = 0; e < n_envs; e++)
      if (slot_of_env[e] >= 0 && !filled[slot_of_env[e]]) return "restoring a slot that was never saved";
  }
  return nullptr;
}

// the log records a slot or an env carries: max(blog_n, blog_fin) capped at the log capacity, as
// mxa_read_book_log counts them
constexpr int32_t log_count(int32_t blog_n, int32_t blog_fin, int32_t log_cap) {
  const int32_t c = blog_fin > blog_n ? blog_fin : blog_n;
  return c < 0 ? 0 : c > log_cap ? log_cap : c;
}

// the copy kernel's shape: workgroups of 256 lanes, each lane `loads` 16-byte loads in flight
constexpr int WG_LANES = 256;
constexpr int64_t wg_bytes(int loads) { return (int64_t)WG_LANES * 16 * loads; }
constexpr int64_t wg_count(int64_t bytes, int loads) { return (bytes + wg_bytes(loads) - 1) / wg_bytes(loads); }

}  // namespace mxa_snap

#ifdef __HIPCC__
// One launch copies envs <-> slots as map[env] says (-1: the workgroup leaves).  blockIdx.y walks the
// envs; blockIdx.x < nb_block are the pieces of the env block, the others the pieces of the log rows,
// of which a workgroup copies only the records the SOURCE header counts.  Piece 0 also moves the seed
// word between d_built and the slot's trailer.  restore != 0: slot -> env.  Each lane issues LOADS
// 16-byte loads before its first store, lanes side by side (one wave-instruction: 1 KiB; a 256-byte
// run is 16 lanes, so a stride that is a multiple of 256 needs no tail path, only the lane's bound).
// map[env] is read once per env and is workgroup-uniform.  No atomics, no LDS: a save's slots are
// distinct (mxa_snap::check_map), a restore only reads its slots.
template <int LOADS>
__global__ __launch_bounds__(mxa_snap::WG_LANES) void mxa_snapshot_kernel(
    char* env_base, uint64_t env_stride, char* slot_base, uint64_t slot_bytes, const int32_t* map, int n_envs,
    uint32_t* built, char* blog, int32_t log_cap, uint32_t nb_block, int restore) {
  constexpr uint32_t PIECE = mxa_snap::WG_LANES * 16;  // one load of every lane
  for (int env = blockIdx.y; env < n_envs; env += gridDim.y) {
    const int32_t s = map[env];
    if (s < 0) continue;
    char* e = env_base + (size_t)env * env_stride;
    char* sl = slot_base + (size_t)s * slot_bytes;
    char *src, *dst;
    uint64_t len;
    uint32_t piece = blockIdx.x;
    if (piece < nb_block) {
      src = restore ? sl : e;
      dst = restore ? e : sl;
      len = env_stride;
      if (piece == 0 && threadIdx.x == 0) {
        uint32_t* tr = (uint32_t*)(sl + env_stride);
        if (restore) built[env] = tr[0];
        else tr[0] = built[env];
      }
    } else {
      piece -= nb_block;
      char* el = blog + (size_t)env * (size_t)log_cap * mxa_snap::LOG_REC_BYTES;
      char* ll = sl + mxa_snap::log_offset((int64_t)env_stride);
      const EnvHdr* sh = (const EnvHdr*)(restore ? sl : e);  // the source's counts
      src = restore ? ll : el;
      dst = restore ? el : ll;
      len = (uint64_t)mxa_snap::log_count(sh->blog_n, sh->blog_fin, log_cap) * mxa_snap::LOG_REC_BYTES;
    }
    const uint64_t p0 = (uint64_t)piece * (PIECE * LOADS), o0 = p0 + threadIdx.x * 16u;
    if (p0 >= len) continue;
    uint4 v[LOADS];
    if (p0 + PIECE * LOADS <= len) {  // a whole piece (workgroup-uniform): LOADS loads, then LOADS stores
#pragma unroll
      for (int u = 0; u < LOADS; u++) v[u] = *(const uint4*)(src + o0 + (uint64_t)u * PIECE);
#pragma unroll
      for (int u = 0; u < LOADS; u++) *(uint4*)(dst + o0 + (uint64_t)u * PIECE) = v[u];
      continue;
    }
    // the last piece: a lane past the end loads the last 16 bytes again (len >= 16 here) and stores
    // nothing, so no load sits under a branch here either
#pragma unroll
    for (int u = 0; u < LOADS; u++) {
      const uint64_t o = o0 + (uint64_t)u * PIECE;
      v[u] = *(const uint4*)(src + (o < len ? o : len - 16));
    }
#pragma unroll
    for (int u = 0; u < LOADS; u++)
      if (o0 + (uint64_t)u * PIECE < len) *(uint4*)(dst + o0 + (uint64_t)u * PIECE) = v[u];
  }
}
#endif  // __HIPCC__

#endif
