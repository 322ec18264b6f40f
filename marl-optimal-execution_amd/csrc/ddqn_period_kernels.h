// ddqn_period_kernels.h — the per-period kernels of the DDQN learner, written once over the state's
// source S and instantiated by ddqn_period.hip (Grid2: ExecutionTask's two grids, include/mxa_ddqn.h,
// libmxa_ddqn.so) and by ddqn_features.hip (Spec: a list of up to 8 features of the observation row,
// include/mxa_ddqn_features.h, libmxa_ddqn_features.so).  S has W, the most elements a state row
// holds (a constant, so a row stays in registers), width(), how many it does, and eval(o, out).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ddqn_device.h"

namespace {

struct PeriodArgs {
  int n, obs_w, st_w, train;
  const double *obs, *st, *prev, *arrival;
  const int32_t* flags;
  const uint8_t* alive;   // before the step
  uint8_t* alive_next;    // ok & not done
  uint8_t* live;          // [1] any(alive): the learner's update mask for this period
  const float* s;         // [n][width] the state the action was chosen on
  const int64_t* a;       // [n]
  float* s2;              // [n][width] the state after the step (the next period's s)
  double* r_row;          // [n] where(ok, r, 0)
  int64_t* env_steps;     // [n] += alive
  double rscale;          // 1e4 / q0, the Python float of task.reward
  float *ring_s, *ring_s2, *ring_r;
  int64_t* ring_a;
  int64_t cap;
  int64_t* n_dev;   // rows written so far (ReplayRing.n_dev)
  int64_t* stored;  // run_episode's stored count
};

template <class S>
__global__ __launch_bounds__(1024) void ddqn_period_kernel(PeriodArgs p, S state) {
  __shared__ int wn[16];
  __shared__ int any_alive;
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  if (threadIdx.x == 0) any_alive = 0;
  __syncthreads();
  const int64_t n_dev0 = *p.n_dev;
  int64_t done = 0;
  const int sw = state.width();
  for (int i0 = 0; i0 < p.n; i0 += 1024) {
    const int i = i0 + (int)threadIdx.x;
    bool ok = false;
    double rr = 0.0;
    float s2v[S::W];
#pragma unroll
    for (int f = 0; f < S::W; f++) s2v[f] = 0.f;
    if (i < p.n) {
      const int32_t f = p.flags[i];
      const bool al = p.alive[i] != 0;
      if (al) any_alive = 1;  // any writer stores the same value
      ok = al && (f & 2) != 0 && (f & 4) == 0;
      const double* cur = p.st + (size_t)i * p.st_w;
      const double* pre = p.prev + (size_t)i * p.st_w;
      const double dq = cur[2] - pre[2];
      const double dcash = cur[0] - pre[0];
      rr = dq > 0 ? p.rscale * (2.0 * dq + dcash / p.arrival[i]) : 0.0;
      state.eval(p.obs + (size_t)i * p.obs_w, s2v);
#pragma unroll
      for (int f = 0; f < S::W; f++)
        if (f < sw) p.s2[(size_t)sw * i + f] = s2v[f];
      p.env_steps[i] += al ? 1 : 0;
      p.r_row[i] = ok ? rr : 0.0;
      p.alive_next[i] = ok && (f & 1) == 0;
    }
    // replay positions in env order: (n_dev + inclusive count - 1) % cap, as ReplayRing.add_device
    const uint64_t m = __ballot(p.train && ok);
    if (l == 0) wn[w] = __popcll(m);
    __syncthreads();
    int off = 0, tot = 0;
    for (int k = 0; k < 16; k++) {
      off += k < w ? wn[k] : 0;
      tot += wn[k];
    }
    if (p.train && ok) {
      const int64_t c = done + off + __popcll(m & ((1ull << l) - 1)) + 1;
      const int64_t pos = (n_dev0 + c - 1) % p.cap;
#pragma unroll
      for (int f = 0; f < S::W; f++)
        if (f < sw) {
          p.ring_s[sw * pos + f] = p.s[(size_t)sw * i + f];
          p.ring_s2[sw * pos + f] = s2v[f];
        }
      p.ring_a[pos] = p.a[i];
      p.ring_r[pos] = (float)rr;
    }
    done += tot;
    __syncthreads();  // wn is rewritten by the next block
  }
  if (threadIdx.x == 0) {
    *p.live = any_alive ? 1 : 0;
    if (p.train) {
      *p.n_dev = n_dev0 + done;
      *p.stored += done;
    }
  }
}

template <class S>
__global__ __launch_bounds__(256) void ddqn_state_kernel(int n, int obs_w, const double* obs, S state, float* s) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float v[S::W];
  state.eval(obs + (size_t)i * obs_w, v);
  const int sw = state.width();
#pragma unroll
  for (int f = 0; f < S::W; f++)
    if (f < sw) s[(size_t)sw * i + f] = v[f];
}

}  // namespace
