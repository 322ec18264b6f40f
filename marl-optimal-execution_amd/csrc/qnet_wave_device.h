// qnet_wave_device.h — the Q-network's forward of ONE input row on ONE 64-lane wave, the argmax
// and the epsilon-greedy select: the policy of the closed-loop step kernel (mxa_kernels.hip
// mxa_step_policy_kernel, include/mxa.h mxa_step_policy) and of its probe (mxa_policy_probe).
//
// The parameters are the flat fp32 buffer of mxa_qnet_* (include/mxa_ddqn.h): per layer
// weight[out][in] row-major, then bias[out].  Lane l owns the neurons l, l + 64, l + 128 and
// l + 192 of every layer; a layer's activations are those four registers per lane, and neuron k's
// reaches every lane by v_readlane (k is wave-uniform), so the forward needs no LDS.  A lane reads
// its own weight rows from L2 (153 KB for NNModel_1), 16 bytes at a time where in % 4 == 0 and
// the row starts on a 16-byte boundary, one float at a time otherwise.
//
// The arithmetic is ddqn_qnet_device.h's, so the bits are mxa_qnet_forward's: every output is ONE
// fp32 fmaf chain over k = 0 .. in-1 in index order started from 0, then acc + bias, then
// v < 0 ? 0 : v on all but the last layer (a NaN stays a NaN).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace qwave {

constexpr int kMaxLayers = 8;
constexpr int kMaxDim = 256;
constexpr int kRegs = kMaxDim / 64;  // activation registers per lane

// host: the dimensions mxa_qnet_* support
inline bool dims_ok(int n_layers, const int32_t* dims) {
  if (n_layers < 1 || n_layers > kMaxLayers || dims == nullptr) return false;
  for (int i = 0; i <= n_layers; i++)
    if (dims[i] < 1 || dims[i] > kMaxDim) return false;
  return true;
}

__device__ __forceinline__ float lane_get(float v, int l) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}

// one neuron's chain over the `in` activations held as act[k >> 6] of lane k & 63; wr: its weight row
template <bool VEC>
__device__ __forceinline__ float chain(const float* wr, const float (&act)[kRegs], int in) {
  float acc = 0.f;
#pragma unroll
  for (int b = 0; b < kRegs; b++) {
    const int nb = min(64, in - 64 * b);  // <= 0: the layer has no such inputs
    if constexpr (VEC) {
      for (int k = 0; k < nb; k += 4) {  // in % 4 == 0: nb is a multiple of 4
        const float4 w = *reinterpret_cast<const float4*>(wr + 64 * b + k);
        acc = __builtin_fmaf(lane_get(act[b], k), w.x, acc);
        acc = __builtin_fmaf(lane_get(act[b], k + 1), w.y, acc);
        acc = __builtin_fmaf(lane_get(act[b], k + 2), w.z, acc);
        acc = __builtin_fmaf(lane_get(act[b], k + 3), w.w, acc);
      }
    } else {
      for (int k = 0; k < nb; k++) acc = __builtin_fmaf(lane_get(act[b], k), wr[64 * b + k], acc);
    }
  }
  return acc;
}

// the forward through every layer.  In: act[r] of lane l is input l + 64 r (what lies past
// dims[0] is not read); out: act[r] of lane l is output l + 64 r for l + 64 r < dims[n_layers]
// (the registers past it hold copies of the last neuron, never read).  n_layers, dims and params
// are wave-uniform; every lane of the wave must call.
__device__ __forceinline__ void forward(const float* params, int n_layers, const int32_t* dims, int lane,
                                        float (&act)[kRegs]) {
  int off = 0;
  for (int layer = 0; layer < n_layers; layer++) {
    const int in = dims[layer], out = dims[layer + 1];
    const float* W = params + off;
    const float* B = W + (size_t)out * in;
    const bool vec = (in & 3) == 0 && (reinterpret_cast<uintptr_t>(W) & 15) == 0;
    const bool relu = layer + 1 < n_layers;
    float nxt[kRegs];
#pragma unroll
    for (int r = 0; r < kRegs; r++) nxt[r] = 0.f;
    for (int r = 0; 64 * r < out; r++) {
      const int j = min(64 * r + lane, out - 1);  // a lane past the layer recomputes its last neuron
      const float* wr = W + (size_t)j * in;
      const float acc = vec ? chain<true>(wr, act, in) : chain<false>(wr, act, in);
      float v = acc + B[j];
      if (relu && v < 0.f) v = 0.f;  // a NaN stays a NaN, as in torch.relu
#pragma unroll
      for (int s = 0; s < kRegs; s++) nxt[s] = s == r ? v : nxt[s];
    }
#pragma unroll
    for (int r = 0; r < kRegs; r++) act[r] = nxt[r];
    off += in * out + out;
  }
}

// qnet::argmax_row's rule over the wave's output registers: the lowest index of the maximum; a NaN
// counts as the maximum.  The result is wave-uniform.
__device__ __forceinline__ int argmax(const float (&q)[kRegs], int n_out) {
  float best = lane_get(q[0], 0);
  int greedy = 0;
#pragma unroll
  for (int b = 0; b < kRegs; b++) {
    const int nb = min(64, n_out - 64 * b);
    for (int k = b == 0 ? 1 : 0; k < nb; k++) {
      const float v = lane_get(q[b], k);
      if (best == best && (v > best || v != v)) {
        best = v;
        greedy = 64 * b + k;
      }
    }
  }
  return greedy;
}

// choose_action's select (ddqlearning_execution_agent.py:333-362), as mxa_qnet_act: exploit when
// U < epsilon with enough experience, else the random action; in test mode u, rnd and eps are not read
__device__ __forceinline__ int64_t select(int greedy, int test, int enough, const double* u, const int64_t* rnd,
                                          const double* eps, size_t i) {
  int64_t a = greedy;
  if (!test && !(u[i] < *eps && enough)) a = rnd[i];
  return a;
}

}  // namespace qwave
