// ddqn_qnet.hip — the DDQN learner's Q-network inference and epsilon-greedy action in one launch
// (libmxa_ddqn.so, include/mxa_ddqn.h, with ddqn_period.hip; mxabides/ddqn.py DDQNLearner(fused_act=True)).
//
// The networks are NNModel_1 / NNModel_2 (util/model/QNets.py:7-51): up to eight Dense layers
// of at most 256 units, ReLU on all but the last, no dropout (Keras predict).  The work per
// period is a few hundred MFLOP on a [n_envs][2] input, so what it costs in PyTorch is its ~25
// launches, not its arithmetic.  Here a workgroup of 256 lanes owns a tile of 16 envs and walks
// the layers with the tile's activations ping-ponged in LDS.  A layer runs in passes of 64 output
// neurons: the pass's weight rows are staged in LDS (row-major as the flat parameter buffer has
// them, the row stride padded so that the lanes' 16-byte reads fall on distinct banks), then lane l
// of wave w computes neuron 64 * pass + l for the four envs 4w .. 4w+3: one 16-byte read of its
// own weight row and four wave-uniform (broadcast) reads of the envs' activations per 16 FMAs.
//
// Every output element is ONE fp32 fmaf chain over k = 0 .. in-1 in index order, started from 0,
// with the bias added last.  Which lane computes it depends only on the env's slot in its tile,
// never on the operands, so a row's result is bitwise the same in any batch, at any n.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ddqn_device.h"

namespace {

constexpr int kMaxLayers = 8;
constexpr int kMaxDim = 256;
constexpr int kTile = 16;       // envs per workgroup
constexpr int kThreads = 256;   // 4 waves; wave w owns envs 4w .. 4w+3 of the tile
constexpr int kEnvsPerLane = 4;
constexpr int kPass = 64;       // output neurons per pass: one per lane
// row strides in floats: multiples of 4 (16-byte reads), and an odd number of 16-byte slots so
// that 16 consecutive rows fall on 16 distinct slots of the 256-byte bank row
constexpr int kActStride = kMaxDim + 4;
constexpr int kWStrideMax = kMaxDim + 4;

struct QnetArgs {
  int n, n_layers;
  int dims[kMaxLayers + 1];
  int woff[kMaxLayers];  // offset of weight[out][in] in the flat buffer; bias[out] follows it
  int vec;               // the parameter buffer is 16-byte aligned: rows with in % 4 == 0 and
                         // woff % 4 == 0 are staged with 16-byte loads
  const float* x;        // [n][dims[0]]
  const float* params;
  float* q;              // [n][n_out] or null
  // epsilon-greedy and the action vector (mxa_qnet_act); a == null: forward only
  int test, enough, obs_w;
  const double* u;       // [n]
  const int64_t* rnd;    // [n]
  const double* eps;     // [1]
  const double* obs;     // [n][obs_w]
  const double* table;   // [n_out][3]
  double q0;
  int64_t* a;            // [n]
  double* act;           // [n][3] or null
};

// the weight rows' LDS stride for a layer of `in` inputs
__host__ __device__ constexpr int w_stride(int in) { return ((in + 3) & ~3) | 4; }

__global__ __launch_bounds__(kThreads) void qnet_kernel(QnetArgs p) {
  __shared__ __attribute__((aligned(16))) float acts[2][kTile][kActStride];
  // + a 16-byte slot per lane past the rows: where a lane without a row element stores instead
  __shared__ __attribute__((aligned(16))) float wbuf[kPass * kWStrideMax + 4 * 64];
  const int t = threadIdx.x, w = t >> 6, l = t & 63;
  const int row0 = blockIdx.x * kTile;  // < n: the grid is ceil(n / kTile)
  const int rows = min(kTile, p.n - row0);

  // the tile's inputs; the slots past n hold zeros (computed like any row, never written out)
  const int n_in = p.dims[0];
  for (int i = t; i < kTile * n_in; i += kThreads) {
    const int e = i / n_in, k = i - e * n_in;
    acts[0][e][k] = e < rows ? p.x[(size_t)(row0 + e) * n_in + k] : 0.f;
  }

  int cur = 0;
  for (int layer = 0; layer < p.n_layers; layer++) {
    const int in = p.dims[layer], out = p.dims[layer + 1];
    const int ws = w_stride(in), in4 = in & ~3;
    const float* W = p.params + p.woff[layer];
    const float* B = W + (size_t)out * in;
    const bool vec = p.vec && (in & 3) == 0 && (p.woff[layer] & 3) == 0;
    const bool relu = layer + 1 < p.n_layers;
    for (int j0 = 0; j0 < out; j0 += kPass) {
      const int nj = min(kPass, out - j0);
      __syncthreads();  // the previous pass has read wbuf; the previous layer has written acts
      // stage rows j0 .. j0+nj-1: wave w takes rows w, w+4, ..., the lanes walk a row; the
      // loads of a wave's 16 rows are all issued before the first LDS store waits for one (they
      // are unconditional, from clamped and so valid addresses: a branch around each load would
      // make each wait for the one before, and so would a branch around each store, into which
      // the compiler sinks the load: a lane with nothing to stage stores to its spare slot)
      constexpr int kRowsPerWave = kPass / (kThreads / 64);
      if (vec) {
        const int q = in >> 2;  // <= 64: one 16-byte load per lane and row
        const float4* src = reinterpret_cast<const float4*>(W + (size_t)j0 * in);
        float4 tmp[kRowsPerWave];
#pragma unroll
        for (int i = 0; i < kRowsPerWave; i++) {
          const int r = w + i * (kThreads / 64);
          tmp[i] = src[min(r, nj - 1) * q + min(l, q - 1)];
        }
#pragma unroll
        for (int i = 0; i < kRowsPerWave; i++) {
          const int r = w + i * (kThreads / 64);
          float* dst = (r < nj && l < q) ? wbuf + r * ws + 4 * l : wbuf + kPass * kWStrideMax + 4 * l;
          *reinterpret_cast<float4*>(dst) = tmp[i];
        }
      } else {
        const float* src = W + (size_t)j0 * in;
        for (int k = l; k < in; k += 64) {
          float tmp[kRowsPerWave];
#pragma unroll
          for (int i = 0; i < kRowsPerWave; i++) {
            const int r = w + i * (kThreads / 64);
            tmp[i] = src[min(r, nj - 1) * in + k];
          }
#pragma unroll
          for (int i = 0; i < kRowsPerWave; i++) {
            const int r = w + i * (kThreads / 64);
            if (r < nj) wbuf[r * ws + k] = tmp[i];
          }
        }
      }
      __syncthreads();
      if (l < nj) {
        const float* wr = wbuf + l * ws;
        const float* ar = &acts[cur][w * kEnvsPerLane][0];
        float acc[kEnvsPerLane] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
        for (int k = 0; k < in4; k += 4) {
          const float4 wv = *reinterpret_cast<const float4*>(wr + k);
#pragma unroll
          for (int e = 0; e < kEnvsPerLane; e++) {
            const float4 av = *reinterpret_cast<const float4*>(ar + e * kActStride + k);
            acc[e] = __builtin_fmaf(av.x, wv.x, acc[e]);
            acc[e] = __builtin_fmaf(av.y, wv.y, acc[e]);
            acc[e] = __builtin_fmaf(av.z, wv.z, acc[e]);
            acc[e] = __builtin_fmaf(av.w, wv.w, acc[e]);
          }
        }
        for (int k = in4; k < in; k++) {
          const float wv = wr[k];
#pragma unroll
          for (int e = 0; e < kEnvsPerLane; e++) acc[e] = __builtin_fmaf(ar[e * kActStride + k], wv, acc[e]);
        }
        const float b = B[j0 + l];
#pragma unroll
        for (int e = 0; e < kEnvsPerLane; e++) {
          float v = acc[e] + b;
          if (relu && v < 0.f) v = 0.f;  // a NaN stays a NaN, as in torch.relu
          acts[cur ^ 1][w * kEnvsPerLane + e][j0 + l] = v;
        }
      }
    }
    cur ^= 1;
  }
  __syncthreads();

  const int n_out = p.dims[p.n_layers];
  if (p.q != nullptr) {
    for (int e = 0; e < rows; e++)
      for (int j = t; j < n_out; j += kThreads) p.q[(size_t)(row0 + e) * n_out + j] = acts[cur][e][j];
  }
  if (p.a == nullptr || t >= rows) return;

  // one lane per env: torch.argmax (the lowest index of the maximum; a NaN counts as the maximum)
  const float* qr = &acts[cur][t][0];
  float best = qr[0];
  int greedy = 0;
  for (int j = 1; j < n_out; j++) {
    const float v = qr[j];
    if (best == best && (v > best || v != v)) {
      best = v;
      greedy = j;
    }
  }
  const int i = row0 + t;
  // choose_action (ddqlearning_execution_agent.py:333-362): exploit when U < epsilon with enough
  // experience, else the random action; in test mode u and rnd are not read
  int64_t a = greedy;
  if (!p.test && !(p.u[i] < *p.eps && p.enough)) a = p.rnd[i];
  p.a[i] = a;
  if (p.act == nullptr) return;
  // ExecutionTask.actions, as mxa_ddqn_actions
  action_of(p.table + 3 * a, p.obs + (size_t)i * p.obs_w, p.q0, p.act + 3 * (size_t)i);
}

// fills the layer table; false when the dimensions are outside what the kernel supports
bool layout(QnetArgs& p, int n, int n_layers, const int* dims, const float* params) {
  if (n < 0 || n_layers < 1 || n_layers > kMaxLayers || dims == nullptr) return false;
  for (int i = 0; i <= n_layers; i++)
    if (dims[i] < 1 || dims[i] > kMaxDim) return false;
  p.n = n;
  p.n_layers = n_layers;
  int off = 0;
  for (int i = 0; i <= kMaxLayers; i++) p.dims[i] = i <= n_layers ? dims[i] : 0;
  for (int i = 0; i < kMaxLayers; i++) {
    p.woff[i] = off;
    if (i < n_layers) off += dims[i] * dims[i + 1] + dims[i + 1];
  }
  p.vec = (reinterpret_cast<uintptr_t>(params) & 15) == 0;
  p.params = params;
  return true;
}

int launch(hipStream_t stream, const QnetArgs& p) {
  hipLaunchKernelGGL(qnet_kernel, dim3((p.n + kTile - 1) / kTile), dim3(kThreads), 0, stream, p);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int mxa_qnet_forward(hipStream_t stream, int n, const float* x, const float* params, int n_layers, const int* dims,
                     float* q) {
  QnetArgs p{};
  if (!layout(p, n, n_layers, dims, params)) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  p.x = x;
  p.q = q;
  return launch(stream, p);
}

int mxa_qnet_act(hipStream_t stream, int n, const float* x, const float* params, int n_layers, const int* dims,
                 int test, int enough, const double* u, const int64_t* rnd, const double* eps, int obs_w,
                 const double* obs, const double* table, double q0, int64_t* a, double* act, float* q) {
  QnetArgs p{};
  if (!layout(p, n, n_layers, dims, params) || obs_w < 2) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  if (a == nullptr) return (int)hipErrorInvalidValue;  // without actions it would be mxa_qnet_forward
  p.x = x;
  p.q = q;
  p.test = test;
  p.enough = enough;
  p.obs_w = obs_w;
  p.u = u;
  p.rnd = rnd;
  p.eps = eps;
  p.obs = obs;
  p.table = table;
  p.q0 = q0;
  p.a = a;
  p.act = act;
  return launch(stream, p);
}

}  // extern "C"
