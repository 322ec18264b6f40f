// ddqn_train.hip — one train_neural_nets update of the DDQN learner in two launches
// (libmxa_ddqn.so, include/mxa_ddqn_train.h; mxabides/ddqn.py DDQNLearner(fused_learn=True)).
//
// The update is about 38 k parameters at batch 32: what it costs on autograd is its ~100 small
// launches, not its arithmetic.  Here it is
//
//   fwd_bwd_kernel   one workgroup per tile of 16 batch rows, ddqn_qnet_device.h's tile forward
//                    three times (target(s2) and eval(s) in predict mode for the Q-target, then
//                    eval(s) in training mode with the dropout keep masks, every layer's
//                    activation kept in the workspace), then the backward deltas per row, layer
//                    by layer with the same weight staging: delta_prev = (delta . W) * pass * scale,
//                    written to the workspace; one lane per row sums the row's squared error.
//                    Block 0 takes the snapshot of the target-copy decision and steps the counter
//                    and epsilon (nothing else in the launch reads them).
//   grad_update_kernel  one lane per parameter element: the gradient as ONE sum over the batch in
//                    index order (delta[b][j] * act[b][k] by fmaf; the bias plain adds), then that
//                    element's target copy, RMSprop step and write-back.  Block 0 sums the rows'
//                    squared errors in index order into the loss.
//   scalars_kernel   mxa_qnet_update alone has no first launch to step the counter and epsilon
//                    in: one lane does it after the elementwise pass has read them.
//
// No floating-point atomics, no reduction across lanes: the same inputs give the same bits.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ddqn_qnet_device.h"

namespace {

using namespace qnet;

// where the workspace keeps what the two launches share, in floats from its start
struct Workspace {
  int aoff[kMaxLayers];  // the training forward's input of layer l >= 1 (hidden layer l-1's output), [B][dims[l]]
  int doff[kMaxLayers];  // d loss / d (layer l's pre-activation), [B][dims[l+1]]
  int rowloss;           // [B]: sum_j (out - tgt)^2 of the row
  int snap;              // one int: the target copy's decision, taken before the counter steps
  int floats;
};

Workspace workspace(int batch, int n_layers, const int* dims) {
  Workspace w{};
  int off = 0;
  for (int l = 1; l < n_layers; l++) {
    w.aoff[l] = off;
    off += batch * dims[l];
  }
  for (int l = 0; l < n_layers; l++) {
    w.doff[l] = off;
    off += batch * dims[l + 1];
  }
  w.rowloss = off;
  off += batch;
  w.snap = off;
  off += 1;
  w.floats = off;
  return w;
}

// the masked update's scalars (learn_on's, in its order)
struct UpdateArgs {
  int on;               // 0: the gradient only
  const uint8_t* live;  // device bool or null (true)
  int64_t* counter;
  int iter;
  double* eps;
  int has_inc;
  double inc, eps_max;
  float lr, rho, one_minus_rho, rms_eps;
  float* rms;
  float* target;  // written where the copy is due
  float* eval;    // stepped
};

struct FwdBwdArgs {
  Net ev, tg;
  int B;
  const float *s, *s2, *r;
  const int64_t* a;
  const uint8_t* masks[kMaxLayers];  // per hidden layer h: keep mask [B][dims[h+1]] or null
  float keep_scale, gamma;
  float* ws;
  Workspace w;
  float* tgt_out;  // [B][n_out] or null
  UpdateArgs u;
};

struct GradArgs {
  int P, B, n_layers;
  int dims[kMaxLayers + 1];
  int woff[kMaxLayers + 1];  // woff[n_layers] = P
  const float* s;
  const float* ws;  // null: the gradient is read from grad (mxa_qnet_update)
  Workspace w;
  float* grad;  // [P], or null
  float* loss;  // or null
  UpdateArgs u;
};

__device__ inline bool is_live(const UpdateArgs& u) { return u.live == nullptr || *u.live != 0; }

// epsilon (:515, may overshoot eps_max by one step), then learn_step_counter += 1
__device__ inline void step_scalars(const UpdateArgs& u) {
  if (u.has_inc) {
    const double e = *u.eps;
    *u.eps = e < u.eps_max ? e + u.inc : u.eps_max;
  }
  *u.counter += 1;
}

// the training forward's epilogue: Dropout after hidden layers 2..n (kept units scaled), and
// every hidden layer's output kept for the backward pass
struct TrainEpi {
  const FwdBwdArgs& p;
  int row0, rows;
  __device__ float operator()(int layer, int e, int j, float v) const {
    if (layer + 1 == p.ev.n_layers) return v;
    const int width = p.ev.dims[layer + 1];
    const bool valid = e < rows;
    const uint8_t* m = p.masks[layer];
    if (m != nullptr && valid) v = (v * (m[(size_t)(row0 + e) * width + j] ? 1.f : 0.f)) * p.keep_scale;
    if (valid) p.ws[p.w.aoff[layer + 1] + (row0 + e) * width + j] = v;
    return v;
  }
};

__global__ __launch_bounds__(kThreads) void fwd_bwd_kernel(FwdBwdArgs p) {
  __shared__ __attribute__((aligned(16))) float acts[2][kTile][kActStride];
  __shared__ __attribute__((aligned(16))) float wbuf[kWbufFloats];
  __shared__ float tgt[kTile][kMaxDim];  // the Q-target, then the squared errors
  __shared__ float qsel[kTile];
  const int t = threadIdx.x, w = t >> 6, l = t & 63;
  const int row0 = blockIdx.x * kTile;  // < B: the grid is ceil(B / kTile)
  const int rows = min(kTile, p.B - row0);
  const int L = p.ev.n_layers, n_in = p.ev.dims[0], n_out = p.ev.dims[L];

  if (p.u.on && blockIdx.x == 0 && t == 0) {
    const bool live = is_live(p.u);
    reinterpret_cast<int*>(p.ws)[p.w.snap] = live && *p.u.counter % p.u.iter == 0;
    if (live) step_scalars(p.u);
  }

  // q_next = target(s2); per row its maximum (the "double" argmax is the target net's own)
  load_tile(p.s2, n_in, row0, rows, acts[0]);
  int cur = forward_tile(p.tg, acts, wbuf, 0, Identity());
  __syncthreads();
  if (t < kTile) qsel[t] = acts[cur][t][argmax_row(&acts[cur][t][0], n_out)];
  __syncthreads();

  // tgt = eval(s) in predict mode, with tgt[b][a[b]] = r[b] + gamma * q_next[b][best]
  load_tile(p.s, n_in, row0, rows, acts[0]);
  cur = forward_tile(p.ev, acts, wbuf, 0, Identity());
  __syncthreads();
  for (int i = t; i < kTile * n_out; i += kThreads) {
    const int e = i / n_out, j = i - e * n_out;
    float v = acts[cur][e][j];
    if (e < rows) {
      if (p.a[row0 + e] == j) v = p.r[row0 + e] + p.gamma * qsel[e];
      if (p.tgt_out != nullptr) p.tgt_out[(size_t)(row0 + e) * n_out + j] = v;
    }
    tgt[e][j] = v;
  }
  __syncthreads();

  // out = eval(s) in training mode; d = 2 (out - tgt) / (B * n_out)
  load_tile(p.s, n_in, row0, rows, acts[0]);
  cur = forward_tile(p.ev, acts, wbuf, 0, TrainEpi{p, row0, rows});
  __syncthreads();
  int dcur = cur ^ 1;
  const float count = (float)(p.B * n_out);
  for (int i = t; i < kTile * n_out; i += kThreads) {
    const int e = i / n_out, j = i - e * n_out;
    const float diff = acts[cur][e][j] - tgt[e][j];
    const float d = e < rows ? (2.f * diff) / count : 0.f;
    acts[dcur][e][j] = d;
    tgt[e][j] = diff * diff;
    if (e < rows) p.ws[p.w.doff[L - 1] + (row0 + e) * n_out + j] = d;
  }
  __syncthreads();
  if (t < rows) {
    float sum = 0.f;
    for (int j = 0; j < n_out; j++) sum += tgt[t][j];
    p.ws[p.w.rowloss + row0 + t] = sum;
  }

  // backward: the deltas of layer-1 from those of layer, for the wave's four rows.  Lane l owns
  // the inputs k = l, l + 64, l + 128, l + 192; W's rows j are staged as in the forward, so a
  // wave reads 64 consecutive floats of a row (no bank conflict) and the rows' deltas by
  // broadcast.  Each delta is one fmaf chain over j in index order.
  constexpr int kCols = kMaxDim / 64;
  for (int layer = L - 1; layer >= 1; layer--) {
    const int in = p.ev.dims[layer], out = p.ev.dims[layer + 1];
    const int ws = w_stride(in);
    const float* W = p.ev.params + p.ev.woff[layer];
    const bool vec = p.ev.vec && (in & 3) == 0 && (p.ev.woff[layer] & 3) == 0;
    float acc[kCols][kEnvsPerLane];
#pragma unroll
    for (int c = 0; c < kCols; c++)
#pragma unroll
      for (int e = 0; e < kEnvsPerLane; e++) acc[c][e] = 0.f;
    for (int j0 = 0; j0 < out; j0 += kPass) {
      const int nj = min(kPass, out - j0);
      __syncthreads();  // the previous pass has read wbuf; the previous layer has written its deltas
      stage_rows(W, j0, nj, in, ws, vec, wbuf);
      __syncthreads();
      const float* dr = &acts[dcur][w * kEnvsPerLane][j0];
      for (int jj = 0; jj < nj; jj++) {
        float dv[kEnvsPerLane];
#pragma unroll
        for (int e = 0; e < kEnvsPerLane; e++) dv[e] = dr[e * kActStride + jj];
#pragma unroll
        for (int c = 0; c < kCols; c++) {
          if (c * 64 < in) {  // wave-uniform
            const int k = l + 64 * c;
            const float wv = k < in ? wbuf[jj * ws + k] : 0.f;
#pragma unroll
            for (int e = 0; e < kEnvsPerLane; e++) acc[c][e] = __builtin_fmaf(dv[e], wv, acc[c][e]);
          }
        }
      }
    }
    // a unit passes gradient exactly where its stored activation is > 0 (torch's ReLU backward,
    // and the keep mask: a dropped unit's activation is 0); kept units' scale multiplies it too
    const float scale = p.masks[layer - 1] != nullptr ? p.keep_scale : 1.f;
#pragma unroll
    for (int c = 0; c < kCols; c++) {
      const int k = l + 64 * c;
      if (k < in) {
#pragma unroll
        for (int e = 0; e < kEnvsPerLane; e++) {
          const int row = w * kEnvsPerLane + e;
          float v = 0.f;
          if (row < rows) {
            const int at = (row0 + row) * in + k;
            v = p.ws[p.w.aoff[layer] + at] > 0.f ? acc[c][e] * scale : 0.f;
            p.ws[p.w.doff[layer - 1] + at] = v;
          }
          acts[dcur ^ 1][row][k] = v;
        }
      }
    }
    dcur ^= 1;
  }
}

__global__ __launch_bounds__(256) void grad_update_kernel(GradArgs p) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (p.loss != nullptr && i == 0) {  // the rows' squared errors in index order
    float sum = 0.f;
    for (int b = 0; b < p.B; b++) sum += p.ws[p.w.rowloss + b];
    *p.loss = sum / (float)(p.B * p.dims[p.n_layers]);
  }
  if (i >= p.P) return;
  float g;
  if (p.ws != nullptr) {
    int layer = 0;
    while (i >= p.woff[layer + 1]) layer++;  // woff[n_layers] = P > i
    const int in = p.dims[layer], out = p.dims[layer + 1];
    const int idx = i - p.woff[layer];
    const float* D = p.ws + p.w.doff[layer];
    g = 0.f;
    if (idx < out * in) {
      const int j = idx / in, k = idx - j * in;
      const float* A = layer == 0 ? p.s : p.ws + p.w.aoff[layer];
      for (int b = 0; b < p.B; b++) g = __builtin_fmaf(D[b * out + j], A[b * in + k], g);
    } else {
      const int j = idx - out * in;
      for (int b = 0; b < p.B; b++) g += D[b * out + j];
    }
    if (p.grad != nullptr) p.grad[i] = g;
  } else {
    g = p.grad[i];
  }
  const UpdateArgs& u = p.u;
  if (!u.on || !is_live(u)) return;
  // with the first launch its snapshot (the counter has stepped since); alone, the counter itself,
  // which scalars_kernel steps afterwards
  const bool do_copy = p.ws != nullptr ? reinterpret_cast<const int*>(p.ws)[p.w.snap] != 0 : *u.counter % u.iter == 0;
  const float e = u.eval[i];
  if (do_copy) u.target[i] = e;  // the eval parameters from before the step
  // learn_on's torch expressions, one rounding each (no contraction: -ffp-contract=off)
  const float rms = u.rho * u.rms[i] + (u.one_minus_rho * g) * g;
  u.rms[i] = rms;
  const float step = (u.lr * g) / (__builtin_sqrtf(rms) + u.rms_eps);
  u.eval[i] = e - step;
}

__global__ void scalars_kernel(UpdateArgs u) {
  if (is_live(u)) step_scalars(u);
}

bool fill_update(UpdateArgs& u, float* eval, float* target, float* rms, const uint8_t* live, int64_t* counter,
                 int replace_target_iter, double* eps, int has_inc, double inc, double eps_max, double lr, double rho,
                 double rms_eps) {
  if (eval == nullptr || target == nullptr || rms == nullptr || counter == nullptr || eps == nullptr ||
      replace_target_iter < 1)
    return false;
  u.on = 1;
  u.live = live;
  u.counter = counter;
  u.iter = replace_target_iter;
  u.eps = eps;
  u.has_inc = has_inc != 0;
  u.inc = inc;
  u.eps_max = eps_max;
  // the Python scalars of learn_on's expressions, rounded to fp32 as torch rounds them
  u.lr = (float)lr;
  u.rho = (float)rho;
  u.one_minus_rho = (float)(1.0 - rho);
  u.rms_eps = (float)rms_eps;
  u.rms = rms;
  u.target = target;
  u.eval = eval;
  return true;
}

// the two launches of mxa_qnet_grad (u.on == 0) and mxa_qnet_train
int run(hipStream_t stream, int batch, const float* s, const int64_t* a, const float* s2, const float* r,
        const float* eval, const float* target, int n_layers, const int* dims, const void* const* masks, double rate,
        double gamma, void* ws, float* grad, float* loss, float* tgt_out, const UpdateArgs& u) {
  FwdBwdArgs f{};
  GradArgs g{};
  if (!layout(f.ev, n_layers, dims, eval, &g.P) || !layout(f.tg, n_layers, dims, target)) return (int)hipErrorInvalidValue;
  if (batch < 0 || batch > kMaxDim || !(rate >= 0.0 && rate < 1.0)) return (int)hipErrorInvalidValue;
  if (batch == 0) return 0;
  if (s == nullptr || a == nullptr || s2 == nullptr || r == nullptr || eval == nullptr || target == nullptr ||
      ws == nullptr || (reinterpret_cast<uintptr_t>(ws) & 3) != 0)
    return (int)hipErrorInvalidValue;
  if (!u.on && (grad == nullptr || loss == nullptr)) return (int)hipErrorInvalidValue;  // nothing would be returned
  f.B = g.B = batch;
  f.s = g.s = s;
  f.s2 = s2;
  f.r = r;
  f.a = a;
  for (int h = 0; h + 1 < n_layers; h++)  // hidden layer h; the first one has no Dropout
    f.masks[h] = (masks != nullptr && h >= 1 && rate > 0.0) ? static_cast<const uint8_t*>(masks[h]) : nullptr;
  f.keep_scale = 1.0f / (float)(1.0 - rate);
  f.gamma = (float)gamma;
  f.ws = static_cast<float*>(ws);
  g.ws = f.ws;
  f.w = g.w = workspace(batch, n_layers, dims);
  f.tgt_out = tgt_out;
  f.u = g.u = u;
  g.n_layers = n_layers;
  for (int i = 0; i <= kMaxLayers; i++) g.dims[i] = f.ev.dims[i];
  for (int i = 0; i <= kMaxLayers; i++) g.woff[i] = i < n_layers ? f.ev.woff[i] : g.P;
  g.grad = grad;
  g.loss = loss;
  hipLaunchKernelGGL(fwd_bwd_kernel, dim3((batch + kTile - 1) / kTile), dim3(kThreads), 0, stream, f);
  int rc = (int)hipGetLastError();
  if (rc) return rc;
  hipLaunchKernelGGL(grad_update_kernel, dim3((g.P + 255) / 256), dim3(256), 0, stream, g);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int64_t mxa_qnet_train_workspace(int batch, int n_layers, const int* dims) {
  Net net{};
  if (!layout(net, n_layers, dims, nullptr) || batch < 0 || batch > kMaxDim) return -1;
  return (int64_t)workspace(batch, n_layers, dims).floats * (int64_t)sizeof(float);
}

int mxa_qnet_grad(hipStream_t stream, int batch, const float* s, const int64_t* a, const float* s2, const float* r,
                  const float* eval, const float* target, int n_layers, const int* dims, const void* const* masks,
                  double rate, double gamma, void* workspace, float* grad, float* loss, float* tgt_out) {
  UpdateArgs u{};
  return run(stream, batch, s, a, s2, r, eval, target, n_layers, dims, masks, rate, gamma, workspace, grad, loss,
             tgt_out, u);
}

int mxa_qnet_update(hipStream_t stream, int64_t n_params, const float* grad, float* eval, float* target, float* rms,
                    const uint8_t* live, int64_t* counter, int replace_target_iter, double* eps, int has_inc,
                    double inc, double eps_max, double lr, double rho, double rms_eps) {
  GradArgs g{};
  if (n_params < 1 || n_params > (int64_t)kMaxLayers * (kMaxDim * kMaxDim + kMaxDim) || grad == nullptr ||
      !fill_update(g.u, eval, target, rms, live, counter, replace_target_iter, eps, has_inc, inc, eps_max, lr, rho,
                   rms_eps))
    return (int)hipErrorInvalidValue;
  g.P = (int)n_params;
  g.grad = const_cast<float*>(grad);  // read only: ws is null
  hipLaunchKernelGGL(grad_update_kernel, dim3((g.P + 255) / 256), dim3(256), 0, stream, g);
  int rc = (int)hipGetLastError();
  if (rc) return rc;
  hipLaunchKernelGGL(scalars_kernel, dim3(1), dim3(1), 0, stream, g.u);
  return (int)hipGetLastError();
}

int mxa_qnet_train(hipStream_t stream, int batch, const float* s, const int64_t* a, const float* s2, const float* r,
                   float* eval, float* target, int n_layers, const int* dims, const void* const* masks, double rate,
                   double gamma, void* workspace, float* grad, float* loss, float* tgt_out, float* rms,
                   const uint8_t* live, int64_t* counter, int replace_target_iter, double* eps, int has_inc, double inc,
                   double eps_max, double lr, double rho, double rms_eps) {
  UpdateArgs u{};
  // the net's dimensions first, as every mxa_qnet_* export: run() refuses them before it reads u
  Net net{};
  if (!layout(net, n_layers, dims, eval) || batch < 0 || batch > kMaxDim) return (int)hipErrorInvalidValue;
  if (batch == 0) return 0;
  if (!fill_update(u, eval, target, rms, live, counter, replace_target_iter, eps, has_inc, inc, eps_max, lr, rho,
                   rms_eps))
    return (int)hipErrorInvalidValue;
  return run(stream, batch, s, a, s2, r, eval, target, n_layers, dims, masks, rate, gamma, workspace, grad, loss,
             tgt_out, u);
}

}  // extern "C"
