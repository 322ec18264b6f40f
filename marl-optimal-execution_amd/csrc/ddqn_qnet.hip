// ddqn_qnet.hip — the DDQN learner's Q-network inference and epsilon-greedy action in one launch
// (libmxa_ddqn.so, include/mxa_ddqn.h, with ddqn_period.hip; mxabides/ddqn.py DDQNLearner(fused_act=True)).
//
// The networks are NNModel_1 / NNModel_2 (util/model/QNets.py:7-51): up to eight Dense layers
// of at most 256 units, ReLU on all but the last, no dropout (Keras predict).  The work per
// period is a few hundred MFLOP on a [n_envs][2] input, so what it costs in PyTorch is its ~25
// launches, not its arithmetic.  The tile forward itself (16 envs per workgroup of 256 lanes, the
// weights staged per pass of 64 neurons in LDS, one fmaf chain per output in index order) is
// ddqn_qnet_device.h's, shared with the training kernels of ddqn_train.hip.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ddqn_device.h"
#include "ddqn_qnet_device.h"

namespace {

using namespace qnet;

struct QnetArgs {
  Net net;
  int n;
  const float* x;        // [n][dims[0]]
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

__global__ __launch_bounds__(kThreads) void qnet_kernel(QnetArgs p) {
  __shared__ __attribute__((aligned(16))) float acts[2][kTile][kActStride];
  __shared__ __attribute__((aligned(16))) float wbuf[kWbufFloats];
  const int t = threadIdx.x;
  const int row0 = blockIdx.x * kTile;  // < n: the grid is ceil(n / kTile)
  const int rows = min(kTile, p.n - row0);

  load_tile(p.x, p.net.dims[0], row0, rows, acts[0]);
  const int cur = forward_tile(p.net, acts, wbuf, 0, Identity());
  __syncthreads();

  const int n_out = p.net.dims[p.net.n_layers];
  if (p.q != nullptr) {
    for (int e = 0; e < rows; e++)
      for (int j = t; j < n_out; j += kThreads) p.q[(size_t)(row0 + e) * n_out + j] = acts[cur][e][j];
  }
  if (p.a == nullptr || t >= rows) return;

  // one lane per env: torch.argmax (the lowest index of the maximum; a NaN counts as the maximum)
  const int greedy = argmax_row(&acts[cur][t][0], n_out);
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
  if (n < 0 || !qnet::layout(p.net, n_layers, dims, params)) return false;
  p.n = n;
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
