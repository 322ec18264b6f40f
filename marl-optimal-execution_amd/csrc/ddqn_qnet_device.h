// ddqn_qnet_device.h — the Q-network's forward of one 16-row tile on the device, ONE statement of it
// shared by the inference kernel (ddqn_qnet.hip) and the training kernels (ddqn_train.hip): the
// layer table, the staging of a pass's weight rows in LDS and the fmaf chain.
//
// A workgroup of 256 lanes owns a tile of 16 rows and walks the layers with the tile's activations
// ping-ponged in LDS.  A layer runs in passes of 64 output neurons: the pass's weight rows are
// staged in LDS (row-major as the flat parameter buffer has them, the row stride padded so that the
// lanes' 16-byte reads fall on distinct banks), then lane l of wave w computes neuron 64 * pass + l
// for the four rows 4w .. 4w+3: one 16-byte read of its own weight row and four wave-uniform
// (broadcast) reads of the rows' activations per 16 FMAs.
//
// Every output element is ONE fp32 fmaf chain over k = 0 .. in-1 in index order, started from 0,
// with the bias added last.  Which lane computes it depends only on the row's slot in its tile,
// never on the operands, so a row's result is bitwise the same in any batch, at any n.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace qnet {

constexpr int kMaxLayers = 8;
constexpr int kMaxDim = 256;
constexpr int kTile = 16;       // rows per workgroup
constexpr int kThreads = 256;   // 4 waves; wave w owns rows 4w .. 4w+3 of the tile
constexpr int kEnvsPerLane = 4;
constexpr int kPass = 64;       // output neurons per pass: one per lane
// row strides in floats: multiples of 4 (16-byte reads), and an odd number of 16-byte slots so
// that 16 consecutive rows fall on 16 distinct slots of the 256-byte bank row
constexpr int kActStride = kMaxDim + 4;
constexpr int kWStrideMax = kMaxDim + 4;
// + a 16-byte slot per lane past the rows: where a lane without a row element stores instead
constexpr int kWbufFloats = kPass * kWStrideMax + 4 * 64;

typedef float ActTile[kTile][kActStride];

// one net's layer table: the flat fp32 buffer holds per layer weight[out][in], then bias[out]
struct Net {
  int n_layers;
  int dims[kMaxLayers + 1];
  int woff[kMaxLayers];  // offset of weight[out][in] in the flat buffer; bias[out] follows it
  int vec;               // the parameter buffer is 16-byte aligned: rows with in % 4 == 0 and
                         // woff % 4 == 0 are staged with 16-byte loads
  const float* params;
};

// the weight rows' LDS stride for a layer of `in` inputs
__host__ __device__ constexpr int w_stride(int in) { return ((in + 3) & ~3) | 4; }

// fills the layer table; false when the dimensions are outside what the kernels support.  Returns
// the parameter count through n_params when it is given
inline bool layout(Net& p, int n_layers, const int* dims, const float* params, int* n_params = nullptr) {
  if (n_layers < 1 || n_layers > kMaxLayers || dims == nullptr) return false;
  for (int i = 0; i <= n_layers; i++)
    if (dims[i] < 1 || dims[i] > kMaxDim) return false;
  p.n_layers = n_layers;
  int off = 0;
  for (int i = 0; i <= kMaxLayers; i++) p.dims[i] = i <= n_layers ? dims[i] : 0;
  for (int i = 0; i < kMaxLayers; i++) {
    p.woff[i] = off;
    if (i < n_layers) off += dims[i] * dims[i + 1] + dims[i + 1];
  }
  p.vec = (reinterpret_cast<uintptr_t>(params) & 15) == 0;
  p.params = params;
  if (n_params != nullptr) *n_params = off;
  return true;
}

// the tile's inputs; the slots past n hold zeros (computed like any row, never written out)
__device__ inline void load_tile(const float* x, int n_in, int row0, int rows, ActTile& dst) {
  for (int i = threadIdx.x; i < kTile * n_in; i += kThreads) {
    const int e = i / n_in, k = i - e * n_in;
    dst[e][k] = e < rows ? x[(size_t)(row0 + e) * n_in + k] : 0.f;
  }
}

// stage rows j0 .. j0+nj-1 of W [out][in] into wbuf at stride ws: wave w takes rows w, w+4, ...,
// the lanes walk a row; the loads of a wave's 16 rows are all issued before the first LDS store
// waits for one (they are unconditional, from clamped and so valid addresses: a branch around
// each load would make each wait for the one before, and so would a branch around each store,
// into which the compiler sinks the load: a lane with nothing to stage stores to its spare slot)
__device__ inline void stage_rows(const float* W, int j0, int nj, int in, int ws, bool vec, float* wbuf) {
  const int t = threadIdx.x, w = t >> 6, l = t & 63;
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
}

// the forward of the tile in acts[cur] through every layer of `net`; returns the buffer index that
// holds the last layer's outputs (all lanes must pass a __syncthreads before reading them).
// epi(layer, e, j, v) is called once per output element, v after the bias and the ReLU (all but
// the last layer), e the row's slot in the tile, j the neuron; what it returns is the activation.
template <class Epi>
__device__ inline int forward_tile(const Net& p, ActTile* acts, float* wbuf, int cur, Epi epi) {
  const int t = threadIdx.x, w = t >> 6, l = t & 63;
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
      stage_rows(W, j0, nj, in, ws, vec, wbuf);
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
          acts[cur ^ 1][w * kEnvsPerLane + e][j0 + l] = epi(layer, w * kEnvsPerLane + e, j0 + l, v);
        }
      }
    }
    cur ^= 1;
  }
  return cur;
}

struct Identity {
  __device__ float operator()(int, int, int, float v) const { return v; }
};

// torch.argmax of one row: the lowest index of the maximum; a NaN counts as the maximum
__device__ inline int argmax_row(const float* qr, int n_out) {
  float best = qr[0];
  int greedy = 0;
  for (int j = 1; j < n_out; j++) {
    const float v = qr[j];
    if (best == best && (v > best || v != v)) {
      best = v;
      greedy = j;
    }
  }
  return greedy;
}

}  // namespace qnet
