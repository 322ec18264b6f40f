// mxa_api.hip — host side of libmxa: the C-ABI declared in include/mxa.h.
//
// Builds the per-configuration parameter block (the constants of the reference config
// scripts), lays out one HBM block per env, and launches the kernels of mxa_kernels.hip.
// Each configuration's engine is its own translation unit (mxa_inst.hip, mxa_entry.h); an
// rmsc03-only variant build (-DMXA_ONLY_RMSC03) compiles everything in this one.
#include <hip/hip_runtime.h>

#include <dlfcn.h>
#include <spawn.h>
#include <sys/stat.h>
#include <sys/wait.h>
#include <unistd.h>

#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

extern char** environ;

#include "../../include/mxa.h"
#define MXA_API_TU
#include "mxa_kernels.hip"
#include "mxa_entry.h"
#include "mxa_snapshot.h"
#include "mxa_depth_kernels.h"
#include "mxa_bars_kernels.h"
#ifdef MXA_ONLY_RMSC03
#ifndef MXA_ONLY_CFG  // single-configuration variant builds (profiling): that one configuration
#define MXA_ONLY_CFG 0
#endif
#define MXA_INST_CFG MXA_ONLY_CFG
#include "mxa_inst.hip"
#endif

namespace {

// the envs still running, in env order, and their count: one workgroup of 16 waves walks the env
// headers 1024 at a time (a ballot per wave, the waves' counts through LDS).  The next launch of
// mxa_run is one wave per listed env
__global__ __launch_bounds__(1024) void mxa_compact_kernel(const char* base, uint64_t stride, int n, int32_t* list,
                                                           int* count) {
  __shared__ int wn[16];
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  int done = 0;
  for (int i0 = 0; i0 < n; i0 += 1024) {
    const int i = i0 + (int)threadIdx.x;
    const bool run = i < n && ((const EnvHdr*)(base + (size_t)i * stride))->status == ST_RUNNING;
    const uint64_t m = __ballot(run);
    if (l == 0) wn[w] = __popcll(m);
    __syncthreads();
    int off = done, tot = 0;
    for (int k = 0; k < 16; k++) {
      off += k < w ? wn[k] : 0;
      tot += wn[k];
    }
    if (run) list[off + __popcll(m & ((1ull << l) - 1))] = i;
    done += tot;
    __syncthreads();  // wn is rewritten by the next block of envs
  }
  if (threadIdx.x == 0) *count = done;
}

// the handle's per-env header settings in every env: the exchange-log switch (EnvHdr::exlog) and
// Kernel.runner's stopTime (EnvHdr::t_stop; 0 = the config's own).  No kernel changes either, so
// an env holds the handle's values unless a build has just cleared its header
__global__ void mxa_set_header_kernel(char* base, uint64_t stride, int n, int32_t exlog, int64_t t_stop) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  EnvHdr* h = (EnvHdr*)(base + (size_t)i * stride);
  h->exlog = exlog;
  h->t_stop = t_stop;
}

// the seeds of the episodes in progress (mxa_handle::d_built): a rebuilt env's (mask NULL: every
// env's) becomes the current one of mxa_set_seeds, the others keep the seed they were built from
__global__ void mxa_built_seeds_kernel(uint32_t* built, const uint32_t* seeds, const uint8_t* mask, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && (!mask || mask[i])) built[i] = seeds[i];
}

__global__ void mxa_results_kernel(const char* base, uint64_t stride, int n, int64_t* out) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const EnvHdr* h = (const EnvHdr*)(base + (size_t)i * stride);
  out[4 * i + 0] = h->pops;
  out[4 * i + 1] = (int64_t)h->hash;
  out[4 * i + 2] = h->status;
  out[4 * i + 3] = h->cur;
}

// per-env episode record of the multi-GPU all-gather (events, status, final cash,
// holdings, return; one wave per env): [n][MXA_RECORD_WORDS] int64, see include/mxa.h.  The cash /
// holdings / gain words sum TradingAgent.holdings over agents 1.. (Kernel.runner configs; the gain
// is markToMarket - starting_cash, TradingAgent.py:609-633, summed over the agents whose mean
// Kernel.runner prints, Kernel.py:330-341) or are the execution agent's own (GymKernel handles)
__global__ __launch_bounds__(64) void mxa_records_kernel(const char* base, uint64_t stride, int n, const uint32_t* seeds,
                                                         uint32_t off_ag, int a0, int a1, int64_t* out) {
  const int i = blockIdx.x, lane = threadIdx.x;
  if (i >= n) return;
  const char* e = base + (size_t)i * stride;
  long long cash = 0, shares = 0, gain = 0;
  for (int a = a0 + lane; a < a1; a += 64) {
    const uint32_t* r = (const uint32_t*)(e + off_ag + (size_t)a * MXA_AGENT_BYTES);
    auto g64 = [&](int f) { return (long long)(((uint64_t)r[f + 1] << 32) | r[f]); };
    const long long c = g64(AF_CASH), s = g64(AF_SHARES);
    cash += c;
    shares += s;
    gain += c + (s ? s * g64(AF_LAST_TRADE) : 0) - g64(AF_START_CASH);
  }
  for (int d = 32; d >= 1; d >>= 1) {
    cash += __shfl_xor(cash, d, 64);
    shares += __shfl_xor(shares, d, 64);
    gain += __shfl_xor(gain, d, 64);
  }
  if (lane == 0) {
    const EnvHdr* h = (const EnvHdr*)e;
    int64_t* o = out + (size_t)MXA_RECORD_WORDS * i;
    o[0] = h->pops;
    o[1] = (int64_t)h->hash;
    o[2] = h->status;
    o[3] = h->cur;
    o[4] = h->status == ST_ERROR ? h->err : 0;
    o[5] = seeds[i];
    o[6] = h->last_trade;
    o[7] = h->order_counter;
    o[8] = cash;
    o[9] = shares;
    o[10] = gain;
    o[11] = 0;
  }
}

// event-class counters of an instrumented run (include/mxa.h mxa_read_counters), one wave per env
__global__ __launch_bounds__(64) void mxa_counters_kernel(const char* base, uint64_t stride, int n, uint32_t off_ag,
                                                          int n_agents, int64_t* out) {
  const int i = blockIdx.x, lane = threadIdx.x;
  if (i >= n) return;
  const char* e = base + (size_t)i * stride;
  const EnvHdr* h = (const EnvHdr*)e;
  long long w = 0;
  for (int a = lane; a < n_agents; a += 64)
    w += (long long)(((const uint32_t*)(e + off_ag + (size_t)a * MXA_AGENT_BYTES))[AF_RS_POS] - MXA_MT_N);
  for (int d = 32; d >= 1; d >>= 1) w += __shfl_xor(w, d, 64);
  int64_t* o = out + (size_t)MXA_COUNTER_WORDS * i;
  if (lane < 26) o[lane] = h->kc[lane];
  if (lane == 0) {
    for (int k = 0; k < 4; k++) w += h->rs_pos[k] - MXA_MT_N;
    const int64_t req = h->kc[MXA_KC_REQUEUE];
    o[26] = (int64_t)h->q_count - h->q0 + h->pops - req;  // every pop but a requeue removed one event
    o[27] = w - (int64_t)h->rng0;
    o[28] = h->pops;
    o[29] = h->max_q;
    o[30] = h->max_book;
    o[31] = h->kc[MXA_KC_REC];
    o[32] = h->kc[MXA_KC_RUN];
    o[33] = 0;
  }
}

// execution-agent state after a step, for a learner on the device: [n][MXA_RL_STATE_WORDS]
// doubles = (CASH, holdings, executed qty, best bid, best ask, bid size, ask size, lob flags)
// of DummyRLExecutionAgent (TradingAgent.holdings, ExecutionAgent.executed quantity,
// ABIDESEnvMetrics' newest LOB: dummy_rl:294-315, execution_agent.py:88-100)
__global__ void mxa_rl_state_kernel(const char* base, uint64_t stride, int n, uint32_t off_rec, uint64_t off_rh,
                                    uint64_t off_ring, double* out) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const char* e = base + (size_t)i * stride;
  const uint32_t* r = (const uint32_t*)(e + off_rec);
  const RpHdr* R = (const RpHdr*)(e + off_rh);
  const RpLob* L = (const RpLob*)(e + off_ring);
  auto g64 = [&](int f) { return (int64_t)(((uint64_t)r[f + 1] << 32) | r[f]); };
  double* o = out + (size_t)MXA_RL_STATE_WORDS * i;
  o[0] = (double)g64(AF_CASH);
  o[1] = (double)g64(AF_SHARES);
  o[2] = (double)R->rl_exec;
  if (R->m_cnt > 0) {
    const RpLob l = L[R->m_head];
    o[3] = (double)l.bid;
    o[4] = (double)l.ask;
    o[5] = (double)R->m_bq;
    o[6] = (double)R->m_aq;
    o[7] = (double)(l.flags & 3);
  } else {
    o[3] = o[4] = o[5] = o[6] = o[7] = 0.0;
  }
}

}  // namespace

// device memory freed with its owner (the owner's device is current then: mxa_destroy, the probes)
template <class T>
struct DevBuf {
  T* p = nullptr;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { free(); }
  hipError_t alloc(size_t n) {
    free();
    return hipMalloc(&p, sizeof(T) * n);
  }
  void free() {
    if (p) hipFree(p);
    p = nullptr;
  }
  operator T*() const { return p; }
};

// host staging of a handle's device-resident arrays (the LOBSTER tape, the ExternalFileOracle
// series): 256-byte-aligned pieces in one blob, each the RpCtx pointer `field` once uploaded
struct TapeBlob {
  std::vector<char> bytes;
  std::vector<std::pair<const void**, size_t>> fields;  // (the RpCtx pointer, its piece's offset)
  template <class T>
  void add(const T*& field, const T* src, size_t n, size_t pad = 0) {
    const size_t off = bytes.size();
    fields.push_back({(const void**)&field, off});
    bytes.resize((off + sizeof(T) * n + pad + 255) / 256 * 256, 0);
    if (n) memcpy(bytes.data() + off, src, sizeof(T) * n);
  }
};

// the handle's own stream and the timing events of its launches: the base, so that they are
// destroyed after the members' device memory is freed (hipFree waits for the device's work)
struct mxa_sync {
  hipStream_t own = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  ~mxa_sync() {
    if (ev0) hipEventDestroy(ev0);
    if (ev1) hipEventDestroy(ev1);
    if (own) hipStreamDestroy(own);
  }
};

struct mxa_handle : mxa_sync {
  MxaParams P;
  int device = 0;
  hipStream_t stream = nullptr;
  DevBuf<char> d_env;
  DevBuf<uint32_t> d_seeds;  // the seeds the next mxa_reset builds from (mxa_set_seeds)
  DevBuf<uint32_t> d_built;  // the seed each env's current episode was built from (record word 5)
  DevBuf<uint8_t> d_mask;
  DevBuf<int> d_count;
  DevBuf<int32_t> d_list;   // [n_envs] the running envs after a launch (mxa_compact_kernel)
  int64_t first_chunk = 0;  // mxa_set_launch_schedule: mxa_run's first launch (0: every launch `chunk`)
  MxaEntry e{};             // the configuration's launchers (mxa_entry.h)
  size_t lds = 0;
  DevBuf<mxa_agent_final> d_final;
  DevBuf<BlRec> d_blog;  // book-update log [n_envs][blog_cap] (mxa_set_book_log)
  int32_t blog_cap = 0;
  double last_ms = 0;
  std::string err;
  // GymKernel handles (ABIDESEnv replay, rmsc03 + DummyRL): stepped with actions
  bool gym = false;
  bool replay = false;  // the replay ladder book + tape
  RpCtx ctx{};          // host copy (pointers are device pointers)
  DevBuf<RpCtx> d_ctx;
  TapeBlob tape;  // uploaded to d_tape by create_common
  DevBuf<char> d_tape;
  DevBuf<double> d_act, d_obs;
  DevBuf<int32_t> d_flags;
  bool parity_hash = true;  // per-pop trace hash (test instrumentation); off: kernel tcap -1
  // GymKernel handles: mxa_reset continues Order.order_id / Order._order_ids of the previous
  // episode (one process running consecutive ABIDESEnv episodes)
  bool persist_ids = false;
  int32_t exlog = 0;   // mxa_set_exchange_log: the exchange's own log rides in the book-update log
  bool started = false;  // a launch ran since the last whole-handle mxa_reset (the exchange log is fixed then)
  int64_t t_stop = 0;  // mxa_set_stop_time: Kernel.runner's stopTime override (0: the config's)
  int32_t tcap_arg() const { return (parity_hash || P.L.trace_cap > 0) ? P.L.trace_cap : -1; }
  // a launcher of the current settings: the instrumented one or, with the hash off and no trace
  // ring, the one without the parity instrumentation where the configuration has it
  template <class F>
  F pick(F instr, F fast) const {
    return tcap_arg() < 0 && fast ? fast : instr;
  }
  mxa_run_fn run_kernel() const { return d_blog ? e.run_log : pick(e.run, e.run_fast); }
  // MXA_RMSC03_MM: per-env market-maker options (config/rmsc03.py --mm-*), read by every build
  std::vector<MmParams> mm;
  DevBuf<MmParams> d_mmp;
};

static int hip_fail(mxa_handle* h, hipError_t e, const char* what) {
  if (h) h->err = std::string(what) + ": " + hipGetErrorString(e);
  return MXA_EHIP;
}
#define HIPCHK(h, x)                                 \
  do {                                               \
    hipError_t _e = (x);                             \
    if (_e != hipSuccess) return hip_fail(h, _e, #x); \
  } while (0)
// every entry point that works on a handle's device starts here: the caller's current device may differ
#define ENTER(h) HIPCHK(h, hipSetDevice(h->device))

static std::string g_cfg_err;  // mxa_last_error(NULL): the last error of a call without a handle

// the one refusal, before any HIP call: "what: why" for mxa_last_error (of the handle, or of NULL)
static int refuse(mxa_handle* h, const char* what, const char* why) {
  (h ? h->err : g_cfg_err) = std::string(what) + ": " + why;
  return MXA_EINVAL;
}

// the one device-to-host path of a handle: copies on its stream, so behind everything submitted to it
// before, and finish() is the wait after the copies a reader can size (include/mxa.h, the readers)
static hipError_t dev_read(mxa_handle* h, const void* src, size_t bytes, void* dst) {
  return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream) : hipSuccess;
}
// `bytes` at `offset` of one env's block
static hipError_t env_read(mxa_handle* h, int32_t env, uint64_t offset, size_t bytes, void* dst) {
  return dev_read(h, h->d_env + (size_t)env * h->P.L.env_stride + offset, bytes, dst);
}
// the same field of every env, packed: dst [n_envs][bytes]
static hipError_t env_read_all(mxa_handle* h, uint64_t offset, size_t bytes, void* dst) {
  return hipMemcpy2DAsync(dst, bytes, h->d_env + offset, h->P.L.env_stride, bytes, h->P.n_envs, hipMemcpyDeviceToHost,
                          h->stream);
}
static hipError_t finish(mxa_handle* h) { return hipStreamSynchronize(h->stream); }

// a stream-ordered temporary, freed on its stream on every return path
struct StreamTmp {
  char* p = nullptr;
  hipStream_t stream = nullptr;
  StreamTmp() = default;
  StreamTmp(const StreamTmp&) = delete;
  StreamTmp& operator=(const StreamTmp&) = delete;
  ~StreamTmp() {
    if (p) (void)hipFreeAsync(p, stream);
  }
  hipError_t alloc(size_t bytes, hipStream_t s) {
    stream = s;
    return hipMallocAsync((void**)&p, bytes, s);
  }
};

// pops a step launch may take: a step ends at its own time (GymKernel.stepRunner), never at this
static constexpr int64_t STEP_POPS = (int64_t)1 << 40;

// the configuration's launchers (mxa_entry.h); false: not built into this library
static bool builtin_entry(int cfg, MxaEntry& e) {
  switch (cfg) {
#define MXA_ENTRY_CASE(id) \
  case id: e = MXA_ENTRY_FN(id)(); return true;
#ifdef MXA_ONLY_RMSC03
    MXA_ENTRY_CASE(MXA_ONLY_CFG)
#else
    MXA_CONFIGS(MXA_ENTRY_CASE)
#endif
  }
  return false;
}

// the one constructor: a handle bound to launchers `e` with the parameter block P sized for
// (n_envs, trace_cap).  Owned, so a constructor's early return needs no clean-up
static std::unique_ptr<mxa_handle> new_handle(const MxaEntry& e, size_t lds, const MxaParams& P, int32_t n_envs,
                                              int32_t trace_cap) {
  auto h = std::make_unique<mxa_handle>();
  h->e = e;
  h->lds = lds;
  h->P = P;
  h->P.n_envs = n_envs;
  h->P.L.trace_cap = trace_cap;
  h->P.L.env_stride = mxa_cfg::align_up(P.L.off_trace + (uint64_t)trace_cap * MXA_TRACE_ROW_BYTES, 256);
  return h;
}
// of a built-in configuration (GymKernel handles: those with a step kernel); null: not in this library
static std::unique_ptr<mxa_handle> new_handle(int cfg, int32_t n_envs, int32_t trace_cap) {
  MxaEntry e{};
  if (!builtin_entry(cfg, e)) return nullptr;
  auto h = new_handle(e, mxa_cfg::lds_bytes(cfg), mxa_cfg::params(cfg), n_envs, trace_cap);
  h->gym = e.step != nullptr;
  return h;
}

// the device side of every constructor.  *out takes the handle first: a HIP failure leaves it with
// the caller, who reads mxa_last_error and destroys it
static int create_common(std::unique_ptr<mxa_handle> owned, const uint32_t* seeds, int32_t device, mxa_handle** out) {
  mxa_handle* h = *out = owned.release();
  const int n_envs = h->P.n_envs;
  h->device = device;
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) return hip_fail(h, e, "hipSetDevice");
  HIPCHK(h, hipStreamCreateWithFlags(&h->own, hipStreamNonBlocking));
  h->stream = h->own;
  HIPCHK(h, hipEventCreate(&h->ev0));
  HIPCHK(h, hipEventCreate(&h->ev1));
  size_t bytes = (size_t)h->P.L.env_stride * n_envs;
  HIPCHK(h, h->d_env.alloc(bytes));
  HIPCHK(h, h->d_seeds.alloc(n_envs));
  HIPCHK(h, h->d_built.alloc(n_envs));
  HIPCHK(h, h->d_mask.alloc(n_envs));
  HIPCHK(h, h->d_count.alloc(1));
  HIPCHK(h, h->d_list.alloc(n_envs));
  HIPCHK(h, hipMemsetAsync(h->d_env, 0, bytes, h->stream));
  HIPCHK(h, hipMemcpyAsync(h->d_seeds, seeds, sizeof(uint32_t) * n_envs, hipMemcpyHostToDevice, h->stream));
  const TapeBlob& tape = h->tape;
  if (!tape.bytes.empty()) {
    HIPCHK(h, h->d_tape.alloc(tape.bytes.size()));
    HIPCHK(h, hipMemcpyAsync(h->d_tape, tape.bytes.data(), tape.bytes.size(), hipMemcpyHostToDevice, h->stream));
    for (auto& [field, off] : tape.fields) *field = h->d_tape + off;
  }
  if (!h->mm.empty()) {
    HIPCHK(h, h->d_mmp.alloc(n_envs));
    HIPCHK(h, hipMemcpyAsync(h->d_mmp, h->mm.data(), sizeof(MmParams) * n_envs, hipMemcpyHostToDevice, h->stream));
    h->ctx.mmp = h->d_mmp;
  }
  if (h->gym || !tape.bytes.empty() || !h->mm.empty()) {
    HIPCHK(h, h->d_ctx.alloc(1));
    HIPCHK(h, hipMemcpyAsync(h->d_ctx, &h->ctx, sizeof(RpCtx), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, h->d_act.alloc(3 * (size_t)n_envs));
    HIPCHK(h, h->d_obs.alloc(9 * (size_t)n_envs));
    HIPCHK(h, h->d_flags.alloc(n_envs));
    HIPCHK(h, finish(h));
  }
  const int rc = mxa_reset(h, nullptr);  // a fresh process: ids from 0
  h->persist_ids = h->gym;               // later resets continue the process (Order.py:8-9)
  return rc;
}

// one launch between the handle's timing events (mxa_last_kernel_ms reads their distance)
template <class Launch>
static int timed_launch(mxa_handle* h, Launch launch) {
  HIPCHK(h, hipEventRecord(h->ev0, h->stream));
  launch();
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipEventRecord(h->ev1, h->stream));
  return MXA_OK;
}
// the time of the last timed_launch, once the stream is synchronised: added to *sum, or (no sum) what
// mxa_last_kernel_ms returns
static int launch_ms(mxa_handle* h, float* sum = nullptr) {
  float ms = 0;
  HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
  if (sum) *sum += ms;
  else h->last_ms = ms;
  return MXA_OK;
}

// a step launch of a GymKernel handle: the arguments every step launcher starts with, then `tail`.
// A null launcher (a library built without the step kernels, a configuration without this one) refuses
template <class F, class... Tail>
static int step_launch(mxa_handle* h, F instr, F fast, Tail... tail) {
  if (!instr) return MXA_EINVAL;
  ENTER(h);
  return timed_launch(h, [&] {
    h->pick(instr, fast)(dim3(h->P.n_envs), dim3(64), h->lds, h->stream, h->d_env, h->P.L.env_stride, h->P.n_envs,
                         h->tcap_arg(), STEP_POPS, h->d_ctx, tail...);
  });
}

// the handle's header settings into every env (after a build cleared headers, or a new setting)
static int set_headers(mxa_handle* h) {
  const int n = h->P.n_envs;
  hipLaunchKernelGGL(mxa_set_header_kernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->d_env, h->P.L.env_stride,
                     n, h->exlog, h->t_stop);
  HIPCHK(h, hipGetLastError());
  return MXA_OK;
}

extern "C" {

#ifdef MXA_PROF
// diagnostics build only (not in include/mxa.h): phase cycle totals, then cleared
int mxa_prof_read(uint64_t* out64) {
  if (hipMemcpyFromSymbol(out64, HIP_SYMBOL(mxa::g_mxa_prof), 128 * 8) != hipSuccess) return MXA_EHIP;
  static const uint64_t z[128] = {0};
  if (hipMemcpyToSymbol(HIP_SYMBOL(mxa::g_mxa_prof), z, 128 * 8) != hipSuccess) return MXA_EHIP;
  return MXA_OK;
}
#endif

int mxa_create(int32_t config, int32_t n_envs, const uint32_t* seeds, int32_t device, int32_t trace_cap,
               mxa_handle** out) {
  if (!out || n_envs <= 0 || !seeds || trace_cap < 0) return MXA_EINVAL;
  static_assert((int)MXA_RMSC03 == (int)MXA_CFG_RMSC03 && (int)MXA_SPARSE_ZI_100 == (int)MXA_CFG_SPARSE_ZI_100 &&
                    (int)MXA_SPARSE_ZI_1000 == (int)MXA_CFG_SPARSE_ZI_1000 &&
                    (int)MXA_MARKETREPLAY == (int)MXA_CFG_MARKETREPLAY && (int)MXA_RMSC03_RL == (int)MXA_CFG_RMSC03_RL &&
                    (int)MXA_VALUE_NOISE == (int)MXA_CFG_VALUE_NOISE && (int)MXA_RMSC01 == (int)MXA_CFG_RMSC01 &&
                    (int)MXA_RMSC02 == (int)MXA_CFG_RMSC02 && (int)MXA_OBI_RMSC02 == (int)MXA_CFG_OBI_RMSC02 &&
                    (int)MXA_RANDOM_FUND_VALUE == (int)MXA_CFG_RANDOM_FUND_VALUE &&
                    (int)MXA_RANDOM_FUND_DIVERSE == (int)MXA_CFG_RANDOM_FUND_DIVERSE &&
                    (int)MXA_HIST_FUND_VALUE == (int)MXA_CFG_HIST_FUND_VALUE &&
                    (int)MXA_HIST_FUND_DIVERSE == (int)MXA_CFG_HIST_FUND_DIVERSE &&
                    (int)MXA_MARKETREPLAY_RUNNER == (int)MXA_CFG_MARKETREPLAY_RUNNER &&
                    (int)MXA_MARKETREPLAY_TWAP == (int)MXA_CFG_MARKETREPLAY_TWAP &&
                    (int)MXA_RMSC03_SBMM == (int)MXA_CFG_RMSC03_SBMM &&
                    (int)MXA_RMSC03_SBMM_POLL == (int)MXA_CFG_RMSC03_SBMM_POLL &&
                    (int)MXA_RMSC03_MM == (int)MXA_CFG_RMSC03_MM,
                "config ids");
  static_assert(MXA_N_CONFIGS == (int)MXA_CFG_RMSC03_MM + 1, "one entry per configuration");
  static_assert(sizeof(mxa_mm_params) == sizeof(MmParams) && offsetof(mxa_mm_params, mm_wake_up_freq_ns) ==
                    offsetof(MmParams, wake_up_freq) && offsetof(mxa_mm_params, mm_num_ticks) == offsetof(MmParams, num_ticks),
                "mxa_mm_params is MmParams");
  if (config == MXA_RMSC03_MM) {  // the config script's defaults in every env
    std::vector<mxa_mm_params> d(n_envs, mxa_mm_defaults());
    return mxa_create_params(MXA_RMSC03, n_envs, seeds, d.data(), device, trace_cap, out);
  }
  // replay handles: mxa_create_replay(_runner); ExternalFileOracle configurations: mxa_create_hist
  if (config == MXA_MARKETREPLAY || config == MXA_MARKETREPLAY_RUNNER || config == MXA_MARKETREPLAY_TWAP ||
      config == MXA_HIST_FUND_VALUE || config == MXA_HIST_FUND_DIVERSE)
    return MXA_EINVAL;
  auto h = new_handle(config, n_envs, trace_cap);
  if (!h) return MXA_EINVAL;
  if (h->gym) {  // the DummyRL metrics header + deque after the trace (no ladder, no tape)
    h->ctx.L = mxa_cfg::replay_layout(h->P.L.env_stride, 0, 0, 0, 0, 0, 0, 0);
    h->P.L.env_stride = h->ctx.L.end;
  }
  return create_common(std::move(h), seeds, device, out);
}

static int check_mm(const mxa_mm_params* p, int n) {
  for (int i = 0; i < n; i++) {
    const mxa_mm_params& x = p[i];
    // the reference raises nowhere on these, but a negative window / tick count, a
    // non-positive wake-up period or a NaN / negative pov is no option the script can run.  A pov
    // whose order size outgrows the 32-bit order words stops that env with MXA_ERR_ORDER_SIZE
    // at the order (the cap here only keeps pov x volume exact in a double)
    if (!(x.mm_pov == x.mm_pov) || x.mm_pov < 0 || x.mm_pov > 1e12 || x.mm_min_order_size < 0 || x.mm_window_size < 0 ||
        x.mm_num_ticks < 0 || x.mm_num_ticks > 100000 || x.mm_wake_up_freq_ns <= 0)
      return MXA_EINVAL;
  }
  return MXA_OK;
}

mxa_mm_params mxa_mm_defaults(void) {
  mxa_mm_params p{};
  const MxaParams P = mxa_cfg::params(MXA_CFG_RMSC03);
  p.mm_pov = P.mm_pov;
  p.mm_min_order_size = P.mm_min_size;
  p.mm_window_size = P.mm_window;
  p.mm_num_ticks = P.mm_ticks;
  p.mm_wake_up_freq_ns = P.mm_wake;
  return p;
}

// config/rmsc03.py with each env's market-maker options; see include/mxa.h
int mxa_create_params(int32_t config, int32_t n_envs, const uint32_t* seeds, const mxa_mm_params* per_env,
                      int32_t device, int32_t trace_cap, mxa_handle** out) {
  if (!out || n_envs <= 0 || !seeds || !per_env || trace_cap < 0 || config != MXA_RMSC03) return MXA_EINVAL;
  if (check_mm(per_env, n_envs)) return MXA_EINVAL;
  auto h = new_handle(MXA_CFG_RMSC03_MM, n_envs, trace_cap);
  if (!h) return MXA_EINVAL;
  h->mm.assign((const MmParams*)per_env, (const MmParams*)per_env + n_envs);
  return create_common(std::move(h), seeds, device, out);
}

int mxa_set_mm_params(mxa_handle* h, const mxa_mm_params* per_env) {
  if (!h || !per_env || !h->d_mmp) return MXA_EINVAL;
  if (check_mm(per_env, h->P.n_envs)) return MXA_EINVAL;
  ENTER(h);
  memcpy(h->mm.data(), per_env, sizeof(MmParams) * h->P.n_envs);
  HIPCHK(h, hipMemcpyAsync(h->d_mmp, h->mm.data(), sizeof(MmParams) * h->P.n_envs, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, finish(h));
  return MXA_OK;
}

int mxa_resident_envs(const mxa_handle* h) {
  if (!h || !h->e.occ) return MXA_EINVAL;
  int dev = 0, cus = 0;
  // (a const handle: ENTER's error text has nowhere to go)
  if (hipSetDevice(h->device) != hipSuccess || hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    return MXA_EHIP;
  const int per_cu = h->e.occ(h->lds);
  if (per_cu < 0) return MXA_EHIP;
  return per_cu * cus < h->P.n_envs ? per_cu * cus : h->P.n_envs;
}

// config/hist_fund_value.py / hist_fund_diverse.py: the ExternalFileOracle's series is the
// handle's (shared by its envs, device-resident); see include/mxa.h
int mxa_create_hist(int32_t config, int32_t n_envs, const uint32_t* seeds, int32_t device, int32_t trace_cap,
                    const int64_t* fund_t, const double* fund_v, int32_t n_fund, mxa_handle** out) {
  if (!out || n_envs <= 0 || !seeds || trace_cap < 0 || !fund_t || !fund_v || n_fund <= 0) return MXA_EINVAL;
  if (config != MXA_HIST_FUND_VALUE && config != MXA_HIST_FUND_DIVERSE) return MXA_EINVAL;
  for (int i = 0; i < n_fund; i++)
    if ((i && fund_t[i] < fund_t[i - 1]) || !(fund_v[i] == fund_v[i]) || fund_v[i] > 1e15 || fund_v[i] < -1e15)
      return MXA_EINVAL;  // unsorted times or a value int(round()) cannot take (NaN raises in the reference)
  auto h = new_handle(config, n_envs, trace_cap);
  if (!h) return MXA_EINVAL;
  h->tape.add(h->ctx.fs_t, fund_t, n_fund);
  h->tape.add(h->ctx.fs_v, fund_v, n_fund);
  h->ctx.fs_n = n_fund;
  return create_common(std::move(h), seeds, device, out);
}

// ---- runtime compositions (include/mxa.h mxa_config): one specialised library per composition
#ifndef MXA_BUILD_ID
#define MXA_BUILD_ID "unknown"
#endif
// the compile line of a specialisation: build_lib.py's flags (passed in when this file is
// compiled), per base configuration its extra flags ("<cfg>:<flags>;...")
#ifndef MXA_JIT_FLAGS
#define MXA_JIT_FLAGS "--offload-arch=gfx950 -O3 -std=c++20"
#endif
#ifndef MXA_JIT_CFG_FLAGS
#define MXA_JIT_CFG_FLAGS ""
#endif
static int cfg_fail(const std::string& what) {
  g_cfg_err = what;
  return MXA_EINVAL;
}

// the directory holding this library (lib/), from which csrc/ and include/ are found
static std::string lib_dir() {
  Dl_info di{};
  if (!dladdr((void*)&mxa_config_defaults, &di) || !di.dli_fname) return ".";
  std::string p = di.dli_fname;
  const size_t k = p.rfind('/');
  return k == std::string::npos ? "." : p.substr(0, k);
}

static std::vector<std::string> split_ws(const std::string& s) {
  std::vector<std::string> v;
  size_t i = 0;
  while (i < s.size()) {
    while (i < s.size() && s[i] == ' ') i++;
    size_t j = i;
    while (j < s.size() && s[j] != ' ') j++;
    if (j > i) v.push_back(s.substr(i, j - i));
    i = j;
  }
  return v;
}

static std::string cfg_key(const mxa_config& c) {
  mxa_config k = c;
  k.date_ns = 0;  // output timestamps only: one specialisation serves every date
  uint64_t h = 0xCBF29CE484222325ull;
  const unsigned char* b = (const unsigned char*)&k;
  for (size_t i = 0; i < sizeof k; i++) h = (h ^ b[i]) * 0x100000001B3ull;
  for (const char* p = MXA_BUILD_ID; *p; p++) h = (h ^ (unsigned char)*p) * 0x100000001B3ull;
  char buf[17];
  snprintf(buf, sizeof buf, "%016llx", (unsigned long long)h);
  return buf;
}

static std::string cfg_dir(const char* cache_dir) { return cache_dir && *cache_dir ? cache_dir : lib_dir() + "/custom"; }
static std::string cfg_lib(const char* cache_dir, const std::string& key) {
  return cfg_dir(cache_dir) + "/libmxa_cfg_" + key + ".so";
}

int mxa_config_defaults(int32_t base, mxa_config* out) {
  if (!out || !mxa_cfg::custom_base_ok(base)) return cfg_fail("mxa_config_defaults: no such base script");
  static_assert(sizeof(mxa_config) % 8 == 0, "mxa_config: no tail padding (its bytes are the cache key)");
  mxa_cfg::config_defaults(base, *out);
  return MXA_OK;
}

int mxa_config_key(const mxa_config* cfg, char* out17) {
  if (!cfg || !out17) return MXA_EINVAL;
  snprintf(out17, 17, "%s", cfg_key(*cfg).c_str());
  return MXA_OK;
}

int mxa_config_capacities(const mxa_config* cfg, int32_t out2[2]) {
  if (!cfg || !out2) return cfg_fail("mxa_config_capacities: bad arguments");
  if (const char* why = mxa_cfg::custom_check(*cfg)) return refuse(nullptr, "mxa_config_capacities", why);
  const mxa_cfg::Shape S = mxa_cfg::custom_shape(*cfg);
  out2[0] = S.sq * 64;
  out2[1] = S.so * 64;
  return MXA_OK;
}

int mxa_config_compile(const mxa_config* cfg, const char* cache_dir, char* path_out, int32_t path_cap) {
  if (!cfg) return cfg_fail("mxa_config_compile: null composition");
  if (const char* why = mxa_cfg::custom_check(*cfg)) return refuse(nullptr, "mxa_config_compile", why);
  const std::string key = cfg_key(*cfg), dir = cfg_dir(cache_dir), so = cfg_lib(cache_dir, key);
  if (path_out && path_cap > 0) snprintf(path_out, path_cap, "%s", so.c_str());
  struct stat st{};
  if (stat(so.c_str(), &st) == 0) return MXA_OK;  // compiled before
  mkdir(dir.c_str(), 0755);
  const std::string hdr = dir + "/mxa_cfg_" + key + ".h";
  {
    FILE* f = fopen(hdr.c_str(), "w");
    if (!f) return cfg_fail("mxa_config_compile: cannot write " + hdr);
    fprintf(f, "// a runtime composition (include/mxa.h mxa_config), written by mxa_config_compile\n");
    fprintf(f, "#define MXA_CUSTOM_BYTES {");
    const unsigned char* b = (const unsigned char*)cfg;
    for (size_t i = 0; i < sizeof(mxa_config); i++) fprintf(f, "%s%u", i ? "," : "", b[i]);
    fprintf(f, "}\n");
    fclose(f);
  }
  const std::string ld = lib_dir(), src = ld + "/../csrc", inc = ld + "/../../include";
  const char* hipcc = getenv("HIPCC");
  std::vector<std::string> argv = {hipcc && *hipcc ? hipcc : "/opt/rocm/bin/hipcc"};
  for (auto& x : split_ws(MXA_JIT_FLAGS)) argv.push_back(x);
  {  // the base's own backend flags
    const std::string all = MXA_JIT_CFG_FLAGS, pre = std::to_string(cfg->base) + ":";
    size_t i = 0;
    while (i < all.size()) {
      size_t j = all.find(';', i);
      if (j == std::string::npos) j = all.size();
      const std::string item = all.substr(i, j - i);
      if (item.compare(0, pre.size(), pre) == 0)
        for (auto& x : split_ws(item.substr(pre.size()))) argv.push_back(x);
      i = j + 1;
    }
  }
  const std::string tmp = so + ".tmp." + std::to_string((long)getpid());
  for (const std::string& x : {std::string("-fvisibility=hidden"), std::string("-fvisibility-inlines-hidden"),
                               std::string("-Wl,-Bsymbolic"), std::string("-shared"),
                               "-DMXA_INST_CFG=" + std::to_string(cfg->base), "-DMXA_CUSTOM_HDR=\"" + hdr + "\"",
                               std::string("-DMXA_BUILD_ID=\"") + MXA_BUILD_ID + "\"", "-I" + src, "-I" + inc,
                               src + "/mxa_inst.hip", std::string("-o"), tmp})
    argv.push_back(x);
  std::vector<char*> av;
  for (auto& x : argv) av.push_back((char*)x.c_str());
  av.push_back(nullptr);
  pid_t pid = 0;
  // a child process (posix_spawn), never an exec of this one
  if (posix_spawn(&pid, av[0], nullptr, nullptr, av.data(), environ) != 0)
    return cfg_fail("mxa_config_compile: cannot start " + argv[0]);
  int status = 0;
  if (waitpid(pid, &status, 0) < 0 || !WIFEXITED(status) || WEXITSTATUS(status) != 0) {
    unlink(tmp.c_str());
    std::string cmd;
    for (auto& x : argv) cmd += x + " ";
    return cfg_fail("mxa_config_compile: the compile failed: " + cmd);
  }
  if (rename(tmp.c_str(), so.c_str()) != 0) return cfg_fail("mxa_config_compile: cannot place " + so);
  return MXA_OK;
}

typedef int (*mxa_custom_entry_fn)(MxaEntry*, MxaParams*, size_t*, mxa_config*, const char**);

int mxa_create_config(const mxa_config* cfg, int32_t n_envs, const uint32_t* seeds, int32_t device, int32_t trace_cap,
                      const char* cache_dir, mxa_handle** out) {
  if (!out || n_envs <= 0 || !seeds || trace_cap < 0 || !cfg) return cfg_fail("mxa_create_config: bad arguments");
  if (const char* why = mxa_cfg::custom_check(*cfg)) return refuse(nullptr, "mxa_create_config", why);
  const std::string key = cfg_key(*cfg), so = cfg_lib(cache_dir, key);
  static std::mutex mu;
  static std::map<std::string, void*> loaded;  // specialisations stay loaded: their kernels are registered
  void* dl = nullptr;
  {
    std::lock_guard<std::mutex> g(mu);
    auto it = loaded.find(so);
    if (it != loaded.end()) {
      dl = it->second;
    } else {
      struct stat st{};
      if (stat(so.c_str(), &st) != 0) {
        g_cfg_err = "mxa_create_config: not compiled (mxa_config_compile first): " + so;
        return MXA_ERANGE;
      }
      dl = dlopen(so.c_str(), RTLD_NOW | RTLD_LOCAL);
      if (!dl) return cfg_fail(std::string("mxa_create_config: dlopen: ") + dlerror());
      loaded[so] = dl;
    }
  }
  auto fn = (mxa_custom_entry_fn)dlsym(dl, "mxa_custom_entry");
  if (!fn) return cfg_fail("mxa_create_config: " + so + " is not a specialisation");
  MxaEntry e{};
  MxaParams P{};
  size_t lds = 0;
  mxa_config c{};
  const char* bid = nullptr;
  if (fn(&e, &P, &lds, &c, &bid) != (int)sizeof(MxaParams) || !bid || strcmp(bid, MXA_BUILD_ID) != 0)
    return cfg_fail("mxa_create_config: " + so + " was built by another libmxa");
  c.date_ns = cfg->date_ns;
  if (memcmp(&c, cfg, sizeof c) != 0) return cfg_fail("mxa_create_config: " + so + " holds another composition");
  // a plain Kernel.runner handle whatever the entry holds: compositions are no GymKernel handles
  return create_common(new_handle(e, lds, P, n_envs, trace_cap), seeds, device, out);
}

int mxa_config_info(int32_t config, int64_t* out8) {
  if (!out8 || config < 0 || config >= MXA_N_CONFIGS) return MXA_EINVAL;
  const MxaParams P = mxa_cfg::params(config);
  const mxa_cfg::Shape S = mxa_cfg::shape(config);
  out8[0] = P.n_agents;
  out8[1] = P.ex_log_orders;
  out8[2] = (int64_t)S.sq * 64;
  out8[3] = (int64_t)S.so * 64;
  out8[4] = P.mkt_open;
  out8[5] = P.mkt_close;
  out8[6] = P.start;
  out8[7] = P.stop;
  return MXA_OK;
}

// ABIDESEnv on a LOBSTER tape (agent_config.py / ABIDESEnv.py), or config/marketreplay.py under
// Kernel.runner (cfg MXA_CFG_MARKETREPLAY_RUNNER); see include/mxa.h
static int create_replay(int cfg, const int64_t* t, const int64_t* oid, const int64_t* price, const int64_t* size,
                         const int8_t* buy, int32_t n_rec, int32_t n_envs, int32_t device, int32_t trace_cap,
                         mxa_handle** out, int32_t twap_trade = 0);
int mxa_create_replay(const int64_t* t, const int64_t* oid, const int64_t* price, const int64_t* size,
                      const int8_t* buy, int32_t n_rec, int32_t n_envs, int32_t device, int32_t trace_cap,
                      mxa_handle** out) {
  return create_replay(MXA_CFG_MARKETREPLAY, t, oid, price, size, buy, n_rec, n_envs, device, trace_cap, out);
}
int mxa_create_replay_runner(const int64_t* t, const int64_t* oid, const int64_t* price, const int64_t* size,
                             const int8_t* buy, int32_t n_rec, int32_t n_envs, int32_t device, int32_t trace_cap,
                             mxa_handle** out) {
  return create_replay(MXA_CFG_MARKETREPLAY_RUNNER, t, oid, price, size, buy, n_rec, n_envs, device, trace_cap, out);
}
int mxa_create_replay_twap(const int64_t* t, const int64_t* oid, const int64_t* price, const int64_t* size,
                           const int8_t* buy, int32_t n_rec, int32_t trade, int32_t n_envs, int32_t device,
                           int32_t trace_cap, mxa_handle** out) {
  return create_replay(MXA_CFG_MARKETREPLAY_TWAP, t, oid, price, size, buy, n_rec, n_envs, device, trace_cap, out,
                       trade != 0);
}
static int create_replay(int cfg, const int64_t* t, const int64_t* oid, const int64_t* price, const int64_t* size,
                         const int8_t* buy, int32_t n_rec, int32_t n_envs, int32_t device, int32_t trace_cap,
                         mxa_handle** out, int32_t twap_trade) {
  if (!out || !t || !oid || !price || !size || !buy || n_rec <= 0 || n_envs <= 0 || trace_cap < 0) return MXA_EINVAL;
  int64_t pmin = INT64_MAX, pmax = INT64_MIN, min_id = INT64_MAX;
  int n_zero = 0;  // ORDER_ID 0 records: LimitOrder(order_id=0) takes an auto id (Order.py:26)
  for (int i = 0; i < n_rec; i++) {
    if ((i && t[i] < t[i - 1]) || oid[i] < 0 || oid[i] >= INT32_MAX || size[i] < 0 || size[i] >= INT32_MAX ||
        price[i] < 0 || price[i] >= (1 << 20))
      return MXA_EINVAL;  // unsorted tape or out-of-range fields
    pmin = std::min(pmin, price[i]);
    pmax = std::max(pmax, price[i]);
    if (oid[i] == 0) n_zero++;
    else min_id = std::min(min_id, oid[i]);
  }
  const MxaParams P0 = mxa_cfg::params(cfg);
  // auto ids (DummyRL's orders and the tape's ORDER_ID 0 records) count up from 0 in one
  // global sequence; Order.generateOrderId would skip explicit tape ids it met, which cannot
  // happen while every auto id stays below the smallest tape id
  const int64_t auto_cap = (int64_t)P0.rl_ids + n_zero;
  if (min_id <= auto_cap) return MXA_EINVAL;
  // Order._order_ids of the tape (for later episodes of a process): each explicit id with its
  // first SIZE > 0 record, sorted by id
  std::vector<std::pair<int32_t, int32_t>> uf;
  for (int i = 0; i < n_rec; i++)
    if (oid[i] != 0 && size[i] > 0) uf.push_back({(int32_t)oid[i], i});
  std::sort(uf.begin(), uf.end());
  uf.erase(std::unique(uf.begin(), uf.end(), [](const std::pair<int32_t, int32_t>& a, const std::pair<int32_t, int32_t>& b) {
             return a.first == b.first;
           }),
           uf.end());  // sorted by (id, record): the first of each id is kept
  auto h = new_handle(cfg, n_envs, trace_cap);
  if (!h) return MXA_EINVAL;
  h->replay = true;
  // dense order-id index in first-appearance order; distinct times and their first records
  std::vector<int32_t> dense(n_rec), tm0;
  std::vector<int64_t> tm;
  std::vector<std::pair<int64_t, int32_t>> ids;
  ids.reserve(n_rec);
  for (int i = 0; i < n_rec; i++)
    if (oid[i] != 0) ids.push_back({oid[i], i});
  std::sort(ids.begin(), ids.end());
  int n_ids = 0;
  for (size_t i = 0; i < ids.size(); i++) {
    if (i == 0 || ids[i].first != ids[i - 1].first) n_ids++;
    dense[ids[i].second] = n_ids - 1;
  }
  // ORDER_ID 0 records look up `orders.get(0)`: the order whose auto id is 0, which sits at
  // the first auto-id dense index
  for (int i = 0; i < n_rec; i++)
    if (oid[i] == 0) dense[i] = n_ids;
  for (int i = 0; i < n_rec; i++)
    if (i == 0 || t[i] != t[i - 1]) {
      tm.push_back(t[i]);
      tm0.push_back(i);
    }
  tm0.push_back(n_rec);
  const int ntm = (int)tm.size();
  const int C = n_rec + h->P.rl_ids;  // every placement could rest at once
  // auto-id dense range: the episode's auto ids, the explicit ids they may skip over in a later
  // episode (MXA_AUTO_SKIP), and one never-present index (orders.get(0) without an auto id 0)
  h->ctx.L = mxa_cfg::replay_layout(h->P.L.env_stride, (int)pmin, (int)(pmax - pmin + 1), C, n_ids,
                                    (int)auto_cap + MXA_AUTO_SKIP + 1, ntm, n_rec);
  h->ctx.nuid = (int32_t)uf.size();
  h->ctx.twap_trade = twap_trade;
  h->ctx.umin = uf.empty() ? INT32_MAX : uf[0].first;
  h->P.L.env_stride = h->ctx.L.end;
  // the tape in the device's word sizes, then the blob in this order
  std::vector<int32_t> oid32(oid, oid + n_rec), price32(price, price + n_rec), size32(size, size + n_rec), uid, ufirst;
  std::vector<int8_t> buy8(n_rec);
  for (int i = 0; i < n_rec; i++) buy8[i] = buy[i] ? 1 : 0;
  for (auto& u : uf) {
    uid.push_back(u.first);
    ufirst.push_back(u.second);
  }
  RpCtx& c = h->ctx;
  h->tape.add(c.t, t, n_rec);
  h->tape.add(c.oid, oid32.data(), n_rec);
  h->tape.add(c.dense, dense.data(), n_rec);
  h->tape.add(c.price, price32.data(), n_rec);
  h->tape.add(c.size, size32.data(), n_rec);
  h->tape.add(c.buy, buy8.data(), n_rec);
  h->tape.add(c.tm, tm.data(), ntm);
  h->tape.add(c.tm0, tm0.data(), ntm + 1);
  h->tape.add(c.uid, uid.data(), uid.size(), 4);  // (one spare word each: the pieces are never empty)
  h->tape.add(c.ufirst, ufirst.data(), ufirst.size(), 4);
  std::vector<uint32_t> seeds(n_envs, 0u);  // nothing in this composition draws
  return create_common(std::move(h), seeds.data(), device, out);
}

// ABIDESEnv.step for every env: actions [n][3] -> obs [n][9], flags [n] (all host arrays)
int mxa_step(mxa_handle* h, const double* actions, double* obs, int32_t* flags) {
  if (!h || !h->gym || !actions || !obs || !flags) return MXA_EINVAL;
  ENTER(h);
  int n = h->P.n_envs;
  HIPCHK(h, hipMemcpyAsync(h->d_act, actions, sizeof(double) * 3 * n, hipMemcpyHostToDevice, h->stream));
  int rc = mxa_step_device(h, h->d_act, h->d_obs, h->d_flags);
  if (rc) return rc;
  HIPCHK(h, dev_read(h, h->d_obs, sizeof(double) * 9 * n, obs));
  HIPCHK(h, dev_read(h, h->d_flags, sizeof(int32_t) * n, flags));
  HIPCHK(h, finish(h));
  return launch_ms(h);
}

// k consecutive steps in one launch, device arrays: actions [k][n][3] -> obs [k][n][9], flags [k][n]
int mxa_step_many(mxa_handle* h, int32_t k, const double* d_actions, double* d_obs, int32_t* d_flags) {
  if (!h || !h->gym || k <= 0 || !d_actions || !d_obs || !d_flags) return MXA_EINVAL;
  return step_launch(h, h->e.step_many, h->e.step_many_fast, d_actions, d_obs, d_flags, (int)k);
}

// k periods in one launch with the epsilon-greedy Q-network policy evaluated in the step kernel
// (include/mxa.h): every argument is checked before the first HIP call
int mxa_step_policy(mxa_handle* h, int32_t k, int32_t first_zero, const mxa_policy* p, double* d_obs, int32_t* d_flags,
                    int64_t* d_a, double* d_act, double* d_state) {
  if (!h || !h->gym || k <= 0 || !p || !d_obs || !d_flags || !d_a || !d_act) return MXA_EINVAL;
  if (!p->params || !p->grid0 || !p->grid1 || !p->table || p->n0 < 0 || p->n1 < 0) return MXA_EINVAL;
  if (!p->test && (!p->u || !p->rnd || !p->eps)) return MXA_EINVAL;
  if (!qwave::dims_ok(p->n_layers, p->dims) || p->dims[0] != 2) return MXA_EINVAL;
  if (d_state && h->P.n_rl != 1) return MXA_EINVAL;  // the rl-state row is the one execution agent's
  return step_launch(h, h->e.step_policy, h->e.step_policy_fast, *p, d_obs, d_flags, d_a, d_act, d_state, (int)k,
                     (int)(first_zero != 0));
}

// mxa_step_policy with the state of a spec (include/mxa_policy_features.h): every refusal carries
// its message and comes before the first HIP call
int mxa_step_policy_spec(mxa_handle* h, int32_t k, int32_t first_zero, const mxa_policy* p, const mxa_state_spec* spec,
                         double* d_obs, int32_t* d_flags, int64_t* d_a, double* d_act, double* d_state) {
  static const char* const fn = "mxa_step_policy_spec";
  if (!h) return refuse(nullptr, fn, "null handle");
  if (!h->gym) return refuse(h, fn, "not a GymKernel handle");
  if (k <= 0) return refuse(h, fn, "k <= 0");
  if (!p || !d_obs || !d_flags || !d_a || !d_act) return refuse(h, fn, "a null policy or output array");
  if (!p->params || !p->table) return refuse(h, fn, "null parameters or action table");
  if (!p->test && (!p->u || !p->rnd || !p->eps)) return refuse(h, fn, "train mode with a null u, rnd or eps");
  if (!qwave::dims_ok(p->n_layers, p->dims)) return refuse(h, fn, "dimensions outside 1..8 layers of 1..256 units");
  if (const char* why = mxa_state_spec_refusal(spec, 9)) return refuse(h, fn, why);
  if (p->dims[0] != spec->n_feat) return refuse(h, fn, "dims[0] != n_feat");
  if (d_state && h->P.n_rl != 1) return refuse(h, fn, "an rl-state array on a handle without one execution agent");
  if (!h->e.step_policy_spec) return refuse(h, fn, "the library was built without the step kernels");
  return step_launch(h, h->e.step_policy_spec, h->e.step_policy_spec_fast, *p, *spec, d_obs, d_flags, d_a, d_act,
                     d_state, (int)k, (int)(first_zero != 0));
}

// the same with device arrays (e.g. torch tensors), asynchronous on the handle's stream
int mxa_step_device(mxa_handle* h, const double* d_actions, double* d_obs, int32_t* d_flags) {
  if (!h || !h->gym) return MXA_EINVAL;
  return step_launch(h, h->e.step, h->e.step_fast, d_actions, d_obs, d_flags);
}

int mxa_reset(mxa_handle* h, const uint8_t* mask) {
  if (!h) return MXA_EINVAL;
  ENTER(h);
  const int n = h->P.n_envs;
  const uint8_t* dm = nullptr;
  if (mask || h->persist_ids) {
    // 1: rebuild the env; 2 (persist_ids): rebuild it and keep its order-id counters
    const uint8_t on = h->persist_ids ? 2 : 1;
    std::vector<uint8_t> m(n);
    for (int i = 0; i < n; i++) m[i] = (!mask || mask[i]) ? on : 0;
    HIPCHK(h, hipMemcpyAsync(h->d_mask, m.data(), n, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, finish(h));  // m is a host temporary
    dm = h->d_mask;
  }
  h->e.build(dim3(n), dim3(64), h->lds, h->stream, h->d_env, h->P.L.env_stride, n, h->d_seeds, dm, h->d_ctx);
  HIPCHK(h, hipGetLastError());
  hipLaunchKernelGGL(mxa_built_seeds_kernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->d_built, h->d_seeds,
                     dm, n);
  HIPCHK(h, hipGetLastError());
  if (!mask) h->started = false;
  // the build cleared the header: the exchange-log switch and the stopTime override outlive resets
  if (h->exlog || h->t_stop > 0)
    if (int rc = set_headers(h)) return rc;
  HIPCHK(h, finish(h));
  return MXA_OK;
}

int mxa_set_stop_time(mxa_handle* h, int64_t t_stop_ns) {
  if (!h || h->gym) return MXA_EINVAL;  // GymKernel handles: ABIDESEnv's own stop (ABIDESEnv.py:42-46)
  ENTER(h);
  h->t_stop = t_stop_ns > 0 ? t_stop_ns : 0;
  if (int rc = set_headers(h)) return rc;
  HIPCHK(h, finish(h));
  return MXA_OK;
}

int mxa_run_until(mxa_handle* h, int64_t t_stop_ns, int64_t* events_out) {
  if (!h || h->gym) return MXA_EINVAL;
  int rc = mxa_set_stop_time(h, t_stop_ns);
  if (rc != MXA_OK) return rc;
  if ((rc = mxa_run(h, (int64_t)1 << 20, 0, nullptr)) != MXA_OK) return rc;
  if (events_out) {
    const int n = h->P.n_envs;
    std::vector<mxa_env_summary> s(n);
    if ((rc = mxa_read_summary(h, s.data())) != MXA_OK) return rc;
    for (int i = 0; i < n; i++) events_out[i] = s[i].events;
  }
  return MXA_OK;
}

int mxa_set_id_persistence(mxa_handle* h, int32_t on) {
  if (!h || (on && !h->gym)) return MXA_EINVAL;
  h->persist_ids = on != 0;
  return MXA_OK;
}

int mxa_launch(mxa_handle* h, int64_t max_pops) {
  if (!h || h->gym) return MXA_EINVAL;  // GymKernel handles advance by mxa_step
  ENTER(h);
  h->started = true;
  h->run_kernel()(dim3(h->P.n_envs), dim3(64), h->lds, h->stream, h->d_env, h->P.L.env_stride, h->P.n_envs, h->tcap_arg(), max_pops,
         h->d_ctx, h->d_blog, h->blog_cap, nullptr);
  HIPCHK(h, hipGetLastError());
  return MXA_OK;
}

int mxa_sync(mxa_handle* h) {
  if (!h) return MXA_EINVAL;
  ENTER(h);
  HIPCHK(h, finish(h));
  return MXA_OK;
}

int mxa_run(mxa_handle* h, int64_t chunk, int32_t max_launches, int32_t* launches_out) {
  if (!h || chunk <= 0 || h->gym) return MXA_EINVAL;
  ENTER(h);
  int launches = 0;
  float total = 0;
  h->started = true;
  const int n = h->P.n_envs;
  // the envs still running (an earlier mxa_run / mxa_launch may have finished some)
  auto compact = [&](int& running) -> int {
    hipLaunchKernelGGL(mxa_compact_kernel, dim3(1), dim3(1024), 0, h->stream, h->d_env, h->P.L.env_stride, n,
                       h->d_list, h->d_count);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, dev_read(h, h->d_count, sizeof(int), &running));
    HIPCHK(h, finish(h));
    if (running < 0 || running > n) {
      h->err = "mxa_run: running-env count out of range";
      return MXA_EHIP;
    }
    return MXA_OK;
  };
  int running = 0, rc;
  if ((rc = compact(running)) != MXA_OK) return rc;
  int64_t pops = h->first_chunk > 0 ? std::min(chunk, h->first_chunk) : chunk;
  while (running > 0) {
    if (max_launches > 0 && launches >= max_launches) break;
    // one wave per running env: every env (no list) while none has finished
    rc = timed_launch(h, [&] {
      h->run_kernel()(dim3(running), dim3(64), h->lds, h->stream, h->d_env, h->P.L.env_stride, n, h->tcap_arg(), pops,
                      h->d_ctx, h->d_blog, h->blog_cap, running == n ? nullptr : (const int32_t*)h->d_list);
    });
    if (rc != MXA_OK) return rc;
    launches++;
    if ((rc = compact(running)) != MXA_OK) return rc;
    if ((rc = launch_ms(h, &total)) != MXA_OK) return rc;
    pops = chunk;  // mxa_set_launch_schedule: the first launch only is first_chunk
  }
  h->last_ms = total;
  if (launches_out) *launches_out = launches;
  return MXA_OK;
}

int mxa_set_launch_schedule(mxa_handle* h, int64_t first_chunk) {
  if (!h || first_chunk < 0) return MXA_EINVAL;
  h->first_chunk = first_chunk;
  return MXA_OK;
}

// book-update log (OrderBook.book_log / the exchange's BEST_BID, BEST_ASK, LAST_TRADE events):
// `cap` records per env in one device buffer; every env's record count restarts at 0
int mxa_set_book_log(mxa_handle* h, int32_t cap) {
  // Kernel.runner handles, the replay's (config/marketreplay.py) included; not GymKernel handles
  if (!h || h->gym || !h->e.run_log || cap < 0) return MXA_EINVAL;
  ENTER(h);
  HIPCHK(h, finish(h));
  h->d_blog.free();
  h->blog_cap = 0;
  if (cap > 0) {
    HIPCHK(h, h->d_blog.alloc((size_t)cap * h->P.n_envs));
    h->blog_cap = cap;
  }
  HIPCHK(h, hipMemset2DAsync(h->d_env + offsetof(EnvHdr, blog_n), h->P.L.env_stride, 0, sizeof(int32_t), h->P.n_envs,
                             h->stream));
  HIPCHK(h, hipMemset2DAsync(h->d_env + offsetof(EnvHdr, blog_fin), h->P.L.env_stride, 0, sizeof(int32_t),
                             h->P.n_envs, h->stream));
  HIPCHK(h, finish(h));
  return MXA_OK;
}

// the exchange's own log (ExchangeAgent.log -> EXCHANGE_AGENT.bz2) in the book-update log: the
// log-variant kernels write its records (mxa_layout.h BL_EV_*) while EnvHdr::exlog is set
int mxa_set_exchange_log(mxa_handle* h, int32_t on) {
  if (!h || h->gym || !h->e.run_log || on < 0 || on > 1) return MXA_EINVAL;
  if (on && !h->d_blog) return MXA_EINVAL;  // it rides in the book-update log: mxa_set_book_log first
  // placements logged before the switch would be missing from the log (its order rows name
  // them), and a log switched off mid-run ends without its tail: set it before the run
  if (h->started && on != h->exlog)
    return refuse(h, "mxa_set_exchange_log", "set it before the first launch (or after a whole-handle mxa_reset)");
  ENTER(h);
  h->exlog = on;
  if (int rc = set_headers(h)) return rc;
  HIPCHK(h, finish(h));
  return MXA_OK;
}

int mxa_read_book_log(mxa_handle* h, int32_t env, mxa_book_rec* out, int64_t cap, int64_t* n) {
  if (!h || env < 0 || env >= h->P.n_envs || !n || cap < 0 || (cap > 0 && !out)) return MXA_EINVAL;
  static_assert(sizeof(mxa_book_rec) == sizeof(BlRec) && offsetof(mxa_book_rec, qty) == offsetof(BlRec, qty),
                "mxa_book_rec mirrors BlRec");
  static_assert((int)MXA_BL_FUNDAMENTAL == (int)BL_FUNDAMENTAL, "f_log record tag");
  static_assert((int)MXA_BL_EV_RX == (int)BL_EV_RX && (int)MXA_BL_EV_NT == (int)BL_EV_NT &&
                    (int)MXA_BL_EV_PLACE == (int)BL_EV_PLACE && (int)MXA_BL_EV_END == (int)BL_EV_END,
                "exchange-log record codes");
  ENTER(h);
  EnvHdr hd;
  HIPCHK(h, env_read(h, env, 0, sizeof hd, &hd));
  HIPCHK(h, finish(h));  // the header sizes the second copy
  // after a kernelStopping pass: its oracle observations follow the run's records
  int64_t cnt = h->d_blog ? (hd.blog_fin > hd.blog_n ? hd.blog_fin : hd.blog_n) : 0;
  *n = cnt;  // beyond the capacity: the log overflowed (the first `blog_cap` records are kept)
  if (cnt > h->blog_cap) cnt = h->blog_cap;
  const int64_t m = cnt < cap ? cnt : cap;
  if (m > 0) HIPCHK(h, dev_read(h, h->d_blog + (size_t)env * h->blog_cap, sizeof(BlRec) * m, out));
  HIPCHK(h, finish(h));
  return MXA_OK;
}

int mxa_finalize(mxa_handle* h) {
  if (!h || h->gym || !h->e.stop) return MXA_EINVAL;
  ENTER(h);
  const size_t rows = (size_t)h->P.n_envs * h->P.n_agents;
  if (!h->d_final) HIPCHK(h, h->d_final.alloc(rows));
  (h->d_blog ? h->e.stop_log : h->e.stop)(dim3(h->P.n_envs), dim3(64), h->lds, h->stream, h->d_env, h->P.L.env_stride,
                                          h->P.n_envs, h->d_final, h->d_blog, h->blog_cap, h->d_ctx);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, finish(h));
  return MXA_OK;
}

int mxa_read_final(mxa_handle* h, int32_t env, mxa_agent_final* out, int32_t cap) {
  if (!h || !h->d_final || env < 0 || env >= h->P.n_envs || !out || cap < h->P.n_agents) return MXA_EINVAL;
  ENTER(h);
  HIPCHK(h, dev_read(h, h->d_final + (size_t)env * h->P.n_agents, sizeof(mxa_agent_final) * h->P.n_agents, out));
  HIPCHK(h, finish(h));
  return h->P.n_agents;
}

int mxa_read_summary(mxa_handle* h, mxa_env_summary* out) {
  if (!h || !out) return MXA_EINVAL;
  ENTER(h);
  int n = h->P.n_envs;
  std::vector<EnvHdr> hd(n);
  HIPCHK(h, env_read_all(h, 0, sizeof(EnvHdr), hd.data()));
  HIPCHK(h, finish(h));
  for (int i = 0; i < n; i++) {
    out[i].status = hd[i].status;
    out[i].err = hd[i].err;
    out[i].events = hd[i].pops;
    out[i].hash = hd[i].hash;
    out[i].current_time = hd[i].cur;
    out[i].order_counter = hd[i].order_counter;
    out[i].last_trade = hd[i].last_trade;
    out[i].max_queue = hd[i].max_q;
    out[i].max_book = hd[i].max_book;
  }
  return MXA_OK;
}

int mxa_read_agents(mxa_handle* h, int32_t env, mxa_agent_state* out, int32_t cap) {
  if (!h || env < 0 || env >= h->P.n_envs) return MXA_ERANGE;
  ENTER(h);
  int n = std::min(cap, h->P.n_agents);
  std::vector<uint32_t> rec((size_t)h->P.n_agents * MXA_AGENT_WORDS);
  std::vector<RpOrder> mo(h->replay ? h->ctx.L.D : 0);  // MarketReplayAgent.orders lives in the dense table
  HIPCHK(h, env_read(h, env, h->P.L.off_ag, rec.size() * 4, rec.data()));
  HIPCHK(h, env_read(h, env, h->ctx.L.off_mro, sizeof(RpOrder) * mo.size(), mo.data()));
  HIPCHK(h, finish(h));
  const int32_t mo_open = (int32_t)std::count_if(mo.begin(), mo.end(), [](const RpOrder& o) { return o.present != 0; });
  for (int a = 0; a < n; a++) {
    const uint32_t* r = &rec[(size_t)a * MXA_AGENT_WORDS];
    auto g64 = [&](int f) { return (int64_t)(((uint64_t)r[f + 1] << 32) | r[f]); };
    out[a].cash = g64(AF_CASH);
    out[a].shares = g64(AF_SHARES);
    out[a].n_open = (int32_t)r[AF_NORD];
    out[a].last_trade = g64(AF_LAST_TRADE);
    out[a].type = (int32_t)r[AF_TYPE];
    out[a].flags = (int32_t)r[AF_FLAGS];
    out[a].starting_cash = g64(AF_START_CASH);
    if (h->replay && out[a].type == AG_REPLAY) out[a].n_open = mo_open;
  }
  return n;
}

int mxa_read_book(mxa_handle* h, int32_t env, int32_t side, int64_t* out4, int32_t cap) {
  if (!h || env < 0 || env >= h->P.n_envs) return MXA_ERANGE;
  ENTER(h);
  if (h->replay) {  // price ladder: levels best-first, FIFO lists
    const RpLayout& L = h->ctx.L;
    std::vector<int32_t> cnt(L.P), head(L.P);
    std::vector<RpEntry> pool(L.C);
    HIPCHK(h, env_read(h, env, L.off_lvc + 4ull * side * L.P, 4ull * L.P, cnt.data()));
    HIPCHK(h, env_read(h, env, L.off_lvh + 4ull * side * L.P, 4ull * L.P, head.data()));
    HIPCHK(h, env_read(h, env, L.off_pool, sizeof(RpEntry) * L.C, pool.data()));
    HIPCHK(h, finish(h));
    int n = 0;
    for (int k = 0; k < L.P; k++) {
      int x = side == 0 ? L.P - 1 - k : k;
      if (!cnt[x]) continue;
      for (int q = head[x]; q >= 0; q = pool[q].next) {
        if (n < cap) {
          out4[4 * n + 0] = pool[q].oid;
          out4[4 * n + 1] = pool[q].meta >> 1;
          out4[4 * n + 2] = pool[q].qty;
          out4[4 * n + 3] = pool[q].price;
        }
        n++;
      }
    }
    return n;
  }
  int oc = h->P.L.ocap;
  std::vector<SavedOrder> so(oc);
  HIPCHK(h, env_read(h, env, h->P.L.off_book, sizeof(SavedOrder) * oc, so.data()));
  HIPCHK(h, finish(h));
  std::vector<SavedOrder> v;
  int buy = side == 0 ? 1 : 0;
  for (auto& o : so)
    if (o.meta >= 0 && (o.meta & 1) == buy) v.push_back(o);
  std::sort(v.begin(), v.end(), [&](const SavedOrder& a, const SavedOrder& b) {
    if (a.price != b.price) return buy ? a.price > b.price : a.price < b.price;
    return a.arrival < b.arrival;
  });
  for (int n = 0; n < (int)v.size() && n < cap; n++) {
    out4[4 * n + 0] = v[n].oid;
    out4[4 * n + 1] = v[n].meta >> 1;
    out4[4 * n + 2] = v[n].qty;
    out4[4 * n + 3] = v[n].price;
  }
  return (int)v.size();  // total on the side; min(total, cap) written
}

int mxa_read_trace(mxa_handle* h, int32_t env, int64_t* out, int64_t cap, int64_t* nout) {
  if (!h || env < 0 || env >= h->P.n_envs) return MXA_ERANGE;
  ENTER(h);
  EnvHdr hd;
  HIPCHK(h, env_read(h, env, 0, sizeof hd, &hd));
  HIPCHK(h, finish(h));  // the header sizes the second copy
  int64_t n = std::min<int64_t>(std::min<int64_t>(hd.trace_len, h->P.L.trace_cap), cap);
  if (n > 0) HIPCHK(h, env_read(h, env, h->P.L.off_trace, (size_t)n * MXA_TRACE_ROW_BYTES, out));
  HIPCHK(h, finish(h));
  if (nout) *nout = n;
  return MXA_OK;
}

int mxa_set_seeds(mxa_handle* h, const uint32_t* seeds) {
  if (!h || !seeds) return MXA_EINVAL;
  ENTER(h);
  HIPCHK(h, hipMemcpyAsync(h->d_seeds, seeds, sizeof(uint32_t) * h->P.n_envs, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, finish(h));
  return MXA_OK;
}

int mxa_write_results(mxa_handle* h, void* device_out) {
  if (!h || !device_out) return MXA_EINVAL;
  ENTER(h);
  int n = h->P.n_envs;
  hipLaunchKernelGGL(mxa_results_kernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->d_env, h->P.L.env_stride,
                     n, (int64_t*)device_out);
  HIPCHK(h, hipGetLastError());
  return MXA_OK;
}

int mxa_write_records(mxa_handle* h, void* device_out) {
  if (!h || !device_out) return MXA_EINVAL;
  ENTER(h);
  int n = h->P.n_envs;
  // GymKernel handles: the execution agent; Kernel.runner handles: every trading agent
  const int a0 = h->gym ? h->P.first_rl : 1, a1 = h->gym ? h->P.first_rl + 1 : h->P.n_agents;
  hipLaunchKernelGGL(mxa_records_kernel, dim3(n), dim3(64), 0, h->stream, h->d_env, h->P.L.env_stride, n, h->d_built,
                     h->P.L.off_ag, a0, a1, (int64_t*)device_out);
  HIPCHK(h, hipGetLastError());
  return MXA_OK;
}

int mxa_read_counters(mxa_handle* h, int64_t* out) {
  if (!h || !out) return MXA_EINVAL;
  ENTER(h);
  const int n = h->P.n_envs;
  const size_t bytes = sizeof(int64_t) * MXA_COUNTER_WORDS * n;
  StreamTmp d;
  HIPCHK(h, d.alloc(bytes, h->stream));
  hipLaunchKernelGGL(mxa_counters_kernel, dim3(n), dim3(64), 0, h->stream, h->d_env, h->P.L.env_stride, n, h->P.L.off_ag,
                     h->P.n_agents, (int64_t*)d.p);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, dev_read(h, d.p, bytes, out));
  HIPCHK(h, finish(h));
  return MXA_OK;
}

int mxa_read_inplace(mxa_handle* h, uint64_t* out) {
  if (!h || !out || !h->e.inplace) return MXA_EINVAL;
  ENTER(h);
  HIPCHK(h, finish(h));
  return h->e.inplace(out) ? MXA_EHIP : MXA_OK;
}

int mxa_set_parity_hash(mxa_handle* h, int32_t enabled) {
  if (!h) return MXA_EINVAL;
  h->parity_hash = enabled != 0;
  return MXA_OK;
}

int mxa_write_rl_state(mxa_handle* h, double* device_out) {
  if (!h || !device_out || !h->gym || h->P.n_rl != 1) return MXA_EINVAL;
  ENTER(h);
  int n = h->P.n_envs;
  hipLaunchKernelGGL(mxa_rl_state_kernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->d_env, h->P.L.env_stride,
                     n, (uint32_t)(h->P.L.off_ag + (uint32_t)MXA_AGENT_BYTES * (uint32_t)h->P.first_rl), h->ctx.L.off_rh,
                     h->ctx.L.off_ring, device_out);
  HIPCHK(h, hipGetLastError());
  return MXA_OK;
}

int mxa_read_raw(mxa_handle* h, int32_t env, int64_t offset, int64_t bytes, void* out) {
  if (!h || env < 0 || env >= h->P.n_envs || offset < 0 || bytes < 0 || offset + bytes > (int64_t)h->P.L.env_stride)
    return MXA_ERANGE;
  ENTER(h);
  HIPCHK(h, env_read(h, env, offset, bytes, out));
  HIPCHK(h, finish(h));
  return MXA_OK;
}

int mxa_layout(const mxa_handle* h, int64_t* o) {
  if (!h || !o) return MXA_EINVAL;
  const Layout& L = h->P.L;
  o[0] = L.off_ag; o[1] = L.off_open; o[2] = L.off_rng; o[3] = L.off_lat;
  o[4] = L.off_q; o[5] = L.off_book; o[6] = L.off_tx; o[7] = L.off_trace;
  return MXA_OK;
}

int32_t mxa_n_agents(const mxa_handle* h) { return h ? h->P.n_agents : 0; }
int32_t mxa_n_envs(const mxa_handle* h) { return h ? h->P.n_envs : 0; }
int64_t mxa_env_bytes(const mxa_handle* h) { return h ? (int64_t)h->P.L.env_stride : 0; }
int mxa_set_stream(mxa_handle* h, void* s) {
  if (!h) return MXA_EINVAL;
  h->stream = s ? (hipStream_t)s : h->own;
  return MXA_OK;
}
double mxa_last_kernel_ms(const mxa_handle* h) { return h ? h->last_ms : 0; }
const char* mxa_last_error(const mxa_handle* h) { return h ? h->err.c_str() : g_cfg_err.c_str(); }

const char* mxa_build_id(void) { return MXA_BUILD_ID; }

void mxa_destroy(mxa_handle* h) {
  if (!h) return;
  hipSetDevice(h->device);
  delete h;  // its device memory, then its events and stream
}

int mxa_rng_probe(int32_t device, uint32_t seed, int32_t mode, double a, double b, int32_t n, double* out) {
  if (n <= 0 || !out || mode < 0 || mode > 5) return MXA_EINVAL;
  if (hipSetDevice(device) != hipSuccess) return MXA_EHIP;
  DevBuf<double> d_out;
  DevBuf<uint32_t> d_s;
  if (d_out.alloc(n) != hipSuccess || d_s.alloc(MXA_RNG_WORDS) != hipSuccess) return MXA_ENOMEM;
  hipLaunchKernelGGL(mxa_rng_probe_kernel, dim3(1), dim3(64), 0, 0, seed, mode, a, b, n, d_out.p, d_s.p);
  if (hipGetLastError() != hipSuccess) return MXA_EHIP;
  return hipMemcpy(out, d_out, sizeof(double) * n, hipMemcpyDeviceToHost) == hipSuccess ? MXA_OK : MXA_EHIP;
}

// include/mxa_variates.h
int mxa_variate_probe(int32_t device, uint32_t seed, const uint8_t* script, int32_t n, int32_t lookahead, double* out,
                      uint64_t* state) {
  if (n <= 0 || !script || !out || !state || lookahead < 2 || lookahead > 256) return MXA_EINVAL;
  for (int32_t i = 0; i < n; i++)
    if (script[i] > 3) return MXA_EINVAL;
  if (hipSetDevice(device) != hipSuccess) return MXA_EHIP;
  DevBuf<uint8_t> d_script;
  DevBuf<double> d_out;
  DevBuf<uint64_t> d_state, d_tab;
  DevBuf<uint32_t> d_s;
  if (d_script.alloc(n) != hipSuccess || d_out.alloc(2 * (size_t)n) != hipSuccess || d_state.alloc(6 * (size_t)n) != hipSuccess ||
      d_tab.alloc(MXA_VT_BYTES / 8) != hipSuccess || d_s.alloc(2 * MXA_RNG_WORDS) != hipSuccess)
    return MXA_ENOMEM;
  if (hipMemcpy(d_script, script, (size_t)n, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(d_tab, 0, MXA_VT_BYTES) != hipSuccess)
    return MXA_EHIP;
  hipLaunchKernelGGL(mxa_variate_probe_kernel, dim3(1), dim3(64), 0, 0, seed, d_script.p, n, lookahead, d_out.p, d_state.p,
                     d_s.p, d_tab.p);
  if (hipGetLastError() != hipSuccess) return MXA_EHIP;
  if (hipMemcpy(out, d_out, sizeof(double) * 2 * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess) return MXA_EHIP;
  return hipMemcpy(state, d_state, sizeof(uint64_t) * 6 * (size_t)n, hipMemcpyDeviceToHost) == hipSuccess ? MXA_OK : MXA_EHIP;
}

// include/mxa_streams.h
int mxa_stream_head_probe(int32_t device, uint32_t seed, int32_t head_words, int32_t n, double* out_values,
                          uint64_t* out_state) {
  if (n <= 0 || !out_values || !out_state || head_words < 2 || head_words > MXA_STREAM_HEAD_WORDS) return MXA_EINVAL;
  if (hipSetDevice(device) != hipSuccess) return MXA_EHIP;
  DevBuf<double> d_out;
  DevBuf<uint64_t> d_state;
  DevBuf<uint32_t> d_s;
  if (d_out.alloc((size_t)n) != hipSuccess || d_state.alloc(2 * (size_t)n) != hipSuccess || d_s.alloc(MXA_RNG_WORDS) != hipSuccess)
    return MXA_ENOMEM;
  if (hipMemset(d_s, 0, sizeof(uint32_t) * MXA_RNG_WORDS) != hipSuccess) return MXA_EHIP;
  hipLaunchKernelGGL(mxa_stream_head_probe_kernel, dim3(1), dim3(64), 0, 0, seed, head_words, n, d_out.p, d_state.p, d_s.p);
  if (hipGetLastError() != hipSuccess) return MXA_EHIP;
  if (hipMemcpy(out_values, d_out, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess) return MXA_EHIP;
  return hipMemcpy(out_state, d_state, sizeof(uint64_t) * 2 * (size_t)n, hipMemcpyDeviceToHost) == hipSuccess ? MXA_OK : MXA_EHIP;
}

int mxa_math_probe(int32_t device, int32_t mode, const double* x, const double* y, double* out, int64_t n) {
  if (n <= 0 || !x || !out) return MXA_EINVAL;
  if (hipSetDevice(device) != hipSuccess) return MXA_EHIP;
  DevBuf<double> dx, dy, dout;
  size_t bytes = sizeof(double) * n;
  if (dx.alloc(n) != hipSuccess || dy.alloc(n) != hipSuccess || dout.alloc(n) != hipSuccess) return MXA_ENOMEM;
  if (hipMemcpy(dx, x, bytes, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(dy, y ? y : x, bytes, hipMemcpyHostToDevice) != hipSuccess)
    return MXA_EHIP;
  hipLaunchKernelGGL(mxa_math_probe_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, mode, dx.p, dy.p, dout.p,
                     n);
  if (hipGetLastError() != hipSuccess) return MXA_EHIP;
  return hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost) == hipSuccess ? MXA_OK : MXA_EHIP;
}

int mxa_policy_probe(void* stream, int32_t n, const float* x, const float* params, int32_t n_layers, const int32_t* dims,
                     int32_t test, int32_t enough, const double* u, const int64_t* rnd, const double* eps, float* q,
                     int64_t* a) {
  if (n <= 0 || !x || !params || !qwave::dims_ok(n_layers, dims) || (!q && !a)) return MXA_EINVAL;
  if (a && !test && (!u || !rnd || !eps)) return MXA_EINVAL;
  MxaPolicyProbe p{};
  p.params = params;
  p.n_layers = n_layers;
  for (int i = 0; i <= n_layers; i++) p.dims[i] = dims[i];
  p.test = test;
  p.enough = enough;
  p.u = u;
  p.rnd = rnd;
  p.eps = eps;
  hipLaunchKernelGGL(mxa_policy_probe_kernel, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, p, n, x, q, a);
  return hipGetLastError() == hipSuccess ? MXA_OK : MXA_EHIP;
}

// ---- env-state snapshots (include/mxa_snap.h; mxa_snapshot.h: slot layout, checks, kernel)
}  // extern "C"

struct mxa_snapshot {
  const mxa_handle* owner = nullptr;  // compared only: a bank shared between handles is out of scope
  int device = 0;
  int32_t n_slots = 0, n_envs = 0;
  // the owner's values at create: a handle that differs in one of them has other blocks or another log
  uint64_t env_stride = 0;
  int32_t blog_cap = 0, exlog = 0;
  int64_t slot_bytes = 0;
  int loads = 4;  // 16-byte loads a lane has in flight (MXA_SNAPSHOT_LOADS=8: the other instantiation)
  std::vector<uint8_t> filled;
  DevBuf<char> d_slots;
  DevBuf<int32_t> d_map;
};

// everything a save / restore refuses, before any HIP call; the message goes to mxa_last_error
static int snapshot_check(mxa_handle* h, const mxa_snapshot* s, const int32_t* map, bool save) {
  if (!h || !s) return refuse(h, "mxa_snapshot", "null argument");
  const char* why = nullptr;
  if (s->owner != h) why = "the snapshot was created by another handle";
  else if (s->env_stride != h->P.L.env_stride) why = "the handle's env_stride is not the snapshot's";
  else if (s->blog_cap != h->blog_cap) why = "the book-update log was reallocated (mxa_set_book_log) after mxa_snapshot_create";
  else if (s->exlog != h->exlog) why = "the exchange-log switch is not the one at mxa_snapshot_create";
  else why = mxa_snap::check_map(map, h->P.n_envs, s->n_slots, save, s->filled.data());
  return why ? refuse(h, save ? "mxa_snapshot_save" : "mxa_snapshot_restore", why) : MXA_OK;
}

// the map to the device (as mxa_reset uploads its mask), then the one launch
static int snapshot_copy(mxa_handle* h, const mxa_snapshot* s, const int32_t* map, int restore) {
  const int n = h->P.n_envs;
  std::vector<int32_t> m(n);
  for (int i = 0; i < n; i++) m[i] = map ? map[i] : i;
  HIPCHK(h, hipMemcpyAsync(s->d_map, m.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, finish(h));  // m is a host temporary
  const uint32_t nb_block = (uint32_t)mxa_snap::wg_count((int64_t)s->env_stride, s->loads);
  const uint32_t nb_log = (uint32_t)mxa_snap::wg_count((int64_t)s->blog_cap * mxa_snap::LOG_REC_BYTES, s->loads);
  const dim3 grid(nb_block + nb_log, (unsigned)std::min(n, 65535));
  auto k = s->loads == 8 ? mxa_snapshot_kernel<8> : mxa_snapshot_kernel<4>;
  return timed_launch(h, [&] {
    hipLaunchKernelGGL(k, grid, dim3(mxa_snap::WG_LANES), 0, h->stream, (char*)h->d_env, s->env_stride,
                       (char*)s->d_slots, (uint64_t)s->slot_bytes, (const int32_t*)s->d_map, n, (uint32_t*)h->d_built,
                       (char*)h->d_blog.p, s->blog_cap, nb_block, restore);
  });
}

extern "C" {

int mxa_snapshot_create(mxa_handle* h, int32_t n_slots, mxa_snapshot** out) {
  if (!h || !out || n_slots <= 0 || !mxa_snap::stride_ok((int64_t)h->P.L.env_stride))
    return refuse(h, "mxa_snapshot_create", "null argument or n_slots <= 0");
  *out = nullptr;
  ENTER(h);
  auto s = std::make_unique<mxa_snapshot>();
  s->owner = h;
  s->device = h->device;
  s->n_slots = n_slots;
  s->n_envs = h->P.n_envs;
  s->env_stride = h->P.L.env_stride;
  s->blog_cap = h->d_blog ? h->blog_cap : 0;
  s->exlog = h->exlog;
  s->slot_bytes = mxa_snap::slot_bytes((int64_t)s->env_stride, s->blog_cap);
  if (const char* l = getenv("MXA_SNAPSHOT_LOADS")) s->loads = atoi(l) == 8 ? 8 : 4;
  s->filled.assign(n_slots, 0);
  hipError_t e = s->d_slots.alloc((size_t)s->slot_bytes * n_slots);
  if (e == hipSuccess) e = s->d_map.alloc(s->n_envs);
  if (e != hipSuccess) {
    (void)hipGetLastError();  // the failed allocation is this call's error, not the next launch's
    return hip_fail(h, e, "mxa_snapshot_create: hipMalloc");
  }
  *out = s.release();
  return MXA_OK;
}

int mxa_snapshot_save(mxa_handle* h, mxa_snapshot* s, const int32_t* slot_of_env) {
  if (int rc = snapshot_check(h, s, slot_of_env, true)) return rc;
  ENTER(h);
  if (int rc = snapshot_copy(h, s, slot_of_env, 0)) return rc;
  HIPCHK(h, finish(h));
  if (int rc = launch_ms(h)) return rc;
  for (int i = 0; i < h->P.n_envs; i++) {
    const int32_t k = slot_of_env ? slot_of_env[i] : i;
    if (k >= 0) s->filled[k] = 1;
  }
  return MXA_OK;
}

int mxa_snapshot_restore(mxa_handle* h, const mxa_snapshot* s, const int32_t* slot_of_env) {
  if (int rc = snapshot_check(h, s, slot_of_env, false)) return rc;
  ENTER(h);
  if (int rc = snapshot_copy(h, s, slot_of_env, 1)) return rc;
  h->started = true;  // the restored envs have popped events: the exchange log is fixed
  // the handle's current stop time (and its exchange-log switch) hold for the restored envs
  if (int rc = set_headers(h)) return rc;
  HIPCHK(h, finish(h));
  return launch_ms(h);
}

int mxa_snapshot_info(const mxa_snapshot* s, int64_t* out4) {
  if (!s || !out4) return MXA_EINVAL;
  out4[0] = s->n_slots;
  out4[1] = s->slot_bytes;
  out4[2] = std::count(s->filled.begin(), s->filled.end(), (uint8_t)1);
  out4[3] = s->blog_cap > 0 ? 1 : 0;
  return MXA_OK;
}

void mxa_snapshot_destroy(mxa_snapshot* s) {
  if (!s) return;
  hipSetDevice(s->device);
  delete s;
}

}  // extern "C"

// ---- book depth (include/mxa_depth.h; mxa_depth_kernels.h: the checks, the sizes and the two kernels)

// everything a depth call refuses, before any HIP call; the message goes to mxa_last_error
static int depth_check(mxa_handle* h, const char* what, int32_t levels, const void* depth) {
  const char* why = mxa_depth::check_args(h != nullptr, depth != nullptr, levels);
  if (!why && !h->replay && !mxa_depth::ocap_ok(h->P.L.ocap)) why = "the book has more slots than the kernel's LDS holds";
  return why ? refuse(h, what, why) : MXA_OK;
}

// the one launch on the handle's stream: the ladder kernel for the replay book, else the slot kernel
static int depth_launch(mxa_handle* h, int32_t levels, int64_t* d_depth, int32_t* d_counts) {
  const int n = h->P.n_envs;
  const unsigned gy = (unsigned)mxa_depth::grid_y(n);
  if (h->replay) {
    const RpLayout& L = h->ctx.L;
    hipLaunchKernelGGL(mxa_depth_ladder_kernel, dim3(2, gy), dim3(mxa_depth::WAVE), 0, h->stream, (const char*)h->d_env,
                       h->P.L.env_stride, L.off_rh, L.off_lvc, L.off_lvq, L.pmin, L.P, n, levels, (mxa_depth::Row*)d_depth,
                       d_counts);
  } else {
    hipLaunchKernelGGL(mxa_depth_slots_kernel, dim3(1, gy), dim3(mxa_depth::WAVE), 0, h->stream, (const char*)h->d_env,
                       h->P.L.env_stride, h->P.L.off_book, h->P.L.ocap, n, levels, (mxa_depth::Row*)d_depth, d_counts);
  }
  HIPCHK(h, hipGetLastError());
  return MXA_OK;
}

extern "C" {

int mxa_write_depth(mxa_handle* h, int32_t levels, int64_t* d_depth, int32_t* d_counts) {
  if (int rc = depth_check(h, "mxa_write_depth", levels, d_depth)) return rc;
  ENTER(h);
  return depth_launch(h, levels, d_depth, d_counts);
}

int mxa_read_depth(mxa_handle* h, int32_t levels, int64_t* depth, int32_t* counts) {
  if (int rc = depth_check(h, "mxa_read_depth", levels, depth)) return rc;
  ENTER(h);
  // one stream-ordered temporary: the rows, then the counts (the rows are a multiple of 16 bytes)
  const size_t nb = (size_t)mxa_depth::depth_bytes(h->P.n_envs, levels), nc = (size_t)mxa_depth::counts_bytes(h->P.n_envs);
  StreamTmp d;
  HIPCHK(h, d.alloc(nb + nc, h->stream));
  if (int rc = depth_launch(h, levels, (int64_t*)d.p, (int32_t*)(d.p + nb))) return rc;
  HIPCHK(h, dev_read(h, d.p, nb, depth));
  if (counts) HIPCHK(h, dev_read(h, d.p + nb, nc, counts));
  HIPCHK(h, finish(h));
  return MXA_OK;
}

}  // extern "C"

// ---- time bars from the book-update log (include/mxa_bars.h; mxa_bars_kernels.h: the checks, the sizes
// and the replay kernel)

// everything a bars call on a handle refuses, before any HIP call
static int bars_check(mxa_handle* h, const char* what, int64_t t0, int64_t dt, int32_t n_bars, const void* bars) {
  const char* why = mxa_bars::check_handle(h != nullptr, h && h->gym, h && h->d_blog && h->blog_cap > 0);
  if (!why) why = mxa_bars::check_grid(t0, dt, n_bars, bars != nullptr, ((uintptr_t)bars & 15) == 0);
  return why ? refuse(h, what, why) : MXA_OK;
}

static hipError_t bars_launch(hipStream_t stream, const char* rec, int64_t rec_stride, int64_t rec_cap, const char* cnt0,
                              const char* cnt1, int64_t cnt_stride, int n_envs, int32_t level_cap, int64_t t0, int64_t dt,
                              int32_t n_bars, int64_t* d_bars, int32_t* d_status) {
  hipLaunchKernelGGL(mxa_bars_kernel, dim3(1, (unsigned)mxa_bars::grid_y(n_envs)), dim3(mxa_bars::WAVE),
                     (size_t)mxa_bars::lds_bytes(level_cap), stream, rec, rec_stride, rec_cap, cnt0, cnt1, cnt_stride, n_envs,
                     level_cap, t0, dt, n_bars, d_bars, d_status);
  return hipGetLastError();
}

// the one launch on the handle's stream: the records of d_blog, the counts from the env headers
static int bars_launch_handle(mxa_handle* h, int64_t t0, int64_t dt, int32_t n_bars, int64_t* d_bars, int32_t* d_status) {
  HIPCHK(h, bars_launch(h->stream, (const char*)(BlRec*)h->d_blog, (int64_t)h->blog_cap * (int64_t)sizeof(BlRec), h->blog_cap,
                        h->d_env + offsetof(EnvHdr, blog_n), h->d_env + offsetof(EnvHdr, blog_fin),
                        (int64_t)h->P.L.env_stride, h->P.n_envs, mxa_bars::handle_level_cap(h->replay, h->P.L.ocap), t0, dt,
                        n_bars, d_bars, d_status));
  return MXA_OK;
}

extern "C" {

int mxa_write_bars(mxa_handle* h, int64_t t0_ns, int64_t dt_ns, int32_t n_bars, int64_t* d_bars, int32_t* d_status) {
  if (int rc = bars_check(h, "mxa_write_bars", t0_ns, dt_ns, n_bars, d_bars)) return rc;
  ENTER(h);
  return bars_launch_handle(h, t0_ns, dt_ns, n_bars, d_bars, d_status);
}

int mxa_read_bars(mxa_handle* h, int64_t t0_ns, int64_t dt_ns, int32_t n_bars, int64_t* bars, int32_t* status) {
  if (int rc = bars_check(h, "mxa_read_bars", t0_ns, dt_ns, n_bars, bars)) return rc;
  ENTER(h);
  // one stream-ordered temporary: the bars, then the status words (the bars are a multiple of 16 bytes)
  const size_t nb = (size_t)mxa_bars::bars_bytes(h->P.n_envs, n_bars), ns = (size_t)mxa_bars::status_bytes(h->P.n_envs);
  StreamTmp d;
  HIPCHK(h, d.alloc(nb + ns, h->stream));
  if (int rc = bars_launch_handle(h, t0_ns, dt_ns, n_bars, (int64_t*)d.p, (int32_t*)(d.p + nb))) return rc;
  HIPCHK(h, dev_read(h, d.p, nb, bars));
  if (status) HIPCHK(h, dev_read(h, d.p + nb, ns, status));
  HIPCHK(h, finish(h));
  return MXA_OK;
}

int mxa_bars_from_records(void* stream, int32_t n_envs, const mxa_book_rec* d_rec, int64_t rec_stride, const int32_t* d_count,
                          int32_t level_cap, int64_t t0_ns, int64_t dt_ns, int32_t n_bars, int64_t* d_bars, int32_t* d_status) {
  const char* what = "mxa_bars_from_records";
  const char* why = mxa_bars::check_records(n_envs, d_rec != nullptr, rec_stride, d_count != nullptr, level_cap);
  if (!why && ((uintptr_t)d_rec & 15)) why = "records not 16-byte aligned";
  if (!why) why = mxa_bars::check_grid(t0_ns, dt_ns, n_bars, d_bars != nullptr, ((uintptr_t)d_bars & 15) == 0);
  if (!why && rec_stride > INT64_MAX / (int64_t)sizeof(BlRec)) why = "rec_stride beyond int64 bytes";
  if (why) return refuse(nullptr, what, why);
  const hipError_t e = bars_launch((hipStream_t)stream, (const char*)d_rec, rec_stride * (int64_t)sizeof(BlRec), rec_stride,
                                   (const char*)d_count, (const char*)d_count, sizeof(int32_t), n_envs, level_cap, t0_ns, dt_ns,
                                   n_bars, d_bars, d_status);
  if (e != hipSuccess) return hip_fail(nullptr, e, what);
  return MXA_OK;
}

}  // extern "C"
