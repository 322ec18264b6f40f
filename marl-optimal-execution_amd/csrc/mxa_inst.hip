// mxa_inst.hip — one configuration's kernels: compiled once per configuration with
// -DMXA_INST_CFG=<id> (mxa_layout.h mxa_config_id), exporting mxa_entry_<id>().
#include "mxa_kernels.hip"
#include "mxa_entry.h"

#ifndef MXA_INST_CFG
#error "mxa_inst.hip is compiled per configuration: -DMXA_INST_CFG=<id>"
#endif

namespace {

template <int CFG>
void launch_build(dim3 g, dim3 b, size_t lds, hipStream_t s, char* base, uint64_t stride, int n, const uint32_t* seeds,
                  const uint8_t* mask, const RpCtx* ctx) {
  hipLaunchKernelGGL((mxa_build_kernel<CFG>), g, b, lds, s, base, stride, n, seeds, mask, ctx);
}
template <int CFG, bool LOG, bool INSTR>
void launch_run(dim3 g, dim3 b, size_t lds, hipStream_t s, char* base, uint64_t stride, int n, int tcap, int64_t max_pops,
                const RpCtx* ctx, BlRec* blog, int blog_cap, const int32_t* list) {
  hipLaunchKernelGGL((mxa_run_kernel<CFG, LOG, INSTR>), g, b, lds, s, base, stride, n, tcap, max_pops, ctx, blog,
                     blog_cap, list);
}
template <int CFG, bool LOG>
void launch_stop(dim3 g, dim3 b, size_t lds, hipStream_t s, char* base, uint64_t stride, int n, mxa_agent_final* out,
                 BlRec* blog, int blog_cap, const RpCtx* ctx) {
  hipLaunchKernelGGL((mxa_stop_kernel<CFG, LOG>), g, b, lds, s, base, stride, n, out, blog, blog_cap, ctx);
}
#ifndef MXA_NO_GYM
template <int CFG, bool INSTR>
void launch_step(dim3 g, dim3 b, size_t lds, hipStream_t s, char* base, uint64_t stride, int n, int tcap, int64_t max_pops,
                 const RpCtx* ctx, const double* act, double* obs, int32_t* flags) {
  hipLaunchKernelGGL((mxa_step_kernel<CFG, INSTR, false>), g, b, lds, s, base, stride, n, tcap, max_pops, ctx, act, obs,
                     flags, 1);
}
template <int CFG, bool INSTR>
void launch_step_many(dim3 g, dim3 b, size_t lds, hipStream_t s, char* base, uint64_t stride, int n, int tcap,
                      int64_t max_pops, const RpCtx* ctx, const double* act, double* obs, int32_t* flags, int k) {
  hipLaunchKernelGGL((mxa_step_kernel<CFG, INSTR, true>), g, b, lds, s, base, stride, n, tcap, max_pops, ctx, act, obs,
                     flags, k);
}
template <int CFG, bool INSTR>
void launch_step_policy(dim3 g, dim3 b, size_t lds, hipStream_t s, char* base, uint64_t stride, int n, int tcap,
                        int64_t max_pops, const RpCtx* ctx, const mxa_policy& p, double* obs, int32_t* flags, int64_t* a,
                        double* act, double* state, int k, int first_zero) {
  MxaStepPolicy pol{p, first_zero, a, act, state};
  hipLaunchKernelGGL((mxa_step_policy_kernel<CFG, INSTR>), g, b, lds, s, base, stride, n, tcap, max_pops, ctx, pol, obs,
                     flags, k);
}
template <int CFG, bool INSTR>
void launch_step_policy_spec(dim3 g, dim3 b, size_t lds, hipStream_t s, char* base, uint64_t stride, int n, int tcap,
                             int64_t max_pops, const RpCtx* ctx, const mxa_policy& p, const mxa_state_spec& spec,
                             double* obs, int32_t* flags, int64_t* a, double* act, double* state, int k,
                             int first_zero) {
  MxaStepPolicySpec ps{{p, first_zero, a, act, state}, spec};
  hipLaunchKernelGGL((mxa_step_policy_spec_kernel<CFG, INSTR>), g, b, lds, s, base, stride, n, tcap, max_pops, ctx, ps,
                     obs, flags, k);
}
#endif

template <int CFG, bool GYM>
int occupancy(size_t lds) {
  int n = 0;
  hipError_t e;
#ifndef MXA_NO_GYM
  if constexpr (GYM) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, mxa_step_kernel<CFG, false, false>, 64, lds);
  else
#endif
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, mxa_run_kernel<CFG, false, false>, 64, lds);
  return e == hipSuccess ? n : -1;
}

// in-place group counts of this translation unit's instrumented kernels, then cleared; 0: ok
int inplace_read(uint64_t* out) {
  static const uint64_t z[MXA_INPLACE_WORDS] = {0};
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(mxa::g_mxa_inplace), sizeof z) != hipSuccess) return 1;
  return hipMemcpyToSymbol(HIP_SYMBOL(mxa::g_mxa_inplace), z, sizeof z) != hipSuccess;
}

template <int CFG>
MxaEntry make_entry() {
  MxaEntry e{};
  e.build = launch_build<CFG>;
  e.inplace = inplace_read;
  e.run = launch_run<CFG, false, true>;
  e.stop = launch_stop<CFG, false>;
  constexpr bool gym = CFG == MXA_CFG_MARKETREPLAY || CFG == MXA_CFG_RMSC03_RL;
#ifndef MXA_NO_GYM
  e.occ = occupancy<CFG, gym>;
#else
  if constexpr (!gym) e.occ = occupancy<CFG, false>;
#endif
  if constexpr (!gym) {  // the book-update log: plain Kernel.runner configurations
    e.run_log = launch_run<CFG, true, true>;
    // measured per configuration (one box, hash off, run kernel): without the instrumentation
    // rmsc03 44.1 vs 44.6 ms, sparse_zi_100 132.5 vs 135.1, value_noise 22.1 vs 22.5, rmsc02
    // 1190 vs 1245; rmsc01 and sparse_zi_1000 measured the other way in round 2 (1201 vs 1147,
    // 986 vs 976), but with the event-class counters in the instrumented kernel (round 3, s10)
    // the plain one wins there too: rmsc01 1047 vs 1082 ms, sparse_zi_1000 916 vs 920
    e.run_fast = launch_run<CFG, false, false>;
    e.stop_log = launch_stop<CFG, true>;
  }
#ifndef MXA_NO_GYM
  if constexpr (gym) {
    e.step = launch_step<CFG, true>;
    e.step_fast = launch_step<CFG, false>;
    e.step_many = launch_step_many<CFG, true>;
    e.step_many_fast = launch_step_many<CFG, false>;
    e.step_policy = launch_step_policy<CFG, true>;
    e.step_policy_fast = launch_step_policy<CFG, false>;
    e.step_policy_spec = launch_step_policy_spec<CFG, true>;
    e.step_policy_spec_fast = launch_step_policy_spec<CFG, false>;
  }
#endif
  return e;
}

}  // namespace

#ifdef MXA_CUSTOM_HDR
// a runtime composition's specialisation (mxa_config_compile): a library of its own, loaded by
// mxa_create_config.  Everything but this entry point is hidden (-fvisibility=hidden), so its
// kernels and launchers never interpose on libmxa's instantiation of the same base
#ifndef MXA_BUILD_ID
#error "a specialisation carries the build id of the libmxa that compiled it"
#endif
extern "C" __attribute__((visibility("default"))) int mxa_custom_entry(MxaEntry* e, MxaParams* P, size_t* lds,
                                                                      mxa_config* cfg, const char** build_id) {
  *e = make_entry<MXA_INST_CFG>();
  *P = mxa_cfg::params(MXA_INST_CFG);
  *lds = mxa_cfg::lds_bytes(MXA_INST_CFG);
  *cfg = mxa_cfg::custom_cfg();
  *build_id = MXA_BUILD_ID;
  return (int)sizeof(MxaParams);
}
#else
MxaEntry MXA_ENTRY_FN(MXA_INST_CFG)() { return make_entry<MXA_INST_CFG>(); }
#endif
