// mxa_entry.h — the kernels of one configuration as seen by the C-ABI (mxa_api.hip).
//
// Each configuration's engine is compiled in a translation unit of its own (mxa_inst.hip built
// with -DMXA_INST_CFG=<id>), so the eight engine instantiations build in parallel; the C-ABI
// picks a configuration's launchers through mxa_entry_<id>().
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/mxa.h"
#include "mxa_layout.h"

typedef void (*mxa_build_fn)(dim3, dim3, size_t, hipStream_t, char*, uint64_t, int, const uint32_t*, const uint8_t*,
                             const RpCtx*);
typedef void (*mxa_run_fn)(dim3, dim3, size_t, hipStream_t, char*, uint64_t, int, int, int64_t, const RpCtx*, BlRec*,
                           int, const int32_t*);
typedef void (*mxa_stop_fn)(dim3, dim3, size_t, hipStream_t, char*, uint64_t, int, mxa_agent_final*, BlRec*, int,
                            const RpCtx*);
typedef void (*mxa_step_fn)(dim3, dim3, size_t, hipStream_t, char*, uint64_t, int, int, int64_t, const RpCtx*,
                            const double*, double*, int32_t*);

typedef void (*mxa_step_many_fn)(dim3, dim3, size_t, hipStream_t, char*, uint64_t, int, int, int64_t, const RpCtx*,
                                 const double*, double*, int32_t*, int);

// the closed-loop flavour (mxa_step_policy): the policy POD by value, then obs, flags, action
// indices, action vectors, rl-state rows (nullable), k, first_zero
typedef void (*mxa_step_policy_fn)(dim3, dim3, size_t, hipStream_t, char*, uint64_t, int, int, int64_t, const RpCtx*,
                                   const mxa_policy&, double*, int32_t*, int64_t*, double*, double*, int, int);

// the same with the state of a spec (mxa_step_policy_spec): the spec by value after the policy
typedef void (*mxa_step_policy_spec_fn)(dim3, dim3, size_t, hipStream_t, char*, uint64_t, int, int, int64_t, const RpCtx*,
                                        const mxa_policy&, const mxa_state_spec&, double*, int32_t*, int64_t*, double*,
                                        double*, int, int);

typedef int (*mxa_inplace_fn)(uint64_t*);  // read and clear the configuration's in-place group counts (mxa_read_inplace)
typedef int (*mxa_occ_fn)(size_t);  // resident blocks (envs) per CU of the measured kernel at that LDS size

struct MxaEntry {
  mxa_build_fn build;
  mxa_run_fn run, run_log;     // run_log: the book-update-log variant (plain Kernel.runner configs)
  mxa_run_fn run_fast;         // without the parity instrumentation (hash off, no trace ring)
  mxa_stop_fn stop, stop_log;
  mxa_step_fn step, step_fast; // GymKernel configurations (step_fast: without the instrumentation)
  mxa_step_many_fn step_many, step_many_fast;  // k steps per launch, actions given up front
  mxa_step_policy_fn step_policy, step_policy_fast;  // k periods per launch, the Q-network policy in place
  mxa_step_policy_spec_fn step_policy_spec, step_policy_spec_fast;  // the same, the state from a spec
  mxa_inplace_fn inplace;      // g_mxa_inplace of the configuration's translation unit
  mxa_occ_fn occ;              // hipOccupancyMaxActiveBlocksPerMultiprocessor of run_fast / step_fast
};

// the built-in configurations (mxa_layout.h mxa_config_id): the one list behind the declarations
// below, MXA_N_CONFIGS and the C-ABI's switch.  A new configuration is one more X(<id>) here
#define MXA_CONFIGS(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16) X(17)

#define MXA_ENTRY_CAT2(a, b) a##b
#define MXA_ENTRY_CAT(a, b) MXA_ENTRY_CAT2(a, b)
#define MXA_ENTRY_FN(id) MXA_ENTRY_CAT(mxa_entry_, id)  // mxa_entry_<id>; id may be a macro
#define MXA_ENTRY_DECL(id) MxaEntry MXA_ENTRY_FN(id)();
MXA_CONFIGS(MXA_ENTRY_DECL)
#define MXA_ENTRY_COUNT(id) +1
#define MXA_N_CONFIGS (0 MXA_CONFIGS(MXA_ENTRY_COUNT))
