"""ctypes binding of libmxa (include/mxa.h).

The product path is the HIP library only: if lib/libmxa.so is missing or cannot be
loaded this module raises — there is deliberately no CPU fallback.
"""
import ctypes
import os

PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("MXA_LIB") or os.path.join(PKG_ROOT, "lib", "libmxa.so")

MXA_RMSC03, MXA_SPARSE_ZI_100, MXA_SPARSE_ZI_1000, MXA_MARKETREPLAY, MXA_RMSC03_RL, MXA_VALUE_NOISE = 0, 1, 2, 3, 4, 5
MXA_RMSC01 = 6
MXA_RMSC02 = 7
MXA_OBI_RMSC02 = 8
MXA_RANDOM_FUND_VALUE = 9
MXA_RANDOM_FUND_DIVERSE = 10
MXA_HIST_FUND_VALUE = 11
MXA_HIST_FUND_DIVERSE = 12
MXA_MARKETREPLAY_RUNNER = 13
MXA_MARKETREPLAY_TWAP = 14
MXA_RMSC03_SBMM = 15
MXA_RMSC03_SBMM_POLL = 16
MXA_RMSC03_MM = 17  # config/rmsc03.py with per-env --mm-* options (mxa_create_params)
CONFIG_IDS = {"rmsc03": MXA_RMSC03, "sparse_zi_100": MXA_SPARSE_ZI_100, "sparse_zi_1000": MXA_SPARSE_ZI_1000,
              "value_noise": MXA_VALUE_NOISE, "rmsc01": MXA_RMSC01, "rmsc02": MXA_RMSC02,
              "obi_rmsc02": MXA_OBI_RMSC02, "random_fund_value": MXA_RANDOM_FUND_VALUE,
              "random_fund_diverse": MXA_RANDOM_FUND_DIVERSE, "hist_fund_value": MXA_HIST_FUND_VALUE,
              "hist_fund_diverse": MXA_HIST_FUND_DIVERSE,
              # config/marketreplay.py (Kernel.runner; ABIDESEnv's GymKernel replay is mxabides.gym)
              "marketreplay_runner": MXA_MARKETREPLAY_RUNNER,
              # config/execution/marketreplay/execution_marketreplay.py (TWAP agent passive / -e)
              "marketreplay_twap": MXA_MARKETREPLAY_TWAP, "marketreplay_twap_e": MXA_MARKETREPLAY_TWAP,
              # rmsc03 with a SpreadBasedMarketMakerAgent in the market maker's slot (subscribe / polling)
              "rmsc03_sbmm": MXA_RMSC03_SBMM, "rmsc03_sbmm_poll": MXA_RMSC03_SBMM_POLL}
ENV_RUNNING, ENV_DONE, ENV_ERROR = 0, 1, 2
ERR_NAMES = {0: "none", 1: "event queue capacity", 2: "order book capacity", 3: "open-order list capacity",
             4: "transaction history capacity", 5: "get_transacted_volume without transactions (pandas error)",
             6: "setWakeup in the past", 7: "ZI theta index (IndexError)", 8: "bad config",
             9: "RNG look-ahead overrun", 10: "price outside the replay ladder", 11: "book entry pool capacity",
             12: "agent order-id capacity", 13: "MarketReplayAgent KeyError (no tape group at wake time)",
             14: "get_observation/get_reward on missing or None data", 15: "kernelStopping with trade on (TypeError)",
             16: "modify changing price or side",
             17: "HBL order stream outside the history window / device ring (MXA_OH_CAP)",
             18: "HBL streamed price range beyond the device histogram (MXA_HBL_RANGE)",
             19: "limit price the reference would carry as a python float (not restated)",
             20: "book-update log full (raise the book_log capacity)",
             21: "market data published before the book's first change (the reference's TypeError)",
             22: "more market-data subscriptions than the device table",
             23: "cancelled a market-data subscription that does not exist (KeyError)",
             24: "two MARKET_DATA messages in flight to one agent (subscription freq below the latency)",
             25: "ExecutionAgent.placeOrders: schedule[Interval(t, t + 30 s)] of a 60 s TWAP schedule (KeyError)",
             26: "ExecutionAgent.placeOrders: (bid + ask) / 2 with a None side (TypeError)",
             27: "ExecutionAgent.placeOrders: placeMarketOrder at horizon[-2] (not restated)",
             28: "SpreadBasedMarketMakerAgent: mid unbound (UnboundLocalError)",
             29: "order quantity beyond the device's 32-bit order words (POVMarketMakerAgent pov x volume)",
             30: "replay QUERY_SPREAD: a best level's total quantity beyond the reply's signed 32-bit word",
             31: "market-maker ladder price beyond the 32-bit order words (mid + --mm-window-size + --mm-num-ticks)"}


class EnvSummary(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int32), ("err", ctypes.c_int32), ("events", ctypes.c_int64),
                ("hash", ctypes.c_uint64), ("current_time", ctypes.c_int64), ("order_counter", ctypes.c_int64),
                ("last_trade", ctypes.c_int64), ("max_queue", ctypes.c_int32), ("max_book", ctypes.c_int32)]


class AgentState(ctypes.Structure):
    _fields_ = [("cash", ctypes.c_int64), ("shares", ctypes.c_int64), ("n_open", ctypes.c_int64),
                ("last_trade", ctypes.c_int64), ("type", ctypes.c_int32), ("flags", ctypes.c_int32),
                ("starting_cash", ctypes.c_int64)]


class Policy(ctypes.Structure):  # mxa_policy: device pointers, host widths and scalars
    _fields_ = [("params", ctypes.c_void_p), ("n_layers", ctypes.c_int32), ("dims", ctypes.c_int32 * 9),
                ("grid0", ctypes.c_void_p), ("n0", ctypes.c_int32), ("grid1", ctypes.c_void_p), ("n1", ctypes.c_int32),
                ("nh", ctypes.c_double), ("q0", ctypes.c_double), ("table", ctypes.c_void_p),
                ("test", ctypes.c_int32), ("enough", ctypes.c_int32), ("u", ctypes.c_void_p), ("rnd", ctypes.c_void_p),
                ("eps", ctypes.c_void_p)]


class StateSpec(ctypes.Structure):  # mxa_state_spec (include/mxa_state_spec.h): host fields, `grid` a device pointer
    _fields_ = [("n_feat", ctypes.c_int32), ("col", ctypes.c_int32 * 8), ("mul", ctypes.c_double * 8),
                ("div", ctypes.c_double * 8), ("add", ctypes.c_double * 8), ("grid", ctypes.c_void_p),
                ("goff", ctypes.c_int32 * 9)]


class AgentFinal(ctypes.Structure):  # mxa_agent_final
    _fields_ = [("final_fundamental", ctypes.c_int64), ("valuation_int", ctypes.c_int64), ("valuation", ctypes.c_double),
                ("kind", ctypes.c_int32), ("err", ctypes.c_int32)]


class MmParams(ctypes.Structure):  # mxa_mm_params (mxabides.configs.MM_PARAMS_DTYPE is its numpy twin)
    _fields_ = [("mm_pov", ctypes.c_double), ("mm_min_order_size", ctypes.c_int32), ("mm_window_size", ctypes.c_int32),
                ("mm_num_ticks", ctypes.c_int32), ("pad", ctypes.c_int32), ("mm_wake_up_freq_ns", ctypes.c_int64)]


_P, _I32, _I64, _U32, _D, _S = (ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32, ctypes.c_double,
                                ctypes.c_char_p)
_OUT, _N32, _N64 = ctypes.POINTER(_P), ctypes.POINTER(_I32), ctypes.POINTER(_I64)  # mxa_handle**, int32_t*, int64_t*
_TAPE = [_P, _P, _P, _P, _P, _I32]  # t, oid, price, size, buy, n_rec
# every export of include/mxa.h: name -> (argtypes, restype)
BINDINGS = {
    "mxa_create": ([_I32, _I32, _P, _I32, _I32, _OUT], _I32),
    "mxa_create_hist": ([_I32, _I32, _P, _I32, _I32, _P, _P, _I32, _OUT], _I32),
    "mxa_mm_defaults": ([], MmParams),
    "mxa_create_params": ([_I32, _I32, _P, _P, _I32, _I32, _OUT], _I32),
    "mxa_config_defaults": ([_I32, _P], _I32),
    "mxa_config_compile": ([_P, _S, _P, _I32], _I32),
    "mxa_config_key": ([_P, _P], _I32),
    "mxa_config_capacities": ([_P, _P], _I32),
    "mxa_create_config": ([_P, _I32, _P, _I32, _I32, _S, _OUT], _I32),
    "mxa_config_info": ([_I32, _P], _I32),
    "mxa_set_mm_params": ([_P, _P], _I32),
    "mxa_resident_envs": ([_P], _I32),
    "mxa_reset": ([_P, _P], _I32),
    "mxa_set_id_persistence": ([_P, _I32], _I32),
    "mxa_launch": ([_P, _I64], _I32),
    "mxa_sync": ([_P], _I32),
    "mxa_run": ([_P, _I64, _I32, _N32], _I32),
    "mxa_set_launch_schedule": ([_P, _I64], _I32),
    "mxa_set_stop_time": ([_P, _I64], _I32),
    "mxa_run_until": ([_P, _I64, _P], _I32),
    "mxa_finalize": ([_P], _I32),
    "mxa_read_final": ([_P, _I32, _P, _I32], _I32),
    "mxa_read_summary": ([_P, _P], _I32),
    "mxa_read_agents": ([_P, _I32, _P, _I32], _I32),
    "mxa_read_book": ([_P, _I32, _I32, _P, _I32], _I32),
    "mxa_read_trace": ([_P, _I32, _P, _I64, _N64], _I32),
    "mxa_set_seeds": ([_P, _P], _I32),
    "mxa_write_results": ([_P, _P], _I32),
    "mxa_write_records": ([_P, _P], _I32),
    "mxa_read_counters": ([_P, _P], _I32),
    "mxa_read_inplace": ([_P, _P], _I32),
    "mxa_read_raw": ([_P, _I32, _I64, _I64, _P], _I32),
    "mxa_layout": ([_P, _P], _I32),
    "mxa_n_agents": ([_P], _I32),
    "mxa_n_envs": ([_P], _I32),
    "mxa_env_bytes": ([_P], _I64),
    "mxa_set_stream": ([_P, _P], _I32),
    "mxa_last_kernel_ms": ([_P], _D),
    "mxa_last_error": ([_P], _S),
    "mxa_destroy": ([_P], None),
    "mxa_create_replay": (_TAPE + [_I32, _I32, _I32, _OUT], _I32),
    "mxa_create_replay_runner": (_TAPE + [_I32, _I32, _I32, _OUT], _I32),
    "mxa_create_replay_twap": (_TAPE + [_I32, _I32, _I32, _I32, _OUT], _I32),
    "mxa_step": ([_P, _P, _P, _P], _I32),
    "mxa_step_device": ([_P, _P, _P, _P], _I32),
    "mxa_step_many": ([_P, _I32, _P, _P, _P], _I32),
    "mxa_step_policy": ([_P, _I32, _I32, ctypes.POINTER(Policy), _P, _P, _P, _P, _P], _I32),
    "mxa_set_parity_hash": ([_P, _I32], _I32),
    "mxa_write_rl_state": ([_P, _P], _I32),
    "mxa_build_id": ([], _S),
    "mxa_set_book_log": ([_P, _I32], _I32),
    "mxa_set_exchange_log": ([_P, _I32], _I32),
    "mxa_read_book_log": ([_P, _I32, _P, _I64, _N64], _I32),
    "mxa_rng_probe": ([_I32, _U32, _I32, _D, _D, _I32, _P], _I32),
    "mxa_math_probe": ([_I32, _I32, _P, _P, _P, _I64], _I32),
    "mxa_policy_probe": ([_P, _I32, _P, _P, _I32, _N32, _I32, _I32, _P, _P, _P, _P, _P], _I32),
}
EXPORTS = list(BINDINGS)
# every export of include/mxa_snap.h (env-state snapshots; the header is a part of mxa.h's C-ABI)
SNAPSHOT_BINDINGS = {
    "mxa_snapshot_create": ([_P, _I32, _OUT], _I32),
    "mxa_snapshot_save": ([_P, _P, _P], _I32),
    "mxa_snapshot_restore": ([_P, _P, _P], _I32),
    "mxa_snapshot_info": ([_P, _P], _I32),
    "mxa_snapshot_destroy": ([_P], None),
}
# every export of include/mxa_depth.h (L2 book depth of every env in one launch; a part of mxa.h's C-ABI too)
DEPTH_BINDINGS = {
    "mxa_write_depth": ([_P, _I32, _P, _P], _I32),
    "mxa_read_depth": ([_P, _I32, _P, _P], _I32),
}
# every export of include/mxa_bars.h (time bars from the book-update log in one launch; a part of mxa.h's C-ABI too)
BARS_BINDINGS = {
    "mxa_write_bars": ([_P, _I64, _I64, _I32, _P, _P], _I32),
    "mxa_read_bars": ([_P, _I64, _I64, _I32, _P, _P], _I32),
    "mxa_bars_from_records": ([_P, _I32, _P, _I64, _P, _I32, _I64, _I64, _I32, _P, _P], _I32),
}
# the export of include/mxa_variates.h (the variate tables' probe; a part of mxa.h's C-ABI too)
VARIATE_BINDINGS = {
    "mxa_variate_probe": ([_I32, _U32, _P, _I32, _I32, _P, _P], _I32),
}
# the export of include/mxa_streams.h (the head streams' probe; a part of mxa.h's C-ABI too)
STREAM_BINDINGS = {
    "mxa_stream_head_probe": ([_I32, _U32, _I32, _I32, _P, _P], _I32),
}
# the export of include/mxa_policy_features.h (the closed-loop step with a state of N features; a part of mxa.h's C-ABI too)
POLICY_FEATURES_BINDINGS = {
    "mxa_step_policy_spec": ([_P, _I32, _I32, ctypes.POINTER(Policy), ctypes.POINTER(StateSpec), _P, _P, _P, _P, _P],
                             _I32),
}
COUNTER_WORDS = 34  # include/mxa.h MXA_COUNTER_WORDS
INPLACE_WORDS = 12  # include/mxa.h MXA_INPLACE_WORDS
RECORD_WORDS = 12  # include/mxa.h MXA_RECORD_WORDS

_lib = None


class MxaError(RuntimeError):
    pass


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MxaError("libmxa.so not built (%s); run __graft_entry__.build()" % LIB_PATH)
    L = ctypes.CDLL(LIB_PATH)
    for name, (argtypes, restype) in list(BINDINGS.items()) + list(SNAPSHOT_BINDINGS.items()) + list(DEPTH_BINDINGS.items()) \
            + list(BARS_BINDINGS.items()) + list(VARIATE_BINDINGS.items()) + list(STREAM_BINDINGS.items()) + list(POLICY_FEATURES_BINDINGS.items()):
        if hasattr(L, name):  # (MXA_LIB may name a variant build that lacks some)
            f = getattr(L, name)
            f.argtypes, f.restype = argtypes, restype
    _lib = L
    return L


def build_id():
    """the kernel-source hash libmxa was built with (build_lib.build_id)"""
    L = load()
    return L.mxa_build_id().decode() if hasattr(L, "mxa_build_id") else "unknown"
