"""What every libmxa entry point (include/mxa.h) answers before it reaches HIP: the argument
checks of the constructors, the null-handle answer of every handle-taking call, the host-only
mxa_config_* calls and the probes.  No call here gets as far as a device, so the module needs the
built library and no GPU; it pins the host side of csrc/mxa_api.hip across refactors."""
import ctypes

import numpy as np
import pytest

from mxabides import _lib, composition, configs

OK, EINVAL, EHIP, ERANGE = 0, -1, -2, -4
N_CONFIGS = 18  # csrc/mxa_entry.h MXA_N_CONFIGS
T0 = 34200 * 10 ** 9


@pytest.fixture(scope="module")
def L():
    return _lib.load()


@pytest.fixture()
def out():
    return ctypes.c_void_p()


SEEDS = np.arange(4, dtype=np.uint32)


def _create(L, out, config=_lib.MXA_RMSC03, n_envs=4, seeds=SEEDS, trace_cap=0, ref=True):
    return L.mxa_create(config, n_envs, None if seeds is None else seeds.ctypes.data, 0, trace_cap,
                        ctypes.byref(out) if ref else None)


def test_create(L, out):
    assert _create(L, out, ref=False) == EINVAL
    assert _create(L, out, n_envs=0) == EINVAL
    assert _create(L, out, n_envs=-3) == EINVAL
    assert _create(L, out, seeds=None) == EINVAL
    assert _create(L, out, trace_cap=-1) == EINVAL
    assert _create(L, out, config=-1) == EINVAL
    assert _create(L, out, config=N_CONFIGS) == EINVAL
    # the configurations with constructors of their own: replay (3, 13, 14), ExternalFileOracle (11, 12)
    for c in (_lib.MXA_MARKETREPLAY, _lib.MXA_HIST_FUND_VALUE, _lib.MXA_HIST_FUND_DIVERSE,
              _lib.MXA_MARKETREPLAY_RUNNER, _lib.MXA_MARKETREPLAY_TWAP):
        assert _create(L, out, config=c) == EINVAL, c
    # the script's defaults in every env go through mxa_create_params' checks: bad arguments first
    assert _create(L, out, config=_lib.MXA_RMSC03_MM, n_envs=0) == EINVAL
    assert not out


def _params(L, out, config=_lib.MXA_RMSC03, per_env="default", **fields):
    p = configs.mm_params(4)
    for k, v in fields.items():
        p[k][2] = v  # one env of the batch is enough to refuse it
    pe = p.ctypes.data if isinstance(per_env, str) else per_env
    return L.mxa_create_params(config, 4, SEEDS.ctypes.data, pe, 0, 0, ctypes.byref(out))


def test_create_params(L, out):
    assert _params(L, out, config=_lib.MXA_RMSC03_MM) == EINVAL
    assert _params(L, out, config=_lib.MXA_RMSC01) == EINVAL
    assert _params(L, out, per_env=None) == EINVAL
    assert _params(L, out, mm_pov=float("nan")) == EINVAL
    assert _params(L, out, mm_pov=-0.05) == EINVAL
    assert _params(L, out, mm_pov=1.5e12) == EINVAL
    assert _params(L, out, mm_num_ticks=100001) == EINVAL
    assert _params(L, out, mm_num_ticks=-1) == EINVAL
    assert _params(L, out, mm_wake_up_freq_ns=0) == EINVAL
    assert _params(L, out, mm_window_size=-1) == EINVAL
    assert _params(L, out, mm_min_order_size=-1) == EINVAL
    p = configs.mm_params(4)
    assert L.mxa_create_params(_lib.MXA_RMSC03, 0, SEEDS.ctypes.data, p.ctypes.data, 0, 0, ctypes.byref(out)) == EINVAL
    assert L.mxa_create_params(_lib.MXA_RMSC03, 4, None, p.ctypes.data, 0, 0, ctypes.byref(out)) == EINVAL
    assert L.mxa_create_params(_lib.MXA_RMSC03, 4, SEEDS.ctypes.data, p.ctypes.data, 0, -1, ctypes.byref(out)) == EINVAL
    assert L.mxa_create_params(_lib.MXA_RMSC03, 4, SEEDS.ctypes.data, p.ctypes.data, 0, 0, None) == EINVAL
    assert not out


def _hist(L, out, config=_lib.MXA_HIST_FUND_VALUE, t=(1, 2, 3), v=(1e5, 1e5 + 1, 1e5 + 2), n=None, n_envs=4,
          trace_cap=0):
    ft, fv = np.array(t, dtype=np.int64) + T0, np.array(v, dtype=np.float64)
    return L.mxa_create_hist(config, n_envs, SEEDS.ctypes.data, 0, trace_cap, ft.ctypes.data, fv.ctypes.data,
                             len(ft) if n is None else n, ctypes.byref(out))


def test_create_hist(L, out):
    assert _hist(L, out, config=_lib.MXA_RMSC03) == EINVAL
    assert _hist(L, out, config=_lib.MXA_RANDOM_FUND_VALUE) == EINVAL
    assert _hist(L, out, n=0) == EINVAL
    assert _hist(L, out, t=(1, 3, 2)) == EINVAL
    assert _hist(L, out, v=(1e5, float("nan"), 1e5)) == EINVAL
    assert _hist(L, out, v=(1e5, 1.5e15, 1e5)) == EINVAL
    assert _hist(L, out, v=(1e5, -1.5e15, 1e5)) == EINVAL
    assert _hist(L, out, config=_lib.MXA_HIST_FUND_DIVERSE, n_envs=0) == EINVAL
    assert _hist(L, out, trace_cap=-1) == EINVAL
    ft, fv = np.array([1, 2], dtype=np.int64), np.array([1.0, 2.0])
    h = ctypes.byref(out)
    assert L.mxa_create_hist(11, 4, SEEDS.ctypes.data, 0, 0, None, fv.ctypes.data, 2, h) == EINVAL
    assert L.mxa_create_hist(11, 4, SEEDS.ctypes.data, 0, 0, ft.ctypes.data, None, 2, h) == EINVAL
    assert L.mxa_create_hist(11, 4, None, 0, 0, ft.ctypes.data, fv.ctypes.data, 2, h) == EINVAL
    assert L.mxa_create_hist(11, 4, SEEDS.ctypes.data, 0, 0, ft.ctypes.data, fv.ctypes.data, 2, None) == EINVAL
    assert not out


TAPE = dict(t=[T0 + 10, T0 + 20, T0 + 30], oid=[100000, 100001, 100000], price=[5000, 5001, 5000],
            size=[100, 50, 0], buy=[1, 0, 1])


def _replay(L, out, which, n_envs=1, trace_cap=0, n_rec=None, **fields):
    f = dict(TAPE, **fields)
    a = [np.ascontiguousarray(f[k], dtype=np.int64) for k in ("t", "oid", "price", "size")]
    b = np.ascontiguousarray(f["buy"], dtype=np.int8)
    tp = [x.ctypes.data for x in a] + [b.ctypes.data, len(a[0]) if n_rec is None else n_rec]
    tail = (n_envs, 0, trace_cap, ctypes.byref(out))
    if which == "twap":
        return L.mxa_create_replay_twap(*tp, 0, *tail)
    return (L.mxa_create_replay if which == "gym" else L.mxa_create_replay_runner)(*tp, *tail)


@pytest.mark.parametrize("which", ["gym", "runner", "twap"])
def test_create_replay(L, out, which):
    assert _replay(L, out, which, t=TAPE["t"][::-1]) == EINVAL
    assert _replay(L, out, which, oid=[100000, -5, 100000]) == EINVAL
    assert _replay(L, out, which, price=[5000, 1 << 20, 5000]) == EINVAL
    assert _replay(L, out, which, price=[5000, -1, 5000]) == EINVAL
    assert _replay(L, out, which, size=[100, -1, 0]) == EINVAL
    assert _replay(L, out, which, n_rec=0) == EINVAL
    assert _replay(L, out, which, n_envs=0) == EINVAL
    assert _replay(L, out, which, trace_cap=-1) == EINVAL
    # one ORDER_ID 0 record takes an auto id, so the auto ids reach rl_ids + 1 at least: an explicit
    # id 1 is never above that, whatever the configuration's rl_ids
    assert _replay(L, out, which, oid=[0, 1, 1]) == EINVAL
    assert not out


def test_create_replay_null_arrays(L, out):
    a = np.array(TAPE["t"], dtype=np.int64)
    b = np.array(TAPE["buy"], dtype=np.int8)
    good = [a.ctypes.data] * 4 + [b.ctypes.data]
    for i in range(5):
        tp = list(good)
        tp[i] = None
        assert L.mxa_create_replay(*tp, 3, 1, 0, 0, ctypes.byref(out)) == EINVAL
        assert L.mxa_create_replay_runner(*tp, 3, 1, 0, 0, ctypes.byref(out)) == EINVAL
        assert L.mxa_create_replay_twap(*tp, 3, 1, 1, 0, 0, ctypes.byref(out)) == EINVAL
    assert L.mxa_create_replay(*good, 3, 1, 0, 0, None) == EINVAL
    assert not out


def test_null_handle(L):
    buf = np.zeros(64, dtype=np.int64)
    p = buf.ctypes.data
    pol = _lib.Policy()
    n = ctypes.c_int64()
    n32 = ctypes.c_int32()
    einval = {
        "mxa_reset": (None,), "mxa_launch": (10,), "mxa_sync": (), "mxa_run": (10, 0, ctypes.byref(n32)),
        "mxa_read_summary": (p,), "mxa_set_stream": (None,), "mxa_set_seeds": (p,), "mxa_write_results": (p,),
        "mxa_layout": (p,), "mxa_step": (p, p, p), "mxa_step_device": (p, p, p), "mxa_finalize": (),
        "mxa_read_final": (0, p, 1), "mxa_write_rl_state": (p,), "mxa_set_parity_hash": (1,),
        "mxa_set_book_log": (16,), "mxa_read_book_log": (0, p, 1, ctypes.byref(n)), "mxa_write_records": (p,),
        "mxa_set_id_persistence": (1,), "mxa_read_counters": (p,), "mxa_read_inplace": (p,),
        "mxa_set_stop_time": (T0,), "mxa_run_until": (T0, p), "mxa_set_mm_params": (p,), "mxa_resident_envs": (),
        "mxa_set_exchange_log": (1,), "mxa_step_many": (2, p, p, p), "mxa_set_launch_schedule": (0,),
        "mxa_step_policy": (1, 0, ctypes.byref(pol), p, p, p, p, None),
    }
    erange = {"mxa_read_agents": (0, p, 1), "mxa_read_book": (0, 0, p, 1), "mxa_read_trace": (0, p, 1, ctypes.byref(n)),
              "mxa_read_raw": (0, 0, 8, p)}
    for name, args in einval.items():
        assert getattr(L, name)(None, *args) == EINVAL, name
    for name, args in erange.items():
        assert getattr(L, name)(None, *args) == ERANGE, name
    # every export that takes a handle is in one of the two tables
    free = {"mxa_create", "mxa_create_params", "mxa_create_hist", "mxa_create_replay", "mxa_create_replay_runner",
            "mxa_create_replay_twap", "mxa_create_config", "mxa_config_defaults", "mxa_config_compile",
            "mxa_config_key", "mxa_config_capacities", "mxa_config_info", "mxa_mm_defaults", "mxa_build_id",
            "mxa_rng_probe", "mxa_math_probe", "mxa_policy_probe"}
    getters = {"mxa_n_agents", "mxa_n_envs", "mxa_env_bytes", "mxa_last_kernel_ms", "mxa_last_error", "mxa_destroy"}
    assert set(einval) | set(erange) | free | getters == set(_lib.EXPORTS)
    assert L.mxa_n_agents(None) == 0 and L.mxa_n_envs(None) == 0 and L.mxa_env_bytes(None) == 0
    assert L.mxa_last_kernel_ms(None) == 0.0
    assert isinstance(L.mxa_last_error(None), bytes)
    assert L.mxa_destroy(None) is None


def test_config_calls(L, out):
    c = composition.MarketConfig()
    assert L.mxa_config_defaults(_lib.MXA_RMSC01, ctypes.byref(c)) == EINVAL
    assert L.mxa_last_error(None) == b"mxa_config_defaults: no such base script"
    assert L.mxa_config_defaults(-1, ctypes.byref(c)) == EINVAL
    assert L.mxa_config_defaults(_lib.MXA_RMSC03, None) == EINVAL
    assert L.mxa_config_defaults(_lib.MXA_RMSC03, ctypes.byref(c)) == OK and c.base == _lib.MXA_RMSC03
    k1, k2, k3 = (ctypes.create_string_buffer(17) for _ in range(3))
    assert L.mxa_config_key(ctypes.byref(c), k1) == OK
    d = composition.MarketConfig.from_buffer_copy(bytes(c))
    d.date_ns += 86400 * 10 ** 9
    assert L.mxa_config_key(ctypes.byref(d), k2) == OK
    d.n_noise += 1
    assert L.mxa_config_key(ctypes.byref(d), k3) == OK
    assert len(k1.value) == 16 and k1.value == k2.value and k3.value != k1.value
    assert L.mxa_config_key(None, k1) == EINVAL and L.mxa_config_key(ctypes.byref(c), None) == EINVAL
    cap = (ctypes.c_int32 * 2)()
    assert L.mxa_config_capacities(None, cap) == EINVAL
    assert L.mxa_last_error(None) == b"mxa_config_capacities: bad arguments"
    assert L.mxa_config_capacities(ctypes.byref(c), cap) == OK and cap[0] > 0 and cap[1] > 0
    assert L.mxa_config_compile(None, None, None, 0) == EINVAL
    assert L.mxa_last_error(None) == b"mxa_config_compile: null composition"
    assert L.mxa_create_config(None, 4, SEEDS.ctypes.data, 0, 0, None, ctypes.byref(out)) == EINVAL
    assert L.mxa_last_error(None) == b"mxa_create_config: bad arguments"
    for args in ((0, SEEDS.ctypes.data, 0, 0, None, ctypes.byref(out)), (4, None, 0, 0, None, ctypes.byref(out)),
                 (4, SEEDS.ctypes.data, 0, -1, None, ctypes.byref(out)), (4, SEEDS.ctypes.data, 0, 0, None, None)):
        assert L.mxa_create_config(ctypes.byref(c), *args) == EINVAL
    info = np.zeros(8, dtype=np.int64)
    assert L.mxa_config_info(-1, info.ctypes.data) == EINVAL
    assert L.mxa_config_info(N_CONFIGS, info.ctypes.data) == EINVAL
    assert L.mxa_config_info(_lib.MXA_RMSC03, None) == EINVAL
    assert L.mxa_config_info(_lib.MXA_RMSC03, info.ctypes.data) == OK and info[0] == 64
    assert not out


def test_probes(L):
    o = np.zeros(8)
    x = np.zeros(8, dtype=np.float32)
    assert L.mxa_rng_probe(0, 1, 1, 0.0, 1.0, 0, o.ctypes.data) == EINVAL
    assert L.mxa_rng_probe(0, 1, 1, 0.0, 1.0, 8, None) == EINVAL
    assert L.mxa_math_probe(0, 0, o.ctypes.data, None, o.ctypes.data, 0) == EINVAL
    assert L.mxa_math_probe(0, 0, None, None, o.ctypes.data, 8) == EINVAL
    assert L.mxa_math_probe(0, 0, o.ctypes.data, None, None, 8) == EINVAL
    dims = (ctypes.c_int32 * 3)(2, 4, 3)
    p, q = x.ctypes.data, o.ctypes.data
    probe = lambda n=1, x=p, params=p, nl=2, dims=dims, q=q, a=None: L.mxa_policy_probe(
        None, n, x, params, nl, dims, 1, 1, None, None, None, q, a)
    assert probe(n=0) == EINVAL
    assert probe(x=None) == EINVAL
    assert probe(params=None) == EINVAL
    assert probe(nl=0) == EINVAL and probe(nl=9) == EINVAL
    assert probe(dims=(ctypes.c_int32 * 3)(2, 257, 3)) == EINVAL
    assert probe(dims=(ctypes.c_int32 * 3)(2, 0, 3)) == EINVAL
    assert probe(dims=None) == EINVAL
    assert probe(q=None, a=None) == EINVAL
    # the action of a training-mode policy needs choose_action's draws
    assert L.mxa_policy_probe(None, 1, p, p, 2, dims, 0, 1, None, None, None, q, q) == EINVAL

