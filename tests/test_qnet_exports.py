"""libmxa_ddqn.so's Q-network exports (include/mxa_ddqn.h mxa_qnet_*) load without a GPU (their names
against the header: tests/test_lib_exports.py) and refuse unsupported dimensions before any HIP call;
the learner's fused_act switch is off by default and falls back quietly on the CPU."""
import ctypes

import pytest
import torch

from mxabides import ddqn

HIP_ERROR_INVALID_VALUE = 1


def _lib():
    L = ddqn.lib()
    assert L is not None, "libmxa_ddqn.so not built (build_lib.build_ddqn)"
    return L


def _dims(*w):
    return (ctypes.c_int * len(w))(*w)


@pytest.mark.parametrize("n,dims", [(1, (2,) + (8,) * 9),            # n_layers = 9
                                    (1, (2, 257, 24)),               # a width of 257
                                    (1, (2, 0, 24)),                 # a width of 0
                                    (-1, (2, 32, 24)),               # n = -1
                                    (1, (2,))])                      # n_layers = 0
def test_qnet_bad_dimensions_are_refused_without_a_device(n, dims):
    L = _lib()
    d = _dims(*dims)
    assert L.mxa_qnet_forward(None, n, None, None, len(dims) - 1, d, None) == HIP_ERROR_INVALID_VALUE
    assert L.mxa_qnet_act(None, n, None, None, len(dims) - 1, d, 1, 0, None, None, None, 9, None, None, 1.0, None,
                          None, None) == HIP_ERROR_INVALID_VALUE


def test_qnet_act_refuses_narrow_obs_and_accepts_empty_batch():
    L = _lib()
    d = _dims(2, 32, 24)
    assert L.mxa_qnet_act(None, 4, None, None, 2, d, 1, 0, None, None, None, 1, None, None, 1.0, None, None,
                          None) == HIP_ERROR_INVALID_VALUE
    # no action buffer: refused (before any HIP call), not silently a forward
    assert L.mxa_qnet_act(None, 4, None, None, 2, d, 1, 0, None, None, None, 9, None, None, 1.0, None, None,
                          None) == HIP_ERROR_INVALID_VALUE
    assert L.mxa_qnet_forward(None, 0, None, None, 2, d, None) == 0
    assert L.mxa_qnet_act(None, 0, None, None, 2, d, 1, 0, None, None, None, 9, None, None, 1.0, None, None,
                          None) == 0


def test_fused_act_on_cpu_raises():
    with pytest.raises(RuntimeError):
        ddqn.DDQNLearner(device="cpu", fused_act=True)
    with pytest.raises(RuntimeError):
        ddqn.DDQNLearner(device="cpu", fused_act=True, dtype=torch.float64)


def test_fused_act_env_switch_falls_back_on_cpu(monkeypatch):
    s = torch.randint(0, 200, (257, 2), generator=torch.Generator().manual_seed(3)).float()
    monkeypatch.delenv("MXA_DDQN_FUSED_ACT", raising=False)
    ref = ddqn.DDQNLearner(device="cpu", seed=4)
    assert ref.fused_act is False
    monkeypatch.setenv("MXA_DDQN_FUSED_ACT", "1")
    L = ddqn.DDQNLearner(device="cpu", seed=4)
    assert L.fused_act is False
    assert torch.equal(L.q_values(s), ref.q_values(s))
    assert torch.equal(L.choose_action(s), ref.choose_action(s))
    assert torch.equal(L.gen.get_state(), ref.gen.get_state())
    with pytest.raises(RuntimeError):
        L.act(s)
