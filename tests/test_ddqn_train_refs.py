"""include/mxa_ddqn_train.h without a GPU: the exact cases of tests/test_gpu_ddqn_train.py satisfy
their conditions and are exact in float32 in either summation order; update_ref_f32 agrees with
oracle/ddqn_ref.rmsprop_step; the header's names are the library's new exports and refuse
unsupported arguments before any HIP call; DDQNLearner's fused_learn switch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ddqn_ref
import ddqn_train_ref as T
from mxabides import ddqn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_ERROR_INVALID_VALUE = 1
NAMES = ["mxa_qnet_grad", "mxa_qnet_train", "mxa_qnet_train_workspace", "mxa_qnet_update"]


@pytest.mark.parametrize("dims,batch,rate,seed", T.EXACT_CASES)
def test_exact_cases_are_exact_in_float32_in_either_order(dims, batch, rate, seed):
    c = T.exact_case(dims, batch, rate, seed)  # asserts the magnitude and the nonzero-gradient conditions
    assert c["worst_forward"] * 8 < 2 ** 24 and c["worst_backward"] * 8 < 2 ** 24  # an 8x margin
    ref_g = T.flat_grads(c["grads"])
    for reverse in (False, True):
        tgt, loss, g = T.eval_f32(c, reverse)
        assert np.array_equal(tgt.astype(np.float64), c["tgt"]), (dims, batch, reverse)
        assert float(loss) == c["loss"], (dims, batch, reverse)
        assert np.array_equal(g.astype(np.float64), ref_g), (dims, batch, reverse)
    # float32 holds the reference exactly
    assert np.array_equal(ref_g.astype(np.float32).astype(np.float64), ref_g)
    assert np.float64(np.float32(c["loss"])) == c["loss"]


def test_inexact_shapes_are_refused():
    with pytest.raises(AssertionError):
        T.exact_case(T.NNMODEL_1, 33, 0.5, 3)
    with pytest.raises(AssertionError):
        T.exact_case(T.NNMODEL_1[:-1] + (24,), 32, 0.5, 3)


def test_update_ref_f32_agrees_with_rmsprop_step():
    """within test_gpu_learner_updates_match_numpy_reference's float32 tolerances"""
    rs = np.random.RandomState(1)
    dims = (2, 32, 64, 24)
    layers = [(rs.normal(0, 0.3, (dims[i], dims[i + 1])), rs.normal(0, 0.3, dims[i + 1])) for i in range(3)]
    grads = [(rs.normal(0, 0.05, W.shape), rs.normal(0, 0.05, b.shape)) for W, b in layers]
    rms = [(rs.rand(*W.shape) * 0.01, rs.rand(*b.shape) * 0.01) for W, b in layers]
    new, new_rms = ddqn_ref.rmsprop_step(layers, grads, rms, 0.01)
    p, g, r = (ddqn_ref.flat_params(x) for x in (layers, grads, rms))
    tflat = np.zeros_like(p)
    for counter in (0, 1):
        e2, t2, r2, eps2, c2 = T.update_ref_f32(p, tflat, g, r, True, counter, 5, 0.25, 0.5, 0.9, 0.01)
        np.testing.assert_allclose(e2, ddqn_ref.flat_params(new), rtol=2e-3, atol=2e-4)
        np.testing.assert_allclose(r2, ddqn_ref.flat_params(new_rms), rtol=2e-3, atol=2e-4)
        assert np.array_equal(t2, p if counter == 0 else tflat)
        assert eps2 == 0.75 and c2 == counter + 1
    e2, t2, r2, eps2, c2 = T.update_ref_f32(p, tflat, g, r, False, 0, 5, 0.25, 0.5, 0.9, 0.01)
    assert np.array_equal(e2, p) and np.array_equal(t2, tflat) and np.array_equal(r2, r) and (eps2, c2) == (0.25, 0)
    # epsilon: no increment; the overshoot just under eps_max, then the clamp
    assert T.update_ref_f32(p, tflat, g, r, True, 0, 5, 0.9, None, 0.9, 0.01)[3] == 0.9
    under = np.nextafter(0.9, 0.0)
    assert T.update_ref_f32(p, tflat, g, r, True, 0, 5, under, 0.5, 0.9, 0.01)[3] == under + 0.5
    assert T.update_ref_f32(p, tflat, g, r, True, 0, 5, under + 0.5, 0.5, 0.9, 0.01)[3] == 0.9


def _lib():
    L = ddqn.lib()
    assert L is not None, "libmxa_ddqn.so not built (build_lib.build_ddqn)"
    return L


def test_train_header_names_are_the_new_exports():
    src = open(os.path.join(ROOT, "include", "mxa_ddqn_train.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert sorted(set(re.findall(r"\b(mxa_[a-z_0-9]+)\s*\(", src))) == NAMES
    L = _lib()
    for n in NAMES:
        assert hasattr(L, n), n
        assert getattr(L, n).argtypes is not None, n
    # the library's exported mxa_* names are those of its two headers
    old = open(os.path.join(ROOT, "include", "mxa_ddqn.h")).read()
    old = re.sub(r"/\*.*?\*/", "", old, flags=re.S)
    declared = set(NAMES) | set(re.findall(r"\b(mxa_[a-z_0-9]+)\s*\(", old))
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", L._name], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("mxa_")}
    assert exported == declared


def _dims(*w):
    return (ctypes.c_int * len(w))(*w)


ONE = ctypes.c_void_p(16)  # a non-null pointer that is never read: every refusal comes before any HIP call


def _grad(L, batch, dims, grad=ONE, loss=ONE):
    return L.mxa_qnet_grad(None, batch, ONE, ONE, ONE, ONE, ONE, ONE, len(dims) - 1, _dims(*dims), None, 0.1, 0.98, ONE,
                           grad, loss, None)


def _train(L, batch, dims, rms=ONE, counter=ONE, eps=ONE, it=5):
    return L.mxa_qnet_train(None, batch, ONE, ONE, ONE, ONE, ONE, ONE, len(dims) - 1, _dims(*dims), None, 0.1, 0.98, ONE,
                            None, None, None, rms, None, counter, it, eps, 0, 0.0, 0.9, 0.01, 0.9, 1e-7)


@pytest.mark.parametrize("batch,dims", [(32, (2,)),                  # 0 layers
                                        (32, (2,) + (8,) * 9),       # 9 layers
                                        (32, (2, 0, 24)),            # a width of 0
                                        (32, (2, 257, 24)),          # a width of 257
                                        (-1, (2, 32, 24)),           # a batch of -1
                                        (257, (2, 32, 24))])         # a batch of 257
def test_train_bad_dimensions_are_refused_without_a_device(batch, dims):
    L = _lib()
    assert _grad(L, batch, dims) == HIP_ERROR_INVALID_VALUE
    assert _train(L, batch, dims) == HIP_ERROR_INVALID_VALUE
    assert L.mxa_qnet_train_workspace(batch, len(dims) - 1, _dims(*dims)) == -1


def test_train_null_outputs_are_refused_and_empty_batch_accepted():
    L = _lib()
    dims = (2, 32, 24)
    assert _grad(L, 32, dims, grad=None) == HIP_ERROR_INVALID_VALUE
    assert _grad(L, 32, dims, loss=None) == HIP_ERROR_INVALID_VALUE
    assert _train(L, 32, dims, rms=None) == HIP_ERROR_INVALID_VALUE
    assert _train(L, 32, dims, counter=None) == HIP_ERROR_INVALID_VALUE
    assert _train(L, 32, dims, eps=None) == HIP_ERROR_INVALID_VALUE
    assert _train(L, 32, dims, it=0) == HIP_ERROR_INVALID_VALUE
    # a null workspace, and a rate of 1
    assert L.mxa_qnet_grad(None, 32, ONE, ONE, ONE, ONE, ONE, ONE, 2, _dims(*dims), None, 0.1, 0.98, None, ONE, ONE,
                           None) == HIP_ERROR_INVALID_VALUE
    assert L.mxa_qnet_grad(None, 32, ONE, ONE, ONE, ONE, ONE, ONE, 2, _dims(*dims), None, 1.0, 0.98, ONE, ONE, ONE,
                           None) == HIP_ERROR_INVALID_VALUE
    upd = lambda n, grad=ONE, ev=ONE, tg=ONE, rms=ONE, counter=ONE, eps=ONE, it=5: L.mxa_qnet_update(
        None, n, grad, ev, tg, rms, None, counter, it, eps, 0, 0.0, 0.9, 0.01, 0.9, 1e-7)
    assert upd(0) == HIP_ERROR_INVALID_VALUE and upd(-1) == HIP_ERROR_INVALID_VALUE
    assert upd(8 * (256 * 256 + 256) + 1) == HIP_ERROR_INVALID_VALUE
    for k in ("grad", "ev", "tg", "rms", "counter", "eps"):
        assert upd(100, **{k: None}) == HIP_ERROR_INVALID_VALUE, k
    assert upd(100, it=0) == HIP_ERROR_INVALID_VALUE
    assert _grad(L, 0, dims, grad=None, loss=None) == 0
    assert _train(L, 0, dims) == 0
    # the workspace: every hidden activation and every delta of the batch, the rows' losses, one flag
    assert L.mxa_qnet_train_workspace(32, 2, _dims(*dims)) == 4 * (32 * 32 + 32 * 32 + 32 * 24 + 32 + 1)
    assert L.mxa_qnet_train_workspace(0, 2, _dims(*dims)) == 4


def test_fused_learn_on_cpu_raises():
    with pytest.raises(RuntimeError):
        ddqn.DDQNLearner(device="cpu", fused_learn=True)
    with pytest.raises(RuntimeError):
        ddqn.DDQNLearner(device="cpu", fused_learn=True, dtype=torch.float64)


def test_fused_learn_env_switch_falls_back_on_cpu(monkeypatch):
    monkeypatch.delenv("MXA_DDQN_FUSED_LEARN", raising=False)
    assert ddqn.DDQNLearner(device="cpu", seed=4).fused_learn is False
    monkeypatch.setenv("MXA_DDQN_FUSED_LEARN", "1")
    L = ddqn.DDQNLearner(device="cpu", seed=4)
    assert L.fused_learn is False and L.fused_act is False
