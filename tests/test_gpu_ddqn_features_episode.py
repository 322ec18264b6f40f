"""run_episode on a task of six features (mxabides.ddqn ExecutionTask(features=...)) and a learner
as wide: the PyTorch ops (fused=False), the per-period kernels (fused=True, include/
mxa_ddqn_features.h) and the policy inside the step kernel (rollout=True, include/
mxa_policy_features.h) give the same two training episodes bit for bit: rewards, actions, stored and
env_steps, the replay ring, the learner's weights, RMSprop state, epsilon and counter. And an update
in the kernels (fused_learn=True), width-generic already, completes on it and reproduces itself."""
import pytest
import torch

import ddqn_features_ref as R
from mxabides import ddqn
from mxabides.gym import VecABIDESEnv

pytestmark = pytest.mark.gpu
SEEDS = [123456789, 2024, 7, 123, 99991, 31337, 4242, 555, 1, 2, 3, 4, 5, 6, 8, 9] * 4  # 64 envs
F = 6
_CACHE = {}


def _run(fused, rollout, fused_learn=False, episodes=2):
    key = (fused, rollout, fused_learn)
    if key in _CACHE:
        return _CACHE[key]
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    v = VecABIDESEnv(seeds=SEEDS)
    v.set_stream(stream.cuda_stream)
    v.set_parity_hash(True)
    learner = ddqn.DDQNLearner(n_state=F, device="cuda", seed=5, mode="train", fused_act=True, fused_learn=fused_learn,
                               epsilon_increment=0.05)
    task = ddqn.ExecutionTask(device="cuda", features=R.to_features(R.FEATURE_SETS[F]))
    out = {}
    for ep in range(episodes):
        res = ddqn.run_episode(v, learner, task, seeds=[s + 77 * ep for s in SEEDS], fused=fused, rollout=rollout)
        torch.cuda.synchronize()
        for k in ("rewards", "actions", "stored", "env_steps"):
            out["%s[%d]" % (k, ep)] = res[k].clone()
        summ = v.summary()
        out["hash[%d]" % ep] = torch.from_numpy(summ["hash"].astype("int64"))
    m = learner.memory
    n_dev = int(m.n_dev.item())
    k = min(n_dev, m.cap)
    out.update({"n_dev": m.n_dev.clone(), "ring_s": m.s[:k].clone(), "ring_s2": m.s2[:k].clone(), "ring_a": m.a[:k].clone(),
                "ring_r": m.r[:k].clone(), "eflat": learner.eflat.clone(), "tflat": learner.tflat.clone(),
                "rms": learner.rms.clone(), "eps": learner._eps.clone(), "counter": learner._counter.clone()})
    v.close()
    _CACHE[key] = out
    return out


def _bits(x):
    return x.view(torch.int64) if x.dtype == torch.float64 else x.view(torch.int32) if x.dtype == torch.float32 else x


def _assert_same(a, b, what):
    assert set(a) == set(b)
    for key in a:
        assert a[key].shape == b[key].shape and a[key].dtype == b[key].dtype, (what, key)
        assert torch.equal(_bits(a[key]), _bits(b[key])), (what, key)


@pytest.mark.parametrize("path", ["fused=True", "rollout=True"])
def test_gpu_features_episode_paths_match_the_pytorch_ops(path):
    ref = _run(False, False)
    got = _run(True, path == "rollout=True")
    _assert_same(got, ref, path)
    # conditions on the run: six-element rows were stored and learned from, and the market columns
    # in them move (the state is not the two schedule elements alone)
    assert tuple(ref["ring_s"].shape[1:]) == (F,) and int(ref["n_dev"]) > 64 and int(ref["counter"]) > 0
    assert float(ref["eps"]) > 0 and int(ref["stored[1]"]) > 0
    for f in range(2, F):
        assert len(torch.unique(ref["ring_s2"][:, f])) > 1, f
    assert len(torch.unique(ref["actions[1]"])) > 1


def test_gpu_features_episode_fused_learn_completes_and_reproduces_itself():
    a = _run(True, True, fused_learn=True)
    _CACHE.pop((True, True, True))
    b = _run(True, True, fused_learn=True)
    _assert_same(a, b, "fused_learn twice")
    assert int(a["counter"]) > 0 and bool(torch.isfinite(a["eflat"]).all())
    assert tuple(a["ring_s"].shape[1:]) == (F,)
