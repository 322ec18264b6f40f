"""run_episode(rollout=True): the episode as the launches of rollout_chunks with the policy inside
the step kernel (include/mxa.h mxa_step_policy) is bitwise the episode of rollout=False: the returned
dict, the replay ring, the learner (weights, RMSprop state, epsilon, counter, losses), the three
random streams and the env blocks, over three consecutive episodes in train mode (with the update
on autograd and in the kernels) and in test mode; with 8 envs and a batch of 32 the replay reaches a
batch mid-episode, so both the one-period launches and the chunks run."""
import pytest
import torch

from mxabides import ddqn
from mxabides.gym import VecABIDESEnv

pytestmark = pytest.mark.gpu
SEEDS = [123456789, 2024, 7, 123, 99991, 31337, 4242, 555, 1, 2, 3, 4, 5, 6, 8, 9]  # test_gpu_ddqn's


def _run(rollout, seeds, mode, fused_learn, batch_size, episodes=3, epsilon_increment=0.05):
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    v = VecABIDESEnv(seeds=seeds)
    v.set_stream(stream.cuda_stream)
    v.set_parity_hash(True)
    learner = ddqn.DDQNLearner(device="cuda", seed=5, batch_size=batch_size, mode=mode, fused_act=True,
                               fused_learn=fused_learn, epsilon_increment=epsilon_increment)
    task = ddqn.ExecutionTask(device="cuda")
    out = {"eps": [], "launches": []}
    for ep in range(episodes):
        rec, timing = [], []
        res = ddqn.run_episode(v, learner, task, seeds=[s + 77 * ep for s in seeds], record=rec, timing=timing,
                               fused=True, rollout=rollout)
        torch.cuda.synchronize()
        e = {k: (x.clone() if torch.is_tensor(x) else x) for k, x in res.items()}
        e["action_vectors"] = torch.stack(rec)
        summ = v.summary()
        e.update({"summary." + k: torch.from_numpy(summ[k].astype("int64")) for k in
                  ("events", "hash", "status", "err", "current_time")})
        out["eps"].append(e)
        out["launches"].append(len(timing))
    m = learner.memory
    out["n_dev"] = int(m.n_dev.item())
    k = min(out["n_dev"], m.cap)
    out["learner"] = {"ring_s": m.s[:k].clone(), "ring_s2": m.s2[:k].clone(), "ring_a": m.a[:k].clone(),
                      "ring_r": m.r[:k].clone(), "eflat": learner.eflat.clone(), "tflat": learner.tflat.clone(),
                      "rms": learner.rms.clone(), "eps": learner._eps.clone(), "counter": learner._counter.clone(),
                      "gen": learner.gen.get_state(), "gen_sample": learner.gen_sample.get_state(),
                      "gen_drop": learner.gen_drop.get_state()}
    out["cost_hist"] = learner.cost_hist
    v.close()
    return out


def _bits(x):
    return x.view(torch.int64) if x.dtype == torch.float64 else x.view(torch.int32) if x.dtype == torch.float32 else x


def _assert_same(a, b, what):
    for i, (ea, eb) in enumerate(zip(a["eps"], b["eps"])):
        assert set(ea) == set(eb)
        for key in ea:
            if torch.is_tensor(ea[key]):
                assert ea[key].shape == eb[key].shape and ea[key].dtype == eb[key].dtype, (what, i, key)
                assert torch.equal(_bits(ea[key]), _bits(eb[key])), (what, i, key)
            else:
                assert ea[key] == eb[key], (what, i, key)
    assert a["n_dev"] == b["n_dev"], what
    for key in a["learner"]:
        assert torch.equal(_bits(a["learner"][key]), _bits(b["learner"][key])), (what, key)
    assert a["cost_hist"] == b["cost_hist"], what


@pytest.mark.parametrize("mode,fused_learn", [("train", False), ("train", True), ("test", False)])
def test_gpu_ddqn_rollout_equals_per_step_episodes(mode, fused_learn):
    seeds = SEEDS * 4  # 64 envs
    a = _run(False, seeds, mode, fused_learn, 32)
    b = _run(True, seeds, mode, fused_learn, 32)
    _assert_same(a, b, (mode, fused_learn))
    assert a["launches"] == [27] * 3  # the timed launches of the per-step loop: its periods
    if mode == "train":
        # 64 envs: the replay holds a batch after the first period, so from the second launch on
        # the episode runs in rollout_chunks' launches: 1 + 1 + five chunks and the last period
        assert b["launches"] == [8, 7, 7]
        assert a["n_dev"] > 0 and len(a["cost_hist"]) > 0 and float(a["learner"]["eps"]) > 0
        assert int(a["learner"]["counter"]) == len(a["cost_hist"])
    else:
        assert b["launches"] == [1] * 3 and a["n_dev"] == 0


def test_gpu_ddqn_rollout_enough_turns_true_mid_episode():
    seeds = SEEDS[:8]
    a = _run(False, seeds, "train", True, 32, episodes=2)
    b = _run(True, seeds, "train", True, 32, episodes=2)
    _assert_same(a, b, "8 envs")
    # the first episode starts on one-period launches and ends on chunks; the second is all chunks
    assert 7 < b["launches"][0] < 28 and b["launches"][1] == 7, b["launches"]
    assert len(a["cost_hist"]) > 0


def test_gpu_ddqn_rollout_needs_fused_act():
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    v = VecABIDESEnv(seeds=SEEDS[:4])
    v.set_stream(stream.cuda_stream)
    task = ddqn.ExecutionTask(device="cuda")
    learner = ddqn.DDQNLearner(device="cuda", seed=5, fused_act=False)
    with pytest.raises(RuntimeError):
        ddqn.run_episode(v, learner, task, rollout=True)
    learner = ddqn.DDQNLearner(device="cuda", seed=5, fused_act=True)
    with pytest.raises(RuntimeError):
        ddqn.run_episode(v, learner, task, rollout=True, fused=False)
    v.close()
