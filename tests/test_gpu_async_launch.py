"""The asynchronous path of a Kernel.runner handle (include/mxa.h): mxa_set_stream, mxa_launch,
mxa_write_results and mxa_sync, as a caller drives it from a stream of its own (one launch of a
fixed pop budget at a time, the per-env (events, hash, status, current_time) rows read from device
memory to decide whether to go on).  rmsc03 x8 against the C oracle, every assertion exact."""
import numpy as np
import pytest
import torch  # before libmxa loads: one HIP runtime per process (the side stream, the result rows)

from test_gpu_partial_reset import SEEDS, assert_blocks_equal, assert_oracle, blocks, oracle

pytestmark = pytest.mark.gpu

POPS = 4096


@pytest.fixture(scope="module")
def mx():
    import mxabides
    mxabides.load()
    return mxabides


def test_gpu_launch_on_a_callers_stream(mx):
    n = len(SEEDS)
    budget = -(-max(oracle("rmsc03", sd)[0] for sd in SEEDS) // POPS) + 1
    side = torch.cuda.Stream()
    buf = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()  # buf is zeroed before another stream writes it
    m = mx.VecMarket("rmsc03", SEEDS)
    m.set_parity_hash(True)
    m.set_stream(side.cuda_stream)
    launches, rows = 0, None
    while True:
        assert launches < budget, "still running after %d launches of %d pops: %s" % (launches, POPS, rows)
        m.launch(POPS)
        m.write_results(buf.data_ptr())
        m.sync()
        launches += 1
        rows = buf.cpu().numpy()
        assert (rows[:, 0] <= launches * POPS).all(), rows[:, 0]
        if (rows[:, 2] != 0).all():
            break
    s = m.summary()
    assert (rows[:, 0] == s["events"]).all() and (rows[:, 1].view(np.uint64) == s["hash"]).all()
    assert (rows[:, 2] == s["status"]).all() and (rows[:, 3] == s["current_time"]).all()
    assert_oracle(m, "rmsc03", SEEDS)
    done = blocks(m)
    m.launch(POPS)  # nothing is running: the launch changes nothing
    m.write_results(buf.data_ptr())
    m.sync()
    assert_blocks_equal(done, blocks(m), range(n), "launch on a finished handle")
    assert (buf.cpu().numpy() == rows).all()
    # back on the handle's own stream
    m.set_stream(None)
    m.reset()
    assert (m.summary()["events"] == 0).all()
    m.run()
    assert_oracle(m, "rmsc03", SEEDS)
    assert (m.summary()["hash"] == rows[:, 1].view(np.uint64)).all()


def test_gpu_launch_refused_on_a_gymkernel_handle(mx):
    """GymKernel handles advance by mxa_step: mxa_launch (and mxa_run) are MXA_EINVAL"""
    from mxabides.gym import VecABIDESEnv
    v = VecABIDESEnv(seeds=SEEDS[:2])
    before = v.summary()
    with pytest.raises(mx.MxaError):
        v._check(v.L.mxa_launch(v._h, POPS), "mxa_launch")
    with pytest.raises(mx.MxaError):
        v._check(v.L.mxa_run(v._h, POPS, 0, None), "mxa_run")
    after = v.summary()
    assert all((before[k] == after[k]).all() for k in before)
