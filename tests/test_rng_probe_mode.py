"""mxa_rng_probe checks its `mode` with its other arguments, before it touches a device."""
import numpy as np

from mxabides import _lib

EINVAL = -1


def test_rng_probe_checks_mode_before_the_device():
    """an out-of-range mode is MXA_EINVAL whether or not the machine has a device (checked after
    hipSetDevice it would be MXA_EHIP on a machine without one)"""
    L = _lib.load()
    o = np.zeros(8)
    assert L.mxa_rng_probe(0, 1, 6, 0.0, 1.0, 8, o.ctypes.data) == EINVAL
    assert L.mxa_rng_probe(0, 1, -1, 0.0, 1.0, 8, o.ctypes.data) == EINVAL
