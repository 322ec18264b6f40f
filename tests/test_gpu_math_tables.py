"""Every row of csrc/glibc_math.h's three tables as the device reads it, against the host build of
the header (tests/glibc_math_cases.py, pinned to libm by tests/test_glibc_math.py).

The tables are private constants of each device unit, read with per-lane indices by the probe
kernel (and with wave-uniform ones by the engine).  One probe launch per function, its arguments
laid out so that neighbouring lanes of a wave read neighbouring rows, and over the launch all 128
rows of the function's table are read: log by 128 mantissas at two exponents, exp by
x = +-j ln2 / 128, pow (log table of its own, then exp's) by 128 bases against three exponents.
Bit for bit; the rows each launch reads are computed here from the arguments and asserted."""
import numpy as np
import pytest

import glibc_math_cases as cases

pytestmark = pytest.mark.gpu

LOG_OFF = 0x3FE6000000000000   # gm_log: row = ((bits(x) - LOG_OFF) >> 45) & 127
POW_OFF = 0x3FE6955500000000   # gm_pow's log_inline likewise
ROWS = np.arange(128, dtype=np.uint64)


@pytest.fixture(scope="module")
def L():
    import mxabides
    return mxabides.load()


@pytest.fixture(scope="module")
def gm():
    return cases.host_lib()


def _device(L, mode, x, y=None):
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.ascontiguousarray(x if y is None else y, dtype=np.float64)
    out = np.zeros(len(x))
    assert L.mxa_math_probe(0, mode, x.ctypes.data, y.ctypes.data, out.ctypes.data, len(x)) == 0
    return out


def _same(L, gm, mode, x, y=None):
    dev, ref = _device(L, mode, x, y), cases.host_eval(gm, mode, x, y)
    assert np.isfinite(ref).all() and (ref != 0).all()  # the table paths, not a special range
    bad = np.nonzero(~cases.same_bits(dev, ref))[0]
    assert len(bad) == 0, "%d of %d differ, first x=%r y=%r device %r host %r" % (
        len(bad), len(x), x[bad[0]], None if y is None else y[bad[0]], dev[bad[0]], ref[bad[0]])


def _mantissas(off, k):
    """one argument per table row, mid-row, at binary exponent offset k"""
    bits = np.uint64(off + (k << 52) + (1 << 44)) + (ROWS << np.uint64(45))
    x = bits.view(np.float64)
    assert ((((bits - np.uint64(off)) >> np.uint64(45)) & np.uint64(127)) == ROWS).all()
    return x


def test_log_reads_every_row(L, gm):
    # exponents away from gm_log's near-1 window [0.9375, 1.0648), which reads no table
    x = np.concatenate([_mantissas(LOG_OFF, -3), _mantissas(LOG_OFF, 5)])
    assert ((x < 0.9375) | (x >= 1.07)).all() and (x > 0).all() and len(x) == 256
    _same(L, gm, 0, x)


def test_exp_reads_every_row(L, gm):
    j = np.arange(129, dtype=np.float64)  # (x = 0 is below gm_exp's table range: row 0 is j = 128's)
    x = np.concatenate([j * np.log(2.0) / 128, -j[1:] * np.log(2.0) / 128])
    rows = np.rint(x * 128 / np.log(2.0)).astype(np.int64) & 127  # gm_exp: ki & 127
    assert set(rows[1:129].tolist()) == set(range(128)) and set(rows[129:].tolist()) == set(range(128))
    _same(L, gm, 1, x)


def test_pow_reads_every_row_of_its_own_table_and_exps(L, gm):
    base = _mantissas(POW_OFF, 0)
    x = np.tile(base, 3)
    y = np.repeat(np.array([3.0, 1 / 3.0, -2.5]), 128)
    # exp_inline's rows over the launch, from y * log(x) (all of them need not be hit; most are)
    rows = np.rint(y * np.log(x) * 128 / np.log(2.0)).astype(np.int64) & 127
    assert len(set(rows.tolist())) > 64
    _same(L, gm, 2, x, y)
