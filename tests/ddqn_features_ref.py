"""The plain reference of a state of N features (include/mxa_state_spec.h), shared by
tests/test_ddqn_features.py (CPU) and the GPU tests of the feature kernels: numpy float64, one
rounding per operation, true divisions, np.digitize per feature. Nothing here comes from the code
under test. A feature is a plain tuple (col, splits, mul, div, add); `to_features` turns a list of
them into mxabides.ddqn.Feature objects for the code under test.

Also the feature sets of the tests (F = 1, 2, 6, 8 on observation rows of 9 columns) and
observation rows made of their edge values: every split point of the features whose transform is the
identity (mul 1, div 1, add 0, so the value lands exactly on the point), the doubles next to it on
both sides, values below the first and above the last point, -0.0, +-inf, NaN, and for the time and
quantity columns every horizon step and the quantities at which a reciprocal would land one bin off."""
import numpy as np

OBS_W = 9
NH, Q0 = 27, 100000.0


def uniform(low, high, bins):
    """agent/execution/util.py:5-22 for one dimension: the interior split points"""
    return np.linspace(low, high, bins + 1)[1:-1]


TIME = (0, uniform(0.0, 1.0, 200), 2.0, float(NH), -1.0)
QTY = (1, uniform(0.0, 1.0, 200), 2.0, Q0, -1.0)
SPREAD = (3, uniform(0.0, 50.0, 10), 1.0, 1.0, 0.0)               # identity transform: values land on the points
IMBALANCE = (4, uniform(0.0, 1.0, 8), 1.0, 1.0, 0.0)
LOG_RETURN = (2, np.zeros(0), 1e4, 1.0, 0.0)                      # passed through, in basis points
VOLATILITY = (6, np.array([1e-6, 1e-5, 1e-4, 1e-3, 0.5]), 1.0, 3.0, 0.0)  # a division that is not by 1
DIRECTION = (7, np.array([-0.5, 0.5]), 1.0, 1.0, 0.0)
EFF_SPREAD = (8, np.zeros(0), 0.5, 7.0, 0.25)                     # passed through after a real division
IRREGULAR = (3, np.array([-0.9, -0.5, -0.25, -0.1, 0.0, 0.3, 0.99]), 1.0, 1.0, 0.0)
FEATURE_SETS = {1: [IRREGULAR], 2: [TIME, QTY], 6: [TIME, QTY, SPREAD, IMBALANCE, LOG_RETURN, VOLATILITY],
                8: [TIME, QTY, SPREAD, IMBALANCE, LOG_RETURN, VOLATILITY, DIRECTION, EFF_SPREAD]}


def to_features(feats):
    from mxabides import ddqn
    return [ddqn.Feature(col, splits=splits if len(splits) else None, mul=mul, div=div, add=add)
            for col, splits, mul, div, add in feats]


def state_ref(obs, feats):
    """[n, F] float32: per feature np.digitize(mul * (obs[:, col] / div) + add, splits), or the value
    itself cast to float32 where the feature has no split points"""
    obs = np.asarray(obs, dtype=np.float64)
    out = np.zeros((len(obs), len(feats)), dtype=np.float32)
    with np.errstate(all="ignore"):
        for f, (col, splits, mul, div, add) in enumerate(feats):
            x = np.float64(mul) * (obs[:, col] / np.float64(div)) + np.float64(add)
            splits = np.asarray(splits, dtype=np.float64)
            out[:, f] = np.digitize(x, splits).astype(np.float32) if len(splits) else x.astype(np.float32)
    return out


def same_state(a, b):
    """exact equality of two float32 state arrays: shape, every value and the sign of every zero; a
    NaN equals a NaN (a passed-through NaN's payload is the platform's)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != np.float32 or b.dtype != np.float32 or a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan], b[~nan])
                and np.array_equal(np.signbit(a[~nan]), np.signbit(b[~nan])))


SPECIALS = [-0.0, 0.0, np.inf, -np.inf, np.nan, -1e300, 1e300, 5e-324]


def edge_pool(col, feats):
    """the edge values of observation column `col` under the feature set"""
    pool = list(SPECIALS)
    if col == 0:
        pool += list(range(0, NH + 1)) + [-1.0, NH + 1.0, 13.5]
    elif col == 1:
        # multiples of 250 from 50250 up: where 2 * (q * (1 / q0)) - 1 lands one bin above the true division
        pool += list(range(50250, 100001, 250)) + [0.0, 1.0, 249.0, 250.0, 499.0, 500.0, 99999.0, 100001.0, -1.0]
    for c, splits, mul, div, add in feats:
        if c != col or not len(splits):
            continue
        pts = np.asarray(splits, dtype=np.float64) * div if (mul, add) == (1.0, 0.0) else np.zeros(0)
        for p in pts:  # on the point (exactly, when div is 1), and the doubles on both sides
            pool += [p, np.nextafter(p, -np.inf), np.nextafter(p, np.inf)]
        if len(pts):
            pool += [pts[0] - 1.0, pts[-1] + 1.0]
    return np.array(pool, dtype=np.float64)


def edge_obs(n, feats, seed=0):
    """[n, 9] float64 observation rows: two thirds of every column's entries walk through the column's
    edge pool (different columns out of step), the rest are random"""
    rs = np.random.RandomState(seed)
    obs = rs.rand(n, OBS_W) * 2.0 - 0.5
    obs[:, 0] = rs.randint(0, NH + 1, n)
    obs[:, 1] = rs.randint(0, int(Q0) + 1, n)
    obs[:, 3] = rs.rand(n) * 60.0 - 5.0
    i = np.arange(n)
    for c in range(OBS_W):
        pool = edge_pool(c, feats)
        take = (i + c) % 3 != 0
        obs[take, c] = pool[(np.arange(int(take.sum())) + 5 * c) % len(pool)]
    return obs


def pool_rows(feats):
    """the number of rows after which edge_obs has walked through every column's whole pool"""
    return 3 * max(len(edge_pool(c, feats)) for c in range(OBS_W)) // 2 + 3
