"""The argument families and special values csrc/glibc_math.h is pinned on, shared by the host
test against libm (tests/test_glibc_math.py) and the device test against the host build of the
very header (tests/test_gpu_parity.py): (name, mode, x, y) with mode 0 log, 1 exp, 2 pow; y is
None for log and exp.  Every array comes from a fixed seed."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "glibc_math_host.cpp")
LIB = os.path.join(ROOT, "tests", "native", "build", "libgm_host.so")


def host_lib():
    """tests/native/glibc_math_host.cpp: gm_check (the header against libm) and gm_eval (the header)"""
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++20", "-fPIC", "-shared", "-ffp-contract=off", "-fno-builtin",
                           "-I" + os.path.join(ROOT, "marl-optimal-execution_amd", "csrc"), SRC, "-o", LIB, "-lm"])
    L = ctypes.CDLL(LIB)
    L.gm_check.restype = ctypes.c_int64
    L.gm_check.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                           ctypes.POINTER(ctypes.c_int64)]
    L.gm_eval.restype = None
    L.gm_eval.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]
    return L


def host_eval(L, mode, x, y=None):
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.ascontiguousarray(x if y is None else y, dtype=np.float64)
    out = np.zeros(len(x))
    L.gm_eval(mode, x.ctypes.data, y.ctypes.data, out.ctypes.data, len(x))
    return out


def path_families(n):
    """the argument distributions of the engine's own calls (the families tests/test_glibc_math.py
    has always had, in its order and from its seeds)"""
    out = []
    rs = np.random.RandomState(0)
    u = rs.rand(n)
    out += [("log 1-u", 0, 1.0 - u, None),                       # legacy exponential: -log(1 - u)
            ("log u", 0, u, None),                               # legacy gauss: log(r2), r2 in (0, 1)
            ("log near 1", 0, 1 + (rs.rand(n) - 0.5) * 0.2, None),  # the near-1 polynomial branch
            ("log wide", 0, np.exp(rs.uniform(-700, 700, n)), None),
            ("log subnormal", 0, rs.rand(n) * 1e-310, None)]
    rs = np.random.RandomState(1)
    out += [("exp -gamma d", 1, -1.67e-12 * np.floor(rs.uniform(0, 2.4e13, n)), None),   # SMRO exp(-gamma d)
            ("exp wide", 1, rs.uniform(-750, 750, n), None),
            ("exp tiny", 1, rs.uniform(-1e-15, 1e-15, n), None)]
    rs = np.random.RandomState(2)
    d = np.floor(rs.uniform(0, 2.5e13, n))
    out += [("pow (1-kappa)^d", 2, np.full(n, 1 - 1.67e-15), d),
            ("pow (1-kappa)^2d", 2, np.full(n, 1 - 1.67e-15), 2 * d),
            ("pow x^3", 2, rs.uniform(0.05, 1, n), np.full(n, 3.0)),       # LatencyModel x ** 3
            ("pow cube root", 2, rs.rand(n) * 0.25, np.full(n, 1 / 3.0)),  # get_wake_time
            ("pow general", 2, rs.uniform(0, 10, n), rs.uniform(-50, 50, n)),
            ("pow negative base, integer y", 2, -rs.uniform(0, 10, n), np.floor(rs.uniform(-50, 50, n))),
            ("pow wide y", 2, rs.uniform(0, 3, n), rs.uniform(-3000, 3000, n))]
    return out


def edge_families(n):
    """the branches a runtime composition's parameters can reach and the path families do not:
    exp's overflow and underflow windows (gm_exp_special), pow's invalid, subnormal-base, tiny-y,
    huge-y and near-1-base paths (gm_pow_special, the log_inline / exp_inline tails), the execution
    agent's square root, and both ends of log's near-1 window"""
    rs = np.random.RandomState(3)
    sign = np.where(rs.rand(n) < 0.5, -1.0, 1.0)
    out = [("exp overflow window", 1, rs.uniform(700, 712, n), None),
           ("exp underflow window", 1, rs.uniform(-750, -700, n), None),
           ("pow negative base, non-integer y", 2, -rs.uniform(0, 10, n), rs.uniform(-50, 50, n)),
           ("pow subnormal x", 2, rs.rand(n) * 1e-310, rs.uniform(-3, 3, n)),
           ("pow square root", 2, rs.uniform(0, 1e6, n), np.full(n, 0.5)),
           ("pow tiny y", 2, rs.uniform(0, 10, n), rs.uniform(-1, 1, n) * 2.0 ** -70),
           ("pow huge y", 2, rs.uniform(0, 3, n), rs.uniform(-1, 1, n) * 2.0 ** 70),
           ("pow base 1 +- 5e-10", 2, 1 + sign * 5e-10, rs.uniform(-1e12, 1e12, n)),
           ("log around 0.9375", 0, 0.9375 + rs.uniform(-5e-13, 5e-13, n), None),
           ("log around 1.06475830078125", 0, 1.06475830078125 + rs.uniform(-5e-13, 5e-13, n), None)]
    return out


def special_values():
    """zeros, ones, infinities, NaN, the subnormal and normal limits, integers around 2^53 (pow's
    odd / even / integer test of y), the neighbours of 1, and exp's overflow, underflow and
    subnormal-result thresholds with their neighbours"""
    inf, tiny = np.inf, np.finfo(np.float64).tiny
    v = [0.0, -0.0, 1.0, -1.0, inf, -inf, np.nan, 5e-324, -5e-324,
         tiny, np.nextafter(tiny, 0.0), -tiny, np.finfo(np.float64).max, -np.finfo(np.float64).max,
         0.5, -0.5, 2.0, -2.0, 3.0, -3.0, 1 / 3.0, -1 / 3.0, 1e300, -1e300, 1e-300,
         2.0 ** 52 + 1, 2.0 ** 53, 2.0 ** 53 + 2, 2.0 ** 63, 2.0 ** 64, 2.0 ** -70, -2.0 ** -70,
         np.nextafter(1.0, 0.0), np.nextafter(1.0, 2.0),
         709.782712893384, np.nextafter(709.782712893384, inf),
         -745.1332191019411, np.nextafter(-745.1332191019411, -inf),
         -708.3964185322641]
    return np.array(v, dtype=np.float64)


def special_families():
    """the table through log and exp, and its full cross product through pow"""
    v = special_values()
    x, y = np.meshgrid(v, v, indexing="ij")
    return [("log table", 0, v, None), ("exp table", 1, v, None), ("pow grid", 2, x.ravel().copy(), y.ravel().copy())]


def same_bits(a, b):
    """element-wise: equal bit patterns, two NaNs counting as equal (as gm_check compares)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))
