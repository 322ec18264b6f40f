"""Book depth without a GPU (include/mxa_depth.h): what the header declares against libmxa.so's exports
and the ctypes binding table; the host helpers of csrc/mxa_depth_kernels.h (the argument check, the
output sizes, the grid arithmetic) as a stand-alone CPU program under AddressSanitizer and UBSan (plain
C++ with no HIP types, so neither a GPU nor libmxa is involved); and the tests' own reference,
depth_util.depth_ref, on handmade sides."""
import os
import subprocess

import numpy as np

from depth_util import depth_ref, refs_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "mxa_depth_kernels.h"
#include <cstdio>
#include <cstring>
using namespace mxa_depth;
static int fails = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); fails++; } } while (0)
static bool says(const char* r, const char* what) { return r && std::strstr(r, what); }
int main() {
  // the argument check: handle, then levels, then the array
  CHECK(check_args(true, true, 1) == nullptr);
  CHECK(check_args(true, true, 10) == nullptr);
  CHECK(check_args(true, true, 1 << 20) == nullptr);
  CHECK(says(check_args(true, true, 0), "levels < 1"));
  CHECK(says(check_args(true, true, -1), "levels < 1"));
  CHECK(says(check_args(true, true, -2147483647 - 1), "levels < 1"));
  CHECK(says(check_args(true, true, (1 << 20) + 1), "levels > 1 << 20"));
  CHECK(says(check_args(true, true, 2147483647), "levels > 1 << 20"));
  CHECK(says(check_args(true, false, 10), "null depth"));
  CHECK(says(check_args(false, true, 10), "null handle"));
  CHECK(says(check_args(false, false, 0), "null handle"));
  CHECK(says(check_args(true, false, 0), "levels < 1"));
  CHECK(MAX_LEVELS == 1 << 20);
  // the output sizes in 64 bits
  CHECK(ROW_BYTES == 16);
  CHECK(rows(1, 1) == 2 && depth_bytes(1, 1) == 32 && counts_bytes(1) == 8);
  CHECK(depth_bytes(8, 10) == 8 * 2 * 10 * 16 && counts_bytes(8) == 64);
  CHECK(depth_bytes(4096, 64) == 8388608);
  CHECK(rows(65536, 1 << 20) == (int64_t)1 << 37);
  CHECK(depth_bytes(65536, 1 << 20) == (int64_t)1 << 41);  // 2 TiB: no 32-bit wrap
  CHECK(depth_bytes(2147483647, 1 << 20) == (int64_t)2147483647 * 2 * 16 * (1 << 20));
  CHECK(counts_bytes(2147483647) == (int64_t)2147483647 * 8);
  CHECK(row_of(0, 0, 10) == 0 && row_of(0, 1, 10) == 10 && row_of(3, 1, 10) == 70);
  CHECK(row_of(65535, 1, 1 << 20) == ((int64_t)65535 * 2 + 1) << 20);
  CHECK(row_of(65535, 1, 1 << 20) + (1 << 20) == rows(65536, 1 << 20));  // the last side ends the array
  // the grid: envs in blockIdx.y, grid-strided above 65,535
  CHECK(grid_y(0) == 0 && grid_y(-3) == 0 && grid_y(1) == 1 && grid_y(5) == 5 && grid_y(8) == 8);
  CHECK(grid_y(65535) == 65535 && grid_y(65536) == 65535 && grid_y((int64_t)1 << 31) == 65535);
  CHECK(envs_of_block(8, 0) == 1 && envs_of_block(8, 7) == 1 && envs_of_block(8, 8) == 0);
  CHECK(envs_of_block(65536, 0) == 2 && envs_of_block(65536, 1) == 1 && envs_of_block(65536, 65534) == 1);
  CHECK(envs_of_block(0, 0) == 0);
  {  // every env is walked by exactly one block
    const int64_t ns[] = {1, 5, 8, 65535, 65536, 65537, 131070, 200000};
    for (int64_t n : ns) {
      int64_t total = 0;
      for (int y = 0; y < grid_y(n); y++) total += envs_of_block(n, y);
      CHECK(total == n);
    }
  }
  // the slot kernel's shape: 64 lanes, up to 16 slots a lane, 8 bytes of LDS a slot
  CHECK(WAVE == 64 && MAX_OCAP == 1024 && MAX_OCAP * 8 == 8192);
  CHECK(slots_per_lane(64) == 1 && slots_per_lane(65) == 2 && slots_per_lane(448) == 7 && slots_per_lane(832) == 13);
  CHECK(slots_per_lane(1024) == 16 && slots_per_lane(1) == 1);
  CHECK(ocap_ok(64) && ocap_ok(1024) && !ocap_ok(1025) && !ocap_ok(0) && !ocap_ok(-64));
  for (int oc = 1; oc <= MAX_OCAP; oc++) CHECK(slots_per_lane(oc) * WAVE >= oc && slots_per_lane(oc) * WAVE <= MAX_OCAP);
  // the ladder kernel's round trip: 4 strides of 64 levels
  CHECK(STRIDES == 4 && round_levels() == 256);
  if (fails) return 1;
  std::printf("depth host checks ok\n");
  return 0;
}
"""


def test_depth_host_arithmetic_under_sanitizers(tmp_path):
    src = tmp_path / "depth_host.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "depth_host"
    inc = os.path.join(ROOT, "marl-optimal-execution_amd", "csrc")
    # the runtimes linked into the program: it runs whatever else the environment preloads
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan",
                           "-static-libubsan", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", "-I", inc, str(src), "-o",
                           str(exe)])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "depth host checks ok" in r.stdout, r.stdout


def test_depth_exports_are_declared_bound_and_refuse_null():
    """include/mxa_depth.h (a part of the C-ABI that include/mxa.h includes): libmxa.so exports the
    two names it declares, mxabides._lib.DEPTH_BINDINGS binds exactly those, and each answers a null
    handle with MXA_EINVAL before it reaches HIP (no GPU needed)"""
    import re

    import mxabides
    from mxabides import _lib
    main = open(os.path.join(ROOT, "include", "mxa.h")).read()
    assert '#include "mxa_depth.h"' in main
    text = open(os.path.join(ROOT, "include", "mxa_depth.h")).read()
    assert "OrderBook.py:377-398" in text
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = sorted(set(re.findall(r"\b(mxa_[a-z_0-9]+)\s*\(", src)))
    assert names == ["mxa_read_depth", "mxa_write_depth"]
    assert set(names) == set(_lib.DEPTH_BINDINGS)
    assert not set(names) & set(_lib.EXPORTS) and not set(names) & set(_lib.SNAPSHOT_BINDINGS)
    P, I32 = _lib._P, _lib._I32
    for n in names:
        assert _lib.DEPTH_BINDINGS[n] == ([P, I32, P, P], I32), n
    L = mxabides.load()
    for n in names:
        f = getattr(L, n)
        assert f.argtypes == _lib.DEPTH_BINDINGS[n][0] and f.restype is _lib.DEPTH_BINDINGS[n][1], n
    EINVAL = -1
    rows, counts = np.zeros((1, 2, 4, 2), dtype=np.int64), np.zeros((1, 2), dtype=np.int32)
    assert L.mxa_write_depth(None, 4, rows.ctypes.data, counts.ctypes.data) == EINVAL
    assert L.mxa_read_depth(None, 4, rows.ctypes.data, counts.ctypes.data) == EINVAL
    assert b"null handle" in L.mxa_last_error(None)
    assert not rows.any() and not counts.any()
    from mxabides.gym import VecABIDESEnv
    from mxabides.handle import Handle
    for cls in (mxabides.VecMarket, VecABIDESEnv):  # both handle classes inherit the three methods
        for meth in ("write_depth", "depth", "inside"):
            assert getattr(cls, meth) is getattr(Handle, meth), (cls, meth)


def _side(levels):
    """[(price, [quantities])] -> a side as Handle.book() returns it"""
    oid = iter(range(1, 1000))
    return [[[next(oid), 3, q, p] for q in qs] for p, qs in levels]


def test_depth_ref_on_handmade_sides():
    rows, n = depth_ref([], 3)
    assert n == 0 and rows.shape == (3, 2) and rows.dtype == np.int64 and not rows.any()
    one = _side([(100250, [100, 7, 43])])  # one level of three orders
    for k in (1, 2, 5):
        rows, n = depth_ref(one, k)
        assert n == 1 and rows[0].tolist() == [100250, 150] and not rows[1:].any()
    bids = _side([(100, [5]), (99, [1, 2]), (90, [10, 20, 30]), (7, [4])])
    full = [[100, 5], [99, 3], [90, 60], [7, 4]]
    for k, want_n in ((1, 1), (3, 3), (4, 4), (5, 4), (64, 4)):  # k below, at and above the level count
        rows, n = depth_ref(bids, k)
        assert n == want_n and rows[:n].tolist() == full[:n] and not rows[n:].any() and len(rows) == k
    big = _side([(1000, [2147483646] * 3)])  # the `fills` tape's level: 6,442,450,938 shares in three orders
    rows, n = depth_ref(big, 2)
    assert n == 1 and int(rows[0, 1]) == 6442450938 > 1 << 32 and rows[0, 0] == 1000
    r, c = refs_of([(bids, one), ([], big)], 3)
    assert r.shape == (2, 2, 3, 2) and c.dtype == np.int32 and c.tolist() == [[3, 1], [0, 1]]
    assert r[0, 0].tolist() == full[:3] and r[1, 1, 0].tolist() == [1000, 6442450938] and not r[1, 0].any()
