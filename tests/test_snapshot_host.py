"""The host arithmetic of the env-state snapshots (csrc/mxa_snapshot.h: slot sizes and the map
checks of mxa_snapshot_save / mxa_snapshot_restore) as a stand-alone CPU program under
AddressSanitizer and UBSan: plain C++ with no HIP types, so no GPU and no libmxa is involved.  And
what include/mxa_snap.h declares against libmxa.so's exports and the ctypes binding table."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "mxa_snapshot.h"
#include <cstdio>
#include <cstring>
#include <vector>
using namespace mxa_snap;
static int fails = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); fails++; } } while (0)
static bool says(const char* r, const char* what) { return r && std::strstr(r, what); }
int main() {
  // heap arrays of the exact length: a read past either end is the sanitizer's to report
  std::vector<uint8_t> none(4, 0), all(4, 1), some = {1, 0, 1, 0};
  {  // maps with -1
    std::vector<int32_t> m = {0, -1, 2, -1};
    CHECK(check_map(m.data(), 4, 4, true, none.data()) == nullptr);
    CHECK(check_map(m.data(), 4, 4, false, some.data()) == nullptr);
    CHECK(says(check_map(m.data(), 4, 4, false, none.data()), "never saved"));
    std::vector<int32_t> off(4, -1);  // nobody takes part
    CHECK(check_map(off.data(), 4, 1, true, none.data()) == nullptr);
    CHECK(check_map(off.data(), 4, 1, false, none.data()) == nullptr);
  }
  {  // out of range at both ends
    std::vector<int32_t> lo = {0, -2, 1, 2}, hi = {0, 1, 2, 4}, top = {3, 2, 1, 0};
    CHECK(says(check_map(lo.data(), 4, 4, true, none.data()), "outside"));
    CHECK(says(check_map(lo.data(), 4, 4, false, all.data()), "outside"));
    CHECK(says(check_map(hi.data(), 4, 4, true, none.data()), "outside"));
    CHECK(says(check_map(hi.data(), 4, 4, false, all.data()), "outside"));
    CHECK(check_map(top.data(), 4, 4, true, none.data()) == nullptr);  // n_slots - 1 is the last slot
    std::vector<int32_t> one = {-1, 1, -1, 0};
    std::vector<uint8_t> f2(2, 1);
    CHECK(check_map(one.data(), 4, 2, false, f2.data()) == nullptr);
    one[1] = 2;
    CHECK(says(check_map(one.data(), 4, 2, false, f2.data()), "outside"));
  }
  {  // a duplicate save target is refused; the same map restores (a fork)
    std::vector<int32_t> dup = {1, -1, 1, 0};
    std::vector<uint8_t> f2(2, 1);
    CHECK(says(check_map(dup.data(), 4, 2, true, f2.data()), "two envs"));
    CHECK(check_map(dup.data(), 4, 2, false, f2.data()) == nullptr);
    std::vector<int32_t> fork(4, 0);
    std::vector<uint8_t> f1(1, 1), e1(1, 0);
    CHECK(check_map(fork.data(), 4, 1, false, f1.data()) == nullptr);
    CHECK(says(check_map(fork.data(), 4, 1, false, e1.data()), "never saved"));
    CHECK(says(check_map(fork.data(), 4, 1, true, e1.data()), "two envs"));
  }
  {  // the identity map
    std::vector<uint8_t> f3(3, 1), f5 = {1, 1, 1, 0, 1};
    CHECK(says(check_map(nullptr, 4, 3, true, f3.data()), "n_slots >= n_envs"));
    CHECK(says(check_map(nullptr, 4, 3, false, f3.data()), "n_slots >= n_envs"));
    CHECK(check_map(nullptr, 4, 4, true, none.data()) == nullptr);
    CHECK(check_map(nullptr, 4, 4, false, all.data()) == nullptr);
    CHECK(says(check_map(nullptr, 4, 5, false, f5.data()), "never saved"));  // slot 3 is env 3's
    f5[3] = 1; f5[4] = 0;
    CHECK(check_map(nullptr, 4, 5, false, f5.data()) == nullptr);            // slot 4 is nobody's
  }
  CHECK(check_map(nullptr, 0, 4, true, none.data()) != nullptr);
  CHECK(check_map(nullptr, 4, 0, true, none.data()) != nullptr);
  CHECK(check_map(nullptr, 4, 4, true, nullptr) != nullptr);
  // slot sizes: the block, the 256-byte trailer, the log rows rounded up to 256 bytes
  CHECK(slot_bytes(256, 0) == 512);
  CHECK(slot_bytes(70400, 0) == 70400 + 256);
  CHECK(slot_bytes(70400, 1) == 70400 + 256 + 256);
  CHECK(slot_bytes(70400, 16) == 70400 + 256 + 256);
  CHECK(slot_bytes(70400, 17) == 70400 + 256 + 512);
  CHECK(slot_bytes(70400, 1 << 20) == 70400 + 256 + ((int64_t)16 << 20));
  CHECK(slot_bytes(70400, 2147483647) == 70400 + 256 + 34359738368ll);  // 64-bit: 2^31 - 1 records
  CHECK(log_offset(70400) == 70656 && log_offset(70400) % 256 == 0);
  CHECK(stride_ok(256) && stride_ok(70400) && !stride_ok(0) && !stride_ok(70400 + 16) && !stride_ok(-256));
  // the records a slot carries: max of the run's and the kernelStopping pass's, capped
  CHECK(log_count(5, 0, 100) == 5 && log_count(5, 9, 100) == 9 && log_count(120, 0, 100) == 100);
  CHECK(log_count(0, 0, 100) == 0 && log_count(7, 7, 0) == 0 && log_count(-1, -3, 100) == 0);
  // the grid: workgroups of 256 lanes x 16 bytes x loads cover the bytes, the last one partly
  CHECK(wg_bytes(4) == 16384 && wg_bytes(8) == 32768);
  CHECK(wg_count(0, 4) == 0 && wg_count(256, 4) == 1 && wg_count(16384, 4) == 1 && wg_count(16640, 4) == 2);
  CHECK(wg_count((int64_t)16 << 20, 4) == 1024 && wg_count((int64_t)16 << 20, 8) == 512);
  if (fails) return 1;
  std::printf("snapshot host checks ok\n");
  return 0;
}
"""


def test_snapshot_host_arithmetic_under_sanitizers(tmp_path):
    src = tmp_path / "snapshot_host.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "snapshot_host"
    inc = os.path.join(ROOT, "marl-optimal-execution_amd", "csrc")
    # the runtimes linked into the program: it runs whatever else the environment preloads
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan",
                           "-static-libubsan", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", "-I", inc, str(src), "-o",
                           str(exe)])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "snapshot host checks ok" in r.stdout, r.stdout


def test_snapshot_exports_are_declared_bound_and_refuse_null():
    """include/mxa_snap.h (the part of the C-ABI that include/mxa.h includes): libmxa.so exports
    every name it declares, mxabides._lib.SNAPSHOT_BINDINGS binds exactly those, and each answers a
    null handle or snapshot with MXA_EINVAL before it reaches HIP (no GPU needed)"""
    import ctypes
    import re

    import numpy as np

    import mxabides
    from mxabides import _lib
    main = open(os.path.join(ROOT, "include", "mxa.h")).read()
    assert '#include "mxa_snap.h"' in main
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mxa_snap.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(mxa_[a-z_0-9]+)\s*\(", src)))
    assert names == ["mxa_snapshot_create", "mxa_snapshot_destroy", "mxa_snapshot_info", "mxa_snapshot_restore",
                     "mxa_snapshot_save"]
    assert set(names) == set(_lib.SNAPSHOT_BINDINGS) and not set(names) & set(_lib.EXPORTS)
    L = mxabides.load()
    for n in names:
        assert hasattr(L, n) and getattr(L, n).argtypes == _lib.SNAPSHOT_BINDINGS[n][0], n
    EINVAL = -1
    out, o4 = ctypes.c_void_p(), np.zeros(4, dtype=np.int64)
    assert L.mxa_snapshot_create(None, 4, ctypes.byref(out)) == EINVAL and not out
    assert L.mxa_snapshot_save(None, None, None) == EINVAL
    assert L.mxa_snapshot_restore(None, None, None) == EINVAL
    assert L.mxa_snapshot_info(None, o4.ctypes.data) == EINVAL
    assert L.mxa_snapshot_destroy(None) is None
