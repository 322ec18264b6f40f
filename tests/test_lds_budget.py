"""Every built-in configuration's LDS block (mxa_cfg::lds_bytes: queue, header, hot records, the
four RNG stream windows, latency row, replay header, LDS book arrays, push scratch) fits the waves
its run kernel is compiled for (Shape::waves per SIMD, four SIMDs) in the CU's 160 KB.  Computed
from mxa_config.h's constants by the host compiler, as test_lib_exports.py checks the layout."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "marl-optimal-execution_amd", "csrc")
CU_LDS = 160 * 1024


def test_lds_bytes_fit_the_waves_per_cu(tmp_path):
    ids = re.search(r"#define\s+MXA_CONFIGS\(X\)((?:\s+X\(\d+\))+)", open(os.path.join(CSRC, "mxa_entry.h")).read()).group(1)
    n = len(re.findall(r"X\((\d+)\)", ids))  # the built-in configurations are ids 0 .. n - 1
    assert n >= 18
    lines = ['#include "mxa_config.h"',
             "constexpr size_t cu_bytes(int c) { return mxa_cfg::lds_bytes(c) * mxa_cfg::shape(c).waves * 4; }"]
    lines += ['static_assert(cu_bytes(%d) <= %d, "config %d: lds_bytes x waves per CU");' % (c, CU_LDS, c) for c in range(n)]
    # rmsc03 and rmsc03_rl: 16 waves per CU (rmsc03_rl's fill the 160 KB exactly)
    lines += ["static_assert(mxa_cfg::lds_bytes(MXA_CFG_RMSC03) * 16 <= %d && mxa_cfg::lds_bytes(MXA_CFG_RMSC03_RL) * 16 <= %d, "
              "\"16 waves per CU\");" % (CU_LDS, CU_LDS),
              "int main() { return 0; }"]
    src = tmp_path / "lds.cpp"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call(["g++", "-std=c++20", "-fsyntax-only", "-I", CSRC, str(src)])
