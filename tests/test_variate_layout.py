"""The variate tables' place in the env block and in LDS (mxa_config.h MXA_VARIATE_*_MASK), computed
from the header's constants by the host compiler as test_lib_exports.py checks the layout: a
configuration outside the masks has no table bytes and the block and LDS sizes it had before the
tables existed, rmsc03 has one table per value agent between the market-data slots and the trace
and the oracle stream's table in LDS, and with both masks 0 nobody has any."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "marl-optimal-execution_amd", "csrc")

# config id -> (Layout::off_trace, lds_bytes) of the build before the tables
BEFORE = {0: (530176, 8704), 1: (637696, 20224), 2: (5991936, 37448), 3: (56576, 14336), 4: (537856, 10240),
          5: (919040, 15616), 6: (1104128, 10240), 7: (1151232, 19968), 8: (745728, 13056), 9: (29921280, 14848),
          10: (39962880, 27136), 11: (29921280, 14848), 12: (39962880, 27136), 13: (49920, 14336), 14: (56576, 14336),
          15: (548608, 10240), 16: (530176, 8704), 17: (669440, 13312)}
MASKED = {0}  # rmsc03 has both bits


def _compile(tmp_path, lines, *flags):
    src = tmp_path / "vt.cpp"
    src.write_text("\n".join(['#include "mxa_config.h"', "using namespace mxa_cfg;"] + lines + ["int main() { return 0; }"]) + "\n")
    subprocess.check_call(["g++", "-std=c++20", "-fsyntax-only", "-I", CSRC] + list(flags) + [str(src)])


def _unchanged(c):
    t, lds = BEFORE[c]
    return ['static_assert(params(%d).L.off_trace == %d && params(%d).L.off_vt == %d, "config %d: no table bytes");' % (c, t, c, t, c),
            'static_assert(lds_bytes(%d) == %d && !variate_o(%d) && !variate_agent(%d), "config %d: LDS");' % (c, lds, c, c, c)]


def test_configurations_outside_the_masks_keep_their_layout(tmp_path):
    lines = []
    for c in sorted(set(BEFORE) - MASKED):
        lines += _unchanged(c)
    _compile(tmp_path, lines)


def test_rmsc03_has_a_table_per_value_agent_and_the_oracle_table_in_lds(tmp_path):
    t, lds = BEFORE[0]
    _compile(tmp_path, [
        "constexpr MxaParams P = params(MXA_CFG_RMSC03);",
        'static_assert(variate_o(MXA_CFG_RMSC03) && variate_agent(MXA_CFG_RMSC03), "rmsc03 has both bits");',
        'static_assert(P.n_value == 10 && P.L.off_vt == %d, "the region starts where the trace did");' % t,
        'static_assert(P.L.off_trace == P.L.off_vt + 10 * MXA_VT_BYTES && P.L.off_trace % 256 == 0, "one table per value agent");',
        'static_assert(MXA_VT_BYTES == 64 * 4 * 8, "64 slots of (e, ret, cache, 0)");',
        'static_assert(AF_VT_B == 46 && AF_VT_N == 47 && AF_VT_ACC == 48 && AF_VT_ACC / 32 == AF_RS_POS / 32, '
        '"the descriptor shares the record quarter the stream state dirties");',
        'static_assert(lds_bytes(MXA_CFG_RMSC03) == %d + MXA_VT_O_BYTES && MXA_VT_O_BYTES == (2 * 64 + 2) * 8, "LDS");' % lds,
        'static_assert(lds_bytes(MXA_CFG_RMSC03) * 16 <= 160 * 1024, "16 waves per CU");'])


def test_global_switch_off_leaves_no_table_anywhere(tmp_path):
    lines = []
    for c in sorted(BEFORE):
        lines += _unchanged(c)
    _compile(tmp_path, lines, "-DMXA_VARIATE_O_MASK=0", "-DMXA_VARIATE_AGENT_MASK=0")


def test_each_mask_alone(tmp_path):
    t, lds = BEFORE[0]
    _compile(tmp_path, ['static_assert(params(0).L.off_trace == %d && lds_bytes(0) == %d + MXA_VT_O_BYTES, "O alone");' % (t, lds)],
             "-DMXA_VARIATE_AGENT_MASK=0")
    _compile(tmp_path, ['static_assert(params(0).L.off_trace == %d + 10 * MXA_VT_BYTES && lds_bytes(0) == %d, "agents alone");' % (t, lds)],
             "-DMXA_VARIATE_O_MASK=0")
