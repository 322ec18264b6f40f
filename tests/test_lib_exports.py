"""libmxa.so loads (no GPU needed) and exports every entry point include/mxa.h declares."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared():
    src = open(os.path.join(ROOT, "include", "mxa.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(mxa_[a-z_0-9]+)\s*\(", src)))


def test_every_declared_symbol_is_exported():
    import mxabides
    L = mxabides.load()
    names = declared()
    assert len(names) >= 18 and "mxa_config_capacities" in names
    for n in names:
        assert hasattr(L, n), n
    assert set(names) == set(mxabides._lib.EXPORTS)


def test_layout_header_is_self_consistent(tmp_path):
    """the env-block structs shared by host and kernels have the sizes the layout assumes"""
    import subprocess
    src = tmp_path / "sz.cpp"
    src.write_text("""#include "mxa_config.h"
static_assert(sizeof(EnvHdr) == 504, "EnvHdr");
static_assert(offsetof(EnvHdr, t_stop) == 496, "EnvHdr.t_stop");
static_assert(offsetof(EnvHdr, kc) == 368, "EnvHdr.kc (tests/test_gpu_hash_switch.py KC_OFF)");
static_assert(sizeof(SubRec) == 32, "SubRec");
static_assert(sizeof(BlRec) == 16, "BlRec");
static_assert(sizeof(SavedEvent) == 48, "SavedEvent");
static_assert(sizeof(SavedOrder) == 32, "SavedOrder");
static_assert(sizeof(RpEntry) == 48, "RpEntry");
static_assert(sizeof(RpHdr) == 208, "RpHdr");
static_assert(sizeof(RpOrder) == 16 && sizeof(RpLob) == 16, "replay tables");
static_assert(mxa_cfg::params(MXA_CFG_RMSC03).n_agents == 64, "rmsc03");
static_assert(mxa_cfg::params(MXA_CFG_MARKETREPLAY).n_agents == 3, "replay");
int main() { return 0; }
""")
    inc = os.path.join(ROOT, "marl-optimal-execution_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++20", "-fsyntax-only", "-I", inc, str(src)])


def test_ddqn_library_exports():
    """libmxa_ddqn.so (include/mxa_ddqn.h) loads and exports what its header declares"""
    src = open(os.path.join(ROOT, "include", "mxa_ddqn.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = sorted(set(re.findall(r"\b(mxa_[a-z_0-9]+)\s*\(", src)))
    assert names == ["mxa_ddqn_actions", "mxa_ddqn_period", "mxa_ddqn_state", "mxa_qnet_act", "mxa_qnet_forward"]
    from mxabides import ddqn
    L = ddqn.lib()
    assert L is not None, "libmxa_ddqn.so not built (build_lib.build_ddqn)"
    assert ddqn.period_lib() is L
    for n in names:
        assert hasattr(L, n), n
