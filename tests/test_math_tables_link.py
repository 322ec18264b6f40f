"""csrc/glibc_math.h's tables in position-independent device code: read pc-relatively, never
through the GOT.  As externally visible `__device__ __constant__` variables every table read was
two dependent scalar loads (the table's address from the GOT, then the entry); the header now
emits them as private constants of the unit.  A kernel that calls gm_log, gm_exp
and gm_pow is compiled to gfx950 assembly the way libmxa's units are, and no line of it may reach a
table through a gotpcrel relocation."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "marl-optimal-execution_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
TABLES = ("gm_log_tab", "gm_exp_tab", "gm_pow_tab")

UNIT = """
#include <hip/hip_runtime.h>
#include "glibc_math.h"
__global__ void k(const double* x, const double* y, double* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  out[3 * i] = gm_log(x[i]);
  out[3 * i + 1] = gm_exp(x[i]);
  out[3 * i + 2] = gm_pow(x[i], y[i]);
}
"""


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.fail("no hipcc at %s: the device compile of csrc/glibc_math.h cannot be checked" % HIPCC)
    d = tmp_path_factory.mktemp("gm_link")
    src, out = d / "gm_unit.hip", d / "gm_unit.s"
    src.write_text(UNIT)
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++20", "-ffp-contract=off", "-fno-fast-math",
                           "-fPIC", "--cuda-device-only", "-S", "-I" + CSRC, str(src), "-o", str(out)])
    return out.read_text()


def test_the_kernel_reads_all_three_tables(asm):
    """(the check below is not vacuous: the compiled kernel does name every table)"""
    for t in TABLES:
        assert re.search(r"\b\w*%s\b" % t, asm), "%s is not referenced by the compiled unit" % t


def test_no_table_is_reached_through_the_got(asm):
    bad = [l.strip() for l in asm.splitlines() if "gotpcrel" in l and any(t in l for t in TABLES)]
    assert not bad, "table reads through the GOT:\n" + "\n".join(bad[:8])


def test_tables_are_not_exported(asm):
    """a .globl table is what makes -fPIC code take its address from the GOT"""
    bad = [l.strip() for l in asm.splitlines() if re.match(r"\s*\.globl\s", l) and any(t in l for t in TABLES)]
    assert not bad, "\n".join(bad)
