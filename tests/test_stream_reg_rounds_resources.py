"""The streamed one-launch kernels keep rounds of the dataset in vector registers (StreamRegRounds,
csrc/assemble_one_launch.hpp).  They run two waves per SIMD, which allows 256 registers per lane: every streamed
instantiation must stay within that without spilling and without scratch, and there are as many of them as before the
register rounds — the slot count is a trait of the instantiation, not a template parameter (not gpu: read from the code
object hipcc cross-compiled into csrc/nos_core.o).
"""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nonlinear_optimizer_for_slam_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))

# 3 problems x 2 element types x 3 losses x {default, non-temporal loads}: the streamed kernels of the build before this one
STREAMED_KERNELS = 36
_STREAMED = re.compile(r"solve_cluster_kernel<nos::\w+<\w+, \d+>, \w+, 512, 0, 0, [1-9]\d*, ")


@pytest.fixture(scope="module")
def streamed():
    import kernel_resources
    obj = os.path.join(CSRC, "nos_core.o")
    assert os.path.exists(obj), "build with python __graft_entry__.py"
    return [k for k in kernel_resources.kernel_resources(obj) if _STREAMED.search(k["name"])]


def test_streamed_kernels_fit_the_register_file(streamed):
    assert streamed
    bad = [(k["name"][:150], k["vgpr"], k["agpr"], k["spill"], k["scratch"]) for k in streamed
           if k["vgpr"] + k["agpr"] > 256 or k["vgpr"] > 256 or k["spill"] != 0 or k["scratch"] != 0]
    assert not bad, bad


def test_no_new_instantiations(streamed):
    assert len(streamed) == STREAMED_KERNELS, sorted(k["name"][:150] for k in streamed)
