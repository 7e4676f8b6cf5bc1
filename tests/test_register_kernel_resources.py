"""The batched registration kernel (nos::register_batch_kernel, csrc/assemble_register.hpp, instantiated in
csrc/nos_register.hip) neither spills nor uses scratch memory in any of its 12 instantiations — ndt6 / ndt3 x fp64 / fp32
x {no loss, exponential, Huber} (not gpu: read from the code object hipcc cross-compiled into csrc/nos_register.o)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nonlinear_optimizer_for_slam_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_every_register_kernel_is_compiled_without_spills_or_scratch():
    import kernel_resources
    obj = os.path.join(CSRC, "nos_register.o")
    assert os.path.exists(obj), "build with python __graft_entry__.py"
    kernels = [k for k in kernel_resources.kernel_resources(obj) if "register_batch_kernel<" in k["name"]]
    assert len(kernels) == 12, [k["name"][:120] for k in kernels]
    for problem in ("Ndt6Problem", "Ndt3Problem"):
        for T in ("double", "float"):
            for loss in (0, 1, 2):
                form = "register_batch_kernel<nos::%s<%s, %d>, %s, 512>" % (problem, T, loss, T)
                assert any(form in k["name"] for k in kernels), form
    bad = [(k["name"][:160], k["spill"], k["scratch"]) for k in kernels if k["spill"] != 0 or k["scratch"] != 0]
    assert not bad, bad
    # one 512-thread workgroup per problem: two waves per SIMD must fit the register file (≤ 256 VGPRs per lane)
    assert all(k["vgpr"] <= 256 for k in kernels), [(k["name"][:100], k["vgpr"]) for k in kernels]
