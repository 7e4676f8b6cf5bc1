"""The batched solve kernel (nos::solve_batch_kernel, csrc/assemble_batch.hpp, instantiated in csrc/nos_batch.hip) neither
spills nor uses scratch memory in any of its 18 instantiations — ndt6 / ndt3 / reprojection x fp64 / fp32 x {no loss,
exponential, Huber} (not gpu: read from the code object hipcc cross-compiled into csrc/nos_batch.o)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nonlinear_optimizer_for_slam_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_every_batch_kernel_is_compiled_without_spills_or_scratch():
    import kernel_resources
    obj = os.path.join(CSRC, "nos_batch.o")
    assert os.path.exists(obj), "build with python __graft_entry__.py"
    batch = [k for k in kernel_resources.kernel_resources(obj) if "solve_batch_kernel<" in k["name"]]
    assert len(batch) >= 18, [k["name"][:120] for k in batch]
    for problem in ("Ndt6Problem", "Ndt3Problem", "ReprojProblem"):
        for T in ("double", "float"):
            for loss in (0, 1, 2):
                form = "solve_batch_kernel<nos::%s<%s, %d>, %s, 512>" % (problem, T, loss, T)
                assert any(form in k["name"] for k in batch), form
    bad = [(k["name"][:160], k["spill"], k["scratch"]) for k in batch if k["spill"] != 0 or k["scratch"] != 0]
    assert not bad, bad
    # one 512-thread workgroup per problem: every wave must fit the register file with room to spare (≤ 256 VGPRs per lane
    # for two waves per SIMD)
    assert all(k["vgpr"] <= 256 for k in batch), [(k["name"][:100], k["vgpr"]) for k in batch]
