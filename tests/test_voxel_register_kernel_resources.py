"""The batched registration kernel on the live voxel store (nos::register_live_kernel, csrc/assemble_register_live.hpp,
instantiated in csrc/nos_voxelregister.hip) neither spills nor uses scratch memory in any of its 12 instantiations — ndt6 /
ndt3 x fp64 / fp32 x {no loss, exponential, Huber} — and stays within the 256 VGPRs per lane that two waves per SIMD (one
512-thread workgroup per problem) allow (not gpu: read from the code object hipcc cross-compiled into
csrc/nos_voxelregister.o).  The snapshot's kernel stays where it was: none of its instantiations is in the new object."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nonlinear_optimizer_for_slam_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_every_live_register_kernel_is_compiled_without_spills_or_scratch():
    import kernel_resources
    obj = os.path.join(CSRC, "nos_voxelregister.o")
    assert os.path.exists(obj), "build with python __graft_entry__.py"
    every = kernel_resources.kernel_resources(obj)
    kernels = [k for k in every if "register_live_kernel<" in k["name"]]
    assert len(kernels) == 12, [k["name"][:120] for k in kernels]
    forms = set()
    for problem in ("Ndt6Problem", "Ndt3Problem"):
        for T in ("double", "float"):
            for loss in (0, 1, 2):
                form = "register_live_kernel<nos::%s<%s, %d>, %s, 512>" % (problem, T, loss, T)
                assert sum(form in k["name"] for k in kernels) == 1, form
                forms.add(form)
    assert len(forms) == 12
    assert not [k["name"][:120] for k in every if "register_batch_kernel<" in k["name"]]
    assert all("VoxelMatchView" in k["name"] for k in kernels)  # the live store's view, not the snapshot's
    bad = [(k["name"][:160], k["spill"], k["scratch"]) for k in kernels if k["spill"] != 0 or k["scratch"] != 0]
    assert not bad, bad
    assert all(k["vgpr"] + k["agpr"] <= 256 for k in kernels), [(k["name"][:100], k["vgpr"], k["agpr"]) for k in kernels]
