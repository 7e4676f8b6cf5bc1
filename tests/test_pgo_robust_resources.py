"""The robust pose-graph kernels in the compiled object (csrc/nos_pgo.o, read through tools/kernel_resources.py): each of
the five new kernels once, without spill or scratch, and every kernel the object held before them still there — the names
were recorded by the same tool into tests/golden/pgo_kernel_names_weighted.json before the robust kernels were written.
No GPU."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nonlinear_optimizer_for_slam_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))

NEW = ("nos::pgo_robust_weights_kernel(", "nos::pgo_linearize_robust_kernel(", "nos::pgo_switch_linearize_robust_kernel(",
       "nos::pgo_matvec_pose_robust_kernel(", "nos::pgo_matvec_cg_robust_kernel(")


def _kernels():
    import kernel_resources
    obj = os.path.join(CSRC, "nos_pgo.o")
    assert os.path.exists(obj), "build with python __graft_entry__.py"
    return kernel_resources.kernel_resources(obj)


def test_the_five_robust_kernels_are_compiled_once_without_spill_or_scratch():
    kernels = _kernels()
    for form in NEW:
        mine = [k for k in kernels if k["name"].startswith(form)]
        assert len(mine) == 1, (form, [k["name"][:80] for k in mine])
        print("%-45s %3d VGPRs, %d spills, %d B scratch, %d B LDS" % (form, mine[0]["vgpr"], mine[0]["spill"], mine[0]["scratch"],
                                                                    mine[0]["lds"]))
        assert mine[0]["spill"] == 0 and mine[0]["scratch"] == 0, mine[0]


def test_every_kernel_the_object_held_before_is_still_there_without_spill_or_scratch():
    recorded = json.load(open(os.path.join(ROOT, "tests", "golden", "pgo_kernel_names_weighted.json")))["kernels"]
    assert len(recorded) == 35 and sum("_weighted_kernel(" in name for name in recorded) == 4
    kernels = _kernels()
    now = [k["name"] for k in kernels]
    missing = [name for name in recorded if now.count(name) != 1]
    assert not missing, missing
    assert sorted(set(now) - set(recorded)) == sorted(k["name"] for k in kernels if k["name"].startswith(NEW))
    weighted = [k for k in kernels if "_weighted_kernel(" in k["name"]]
    assert all(k["spill"] == 0 and k["scratch"] == 0 for k in weighted), weighted
