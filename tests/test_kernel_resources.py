"""No kernel the solve / accumulate entry points can select spills or uses scratch memory (not gpu: read from the code
objects hipcc cross-compiled into csrc/*.o).

Round 2's one-launch kernels carried the whole single-lane LM step inlined and sat at 256 VGPRs with 4-23 spilled
registers; the step is now a noinline function called by lane 0 (nos::lm_step_lane, csrc/assemble_kernels.hpp)
whose registers are its own.  This test keeps it that way for every instantiation of the default build: ndt6 / ndt3 /
reprojection x fp64 / fp32 x {no loss, exponential, Huber}, launch-per-pass (assemble_kernel), single workgroup, resident
and streamed one-launch forms (solve_cluster_kernel), the stand-alone step kernel — and for the other translation units.
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nonlinear_optimizer_for_slam_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def core():
    import kernel_resources
    obj = os.path.join(CSRC, "nos_core.o")
    assert os.path.exists(obj), "build with python __graft_entry__.py"
    return kernel_resources.kernel_resources(obj)


def test_hot_path_kernels_have_no_spills_and_no_scratch(core):
    hot = [k for k in core if any(s in k["name"] for s in ("assemble_kernel<", "solve_cluster_kernel<",
                                                           "solve_single_block_kernel<", "lm_step_kernel<"))]
    # 3 problems x 2 element types x 3 losses of each form at least
    for form, least in (("assemble_kernel<", 18), ("solve_cluster_kernel<", 36), ("solve_single_block_kernel<", 18),
                        ("lm_step_kernel<", 2)):
        assert sum(form in k["name"] for k in hot) >= least, form
    bad = [(k["name"][:160], k["spill"], k["scratch"]) for k in hot if k["spill"] != 0 or k["scratch"] != 0]
    assert not bad, bad
    # the one-launch kernels run two waves per SIMD (one 512-thread workgroup per CU): at most 256 registers, and the
    # default streaming kernel of the headline below that ceiling (room for what the scheduler wants to keep in flight)
    headline = [k for k in hot if "solve_cluster_kernel<nos::Ndt6Problem<double, 1>, double, 512, 0, 0, 1, false, true>" in k["name"]]
    assert len(headline) == 1 and headline[0]["vgpr"] <= 248, headline


def test_default_build_is_not_bloated(core):
    """Round 2 compiled 430 kernels into this translation unit, 83 of them spilling (losing launch geometries kept
    compiled); the default build now carries the geometries that are selected somewhere."""
    assert len(core) <= 260, len(core)
    assert all(k["spill"] == 0 and k["scratch"] == 0 for k in core), [k["name"][:120] for k in core if k["spill"] or k["scratch"]]


@pytest.mark.parametrize("obj", ["nos_match.o", "nos_mapbuild.o", "nos_mapexact.o", "nos_indexed.o", "nos_pgo.o", "nos_dataset.o",
                                 "nos_comm.o"])
def test_other_translation_units_report(obj):
    import kernel_resources
    ks = kernel_resources.kernel_resources(os.path.join(CSRC, obj))
    assert ks
    spilling = [k["name"][:100] for k in ks if k["spill"] > 0]
    # known and off the hot path: the set-up kernel of the pose-graph coarse level's block cyclic reduction (6x6 blocks in
    # registers, once per solve).  The voxel-indexed kernels no longer spill (round 4).
    assert all("pgo_pcr_setup_kernel" in n for n in spilling), spilling


def _core_isa():
    """Instruction lines of nos_core.o's gfx950 code object, addresses and encodings stripped."""
    import subprocess
    import tempfile
    llvm = "/opt/rocm/lib/llvm/bin"
    obj = os.path.join(CSRC, "nos_core.o")
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "fatbin"), os.path.join(d, "co")
        subprocess.check_call([llvm + "/llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, obj])
        subprocess.check_call([llvm + "/clang-offload-bundler", "--type=o", "--input=" + fat,
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co, "--unbundle"])
        txt = subprocess.run([llvm + "/llvm-objdump", "-d", "--no-show-raw-insn", co], capture_output=True, text=True).stdout
    return [l.split("//")[0].strip() for l in txt.splitlines() if l[:1] in ("\t", " ")]


def _vgprs(operand):
    """'v12' → {12}; 'v[4:7]' → {4, 5, 6, 7}; anything else → empty."""
    import re
    m = re.fullmatch(r"v(\d+)", operand)
    if m:
        return {int(m.group(1))}
    m = re.fullmatch(r"v\[(\d+):(\d+)\]", operand)
    return set(range(int(m.group(1)), int(m.group(2)) + 1)) if m else set()


def test_raw_asm_loads_wait_inside_their_statement_and_cross_lane_reads_keep_their_distance():
    """VERDICT r3 #9 / #7a: hipcc neither counts the memory operations of an inline-asm statement nor pads hazards around
    it (cdna_hip_programming.md §5.7), and a 22 000-round soak proves one schedule, not hazard freedom.  Read off the ISA:
      * every `global_load_dwordx4 … sc1` (they only come from tagged_load's asm) is directly followed by its
        `s_waitcnt vmcnt(0)` — the destination registers are written before the statement ends, whatever follows it;
      * every 16-byte store of a one-launch kernel, write-through or plain (tagged_store / tagged_store_plain), is followed
        by `s_nop 1` (see the next test for the write-through ones);
      * no `v_permlane32_swap` / `v_permlane16_swap` / `v_readlane` / `v_readfirstlane` reads a vector register that the
        instruction DIRECTLY in front of it wrote with a VALU instruction (those come from builtins, which hipcc pads — this
        keeps an eye on it), and `s_getreg` (the XCC id probe) is not directly behind an `s_setreg`."""
    import re
    lines = _core_isa()
    loads = [i for i, l in enumerate(lines) if re.match(r"global_load_dwordx4 .* sc1", l)]
    assert len(loads) >= 36, len(loads)
    bare = [lines[i:i + 2] for i in loads if not lines[i + 1].startswith("s_waitcnt vmcnt(0)")]
    assert not bare, bare[:3]
    cross = [i for i, l in enumerate(lines) if re.match(r"v_(permlane(16|32)_swap|readlane|readfirstlane)", l)]
    assert len(cross) > 1000
    hazards = []
    for i in cross:
        prev = lines[i - 1]
        if not prev.startswith("v_") or re.match(r"v_(permlane(16|32)_swap|readlane|readfirstlane|cmp|cmpx)", prev):
            continue  # scalar / memory / nop in front, or another cross-lane instruction (they chain on disjoint registers)
        ops = [o.strip() for o in lines[i].split(None, 1)[1].split(",")]
        reads = set().union(*[_vgprs(o) for o in (ops if lines[i].startswith("v_permlane") else ops[1:])])
        wrote = _vgprs(prev.split(None, 1)[1].split(",")[0].strip())
        if reads & wrote:
            hazards.append((prev, lines[i]))
    assert not hazards, hazards[:5]
    for i, l in enumerate(lines):
        if l.startswith("s_getreg"):
            assert not lines[i - 1].startswith("s_setreg"), lines[i - 2:i + 1]


def test_inline_asm_16_byte_stores_carry_their_wait_states():
    """hipcc pads nothing around inline asm, and a 16-byte store reads its data registers up to two states after issue:
    the tagged all-reduce's `global_store_dwordx4 … sc1` statements end with `s_nop 1` inside the string
    (cdna_hip_programming.md §5.7) — without it the next instruction may overwrite the registers, which once cost four
    sums their low words.  Every write-through 16-byte store in the code object (they only come from that inline asm) must
    be followed by the nop."""
    import re
    lines = _core_isa()
    stores = [i for i, l in enumerate(lines) if re.match(r"global_store_dwordx4 .* sc1", l)]
    assert len(stores) >= 36, len(stores)  # at least one per one-launch solve kernel
    bare = [lines[i:i + 2] for i in stores if not lines[i + 1].startswith("s_nop 1")]
    assert not bare, bare[:3]
    # the plain form (stage-1 units that stay in the XCD's L2): `global_store_dwordx4 v[a:b], v[c:f], off` + nop.  The
    # compiler's own 16-byte stores in this translation unit use a scalar base (`vN, v[..], s[..]`), never `off` + a nop-less
    # neighbour: every `off` form without cache bits must carry the nop too
    plain = [i for i, l in enumerate(lines) if re.match(r"global_store_dwordx4 v\[\d+:\d+\], v\[\d+:\d+\], off$", l)]
    assert len(plain) >= 36, len(plain)
    bare = [lines[i:i + 2] for i in plain if not lines[i + 1].startswith("s_nop 1")]
    assert not bare, bare[:3]
