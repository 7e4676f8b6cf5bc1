"""Are the matcher, registration, batched-solve and score kernels of two source trees the same kernels?  Compares gfx950 assembly as TEXT.

usage: python tools/compare_kernel_asm.py OLD_CSRC NEW_CSRC [--jobs N] [--units a,b,...] [--all-kernels]
                                                                               (the table goes to stdout)

Every unit that holds one of those kernels (UNITS) is compiled from both csrc directories with the Makefile's
flags and `-S --cuda-device-only`; the body of each kernel named in KERNELS — from its label to its s_endpgm — is looked up
by demangled name and compared line for line.  Two things are normalised, both of them numbering, not code: the index of
the function inside its unit in local labels (.LBB12_3 → .LBB_3: a kernel that moved from a .hip file into a header is
emitted at another position) and trailing comments.  Exit status 1 when a body differs or a kernel is missing.
--units replaces UNITS (names without .hip); --all-kernels compares every kernel the units emit — every .amdhsa_kernel,
rocPRIM's instantiations included — instead of those of KERNELS.
"""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall"]  # HIPFLAGS of csrc/Makefile
UNITS = ("nos_match", "nos_indexed", "nos_voxelmap", "nos_register", "nos_voxelregister", "nos_batch", "nos_score")
KERNELS = ("match_kernel<", "voxel_match_kernel<", "match_index_kernel(", "voxel_match_index_kernel(", "voxel_rank_ids_kernel(",
           "register_batch_kernel<", "register_live_kernel<", "solve_batch_kernel<", "score_batch_kernel<", "score_finish_kernel(")


def assembly(csrc, unit, out_dir):
    out = os.path.join(out_dir, unit + ".s")
    subprocess.run([HIPCC] + FLAGS + ["-S", "--cuda-device-only", "-o", out, os.path.join(csrc, unit + ".hip")],
                   check=True, stderr=subprocess.DEVNULL)
    with open(out) as f:
        return f.read()


def kernel_bodies(text, every=False):
    """→ {demangled name: [normalised lines from the kernel's label to s_endpgm]} for the kernels of KERNELS (every: for
    each symbol the unit declares a kernel)."""
    lines = text.split("\n")
    entry_points = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
    starts = [(i, m.group(1)) for i, line in enumerate(lines) for m in [re.match(r"^(_Z\w+):", line)] if m]
    names = subprocess.run(["c++filt"], input="\n".join(s for _, s in starts), capture_output=True, text=True).stdout.split("\n")
    bodies = {}
    for (i, symbol), name in zip(starts, names):
        name = re.sub(r"^void ", "", name.strip())
        # the function's own name, not a type among its arguments: "nos::match_kernel<" must not match voxel_match_kernel
        if not (symbol in entry_points if every else any(re.search(r"(^|::)" + re.escape(k), name) for k in KERNELS)):
            continue
        body = []
        for line in lines[i + 1:]:
            line = re.sub(r"\s*;.*$", "", line)
            line = re.sub(r"\.LBB\d+_", ".LBB_", line)
            if line.strip():
                body.append(line)
            if line.strip() == "s_endpgm":
                break
        bodies[name] = body
    return bodies


def main():
    old_csrc, new_csrc = sys.argv[1], sys.argv[2]
    jobs = int(sys.argv[sys.argv.index("--jobs") + 1]) if "--jobs" in sys.argv else 4
    units = tuple(sys.argv[sys.argv.index("--units") + 1].split(",")) if "--units" in sys.argv else UNITS
    every = "--all-kernels" in sys.argv
    with tempfile.TemporaryDirectory() as d:
        dirs = {"old": os.path.join(d, "old"), "new": os.path.join(d, "new")}
        for p in dirs.values():
            os.mkdir(p)
        with ThreadPoolExecutor(jobs) as pool:
            work = {(side, u): pool.submit(assembly, csrc, u, dirs[side])
                    for side, csrc in (("old", old_csrc), ("new", new_csrc)) for u in units}
            text = {k: f.result() for k, f in work.items()}
    bad = 0
    print("%-18s %6s %6s %-9s %s" % ("unit", "old", "new", "identical", "kernel"))
    for u in units:
        old, new = kernel_bodies(text[("old", u)], every), kernel_bodies(text[("new", u)], every)
        for name in sorted(set(old) | set(new)):
            a, b = old.get(name), new.get(name)
            same = a is not None and a == b
            bad += not same
            print("%-18s %6s %6s %-9s %s" % (u, len(a) if a is not None else "-", len(b) if b is not None else "-",
                                            "yes" if same else "NO", name))
    print("%d kernel(s) differ or are missing on one side" % bad if bad else "every kernel body is identical")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
