#!/usr/bin/env python3
"""Is the device code of this tree the same as that of OTHER_TREE?  (CPU: compiles and diffs, reads nothing from a GPU.)

    python tools/device_code_diff.py OTHER_TREE [--jobs N] [--src svdd_nets.hip ...]

Every source of svdd_amd/csrc/Makefile's SRCS is compiled in both trees with that tree's own Makefile flags plus
--cuda-device-only --no-gpu-bundle-output, and the two code objects are compared by their disassembly (llvm-objdump -d) and
their notes (llvm-readelf --notes: VGPRs, LDS and scratch bytes of every kernel). The line that prints the file name is dropped.
Raw bytes are NOT compared: the object embeds an identifier that changes with the output path. Exit status 0 = identical."""
import argparse
import concurrent.futures
import difflib
import os
import re
import shlex
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")


def sources(tree):
    csrc = os.path.join(tree, "svdd_amd", "csrc")
    db = subprocess.run(["make", "-C", csrc, "-pnq"], capture_output=True, text=True).stdout
    return re.search(r"^SRCS = (.*)$", db, re.M).group(1).split()


def compile_cmd(tree, src, out):
    """The Makefile's own compile line for `src` (make -n), made device-only and sent to `out`."""
    csrc = os.path.join(tree, "svdd_amd", "csrc")
    obj = src[:-len(".hip")] + ".o"
    lines = subprocess.run(["make", "-C", csrc, "--no-print-directory", "-B", "-n", obj], capture_output=True, text=True, check=True).stdout
    cmd = shlex.split([ln for ln in lines.splitlines() if src in ln][-1])
    cmd[cmd.index("-o") + 1] = out
    return cmd + ["--cuda-device-only", "--no-gpu-bundle-output"]


def listing(tree, src, tmp, tag):
    out = os.path.join(tmp, f"{tag}_{src}.co")
    subprocess.run(compile_cmd(tree, src, out), cwd=os.path.join(tree, "svdd_amd", "csrc"), check=True, capture_output=True)
    text = []
    for tool in (["llvm-objdump", "-d"], ["llvm-readelf", "--notes"]):
        got = subprocess.run([os.path.join(LLVM, tool[0])] + tool[1:] + [out], capture_output=True, text=True, check=True).stdout
        text += [ln for ln in got.splitlines() if out not in ln]
    return text


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("other_tree")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--src", action="append", help="only this source (may be repeated)")
    a = ap.parse_args()
    other = os.path.abspath(a.other_tree)
    srcs = sources(HERE)
    if sources(other) != srcs:
        print(f"SRCS differ: {sources(other)} != {srcs}")
        return 1
    srcs = [s for s in srcs if not a.src or s in a.src]
    differ = 0
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(a.jobs) as pool:
        jobs = {(s, tag): pool.submit(listing, tree, s, tmp, tag) for s in srcs for tag, tree in (("other", other), ("this", HERE))}
        for s in srcs:
            old, new = jobs[s, "other"].result(), jobs[s, "this"].result()
            kernels = sum(1 for ln in new if ".vgpr_count:" in ln)
            if old == new:
                print(f"{s}: identical ({kernels} kernels, {len(new)} lines of disassembly and notes)")
            else:
                differ += 1
                d = list(difflib.unified_diff(old, new, "other/" + s, "this/" + s, lineterm="", n=1))
                print(f"{s}: DIFFERENT ({len(d)} diff lines; the first 40:)")
                print("\n".join(d[:40]))
    print("device code: " + ("DIFFERENT in %d of %d sources" % (differ, len(srcs)) if differ else "identical in all %d sources" % len(srcs)))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
