"""Do the tests of svdd_backbone_cnn_grad_f32, svdd_conv1d_cl_f32 and svdd_epilogue_ln_f32 have teeth? One change of a value or of an
index that stays inside the allocated extents at a time (no address leaves a buffer, no barrier or wait count is touched), in patched
copies of the library loaded through SVDD_HIP_LIB (the tracked sources are never edited): which tests turn red
-> profiles/backbone_grad_teeth.txt.
    python tools/backbone_grad_teeth.py build [name ...]   (CPU: hipcc cross-compiles) -> build/teeth/<name>/libsvdd_hip.so
    python tools/backbone_grad_teeth.py run [name ...]     (GPU) -> the report on stdout
"before" = tests/test_fused_gpu.py and tests/test_configs_gpu.py as they stand (what held these entries until now); "new" =
tests/test_backbone_grad_kernel_gpu.py and tests/test_conv_epilogue_kernels_gpu.py.
NOT_BUILT lists a mutation that is named for the record but never compiled, with the reason."""
import os
import re
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "svdd_amd", "csrc")
WORK = os.path.join(ROOT, "build", "teeth")
SRC = "svdd_nets.hip"
_IMG0 = "            img[row * BB_AP + col0] = ((mk >> ((r * 2) * 4 + e)) & 1ull) && row < tile_rows ? G[r][0][e] : 0.0f;"
_IMG1 = "            img[row * BB_AP + col0 + 16] = ((mk >> ((r * 2 + 1) * 4 + e)) & 1ull) && row < tile_rows ? G[r][1][e] : 0.0f;"
_ENTRY = "      const int d = (t - 4) * sdil[step];\n      const int lo = d < 0 ? -d : 0, hi = d > 0 ? L - d : L;"
_ALOAD = "reinterpret_cast<const float4*>(Ah + ((p_ >= 0 && p_ < L) ? arow[R] + delta : CONV_ROWS) * CHP);"
MUTANTS = {
    "control": [],
    # backbone_grad_kernel ---------------------------------------------------------------------------------------------------
    # 1. the per-step image keeps G on the padding rows (12 spaces of indent: the step loop's image, not the first layer's)
    "grad_no_row_mask": [(_IMG0, _IMG0.replace(" && row < tile_rows", "")), (_IMG1, _IMG1.replace(" && row < tile_rows", ""))],
    # 2. the schedule takes every tile up to L for a positive tap: tiles whose taps read only rows >= L are processed too
    "grad_hi_is_L": [(_ENTRY, _ENTRY.replace("hi = d > 0 ? L - d : L;", "hi = L;"))],
    # 2b. ... and the other way: a positive tap's last live row is left out of the tile test (a tile alive for ONE row is dropped)
    "grad_hi_one_short": [(_ENTRY, _ENTRY.replace("hi = d > 0 ? L - d : L;", "hi = d > 0 ? L - d - 1 : L;"))],
    # 3. the dilations in forward order
    "grad_dil_forward": [("sdil[tid] = tid == 0 ? 1 : a.dil[nl - tid];", "sdil[tid] = tid == 0 ? 1 : a.dil[tid - 1];")],
    # 4. LayerNorm backward without the xhat mean(t xhat) term
    "grad_no_xhat_term": [("G[r][0][e] += rsv[e] * (acc[r][0][e] - m1v[e] - xh[r][0][e] * m2v[e]);", "G[r][0][e] += rsv[e] * (acc[r][0][e] - m1v[e]);"),
                          ("G[r][1][e] += rsv[e] * (acc[r][1][e] - m1v[e] - xh[r][1][e] * m2v[e]);", "G[r][1][e] += rsv[e] * (acc[r][1][e] - m1v[e]);")],
    # conv1d_cl_kernel -------------------------------------------------------------------------------------------------------
    # 5'. a tap may read ONE row past its sequence's end: the next sequence's first row where a tile holds several, the zero row
    #     (index CONV_ROWS at most) where it holds one — the memory-safe stand-in for the mutation of NOT_BUILT
    "conv_reads_next_sequence": [(_ALOAD, _ALOAD.replace("p_ < L)", "p_ < L + 1)"))],
    # epilogue_ln_kernel -----------------------------------------------------------------------------------------------------
    # 6. a row stride that skips nothing below 16,384 rows (no second pass) and mis-visits above
    "epilogue_stride": [("for (int64_t r = wave; r < a.R; r += nwaves) {", "for (int64_t r = wave; r < a.R; r += nwaves + 1) {")],
}
NOT_BUILT = {
    "conv_apos_no_tile_rows": "conv1d_cl_kernel: apos[r] = (rt < CONV_RT) ? tr % L : ... (without `tr < tile_rows`). A padding row of the tile "
                              "would then take the taps of position tr % L and read image rows up to tr - tr % L + L - 1, which is past the "
                              "224-row image (L = 200: row 399) and for 64 output channels past the workgroup's LDS: an address outside a "
                              "buffer, which this tool does not compile. It could not show in any output either: the store is guarded by "
                              "`tr < tile_rows && row0 + tr < total_rows`, so what a padding row accumulates is never written.",
}
BEFORE = ["tests/test_fused_gpu.py", "tests/test_configs_gpu.py"]
NEW = ["tests/test_backbone_grad_kernel_gpu.py", "tests/test_conv_epilogue_kernels_gpu.py"]


def build(name):
    work = os.path.join(WORK, name)
    shutil.rmtree(work, ignore_errors=True)
    os.makedirs(work)
    obj = SRC.replace(".hip", ".o")
    for f in os.listdir(CSRC):
        if f.endswith((".hip", ".h")) or f == "Makefile" or (f.endswith(".o") and f != obj):
            shutil.copy(os.path.join(CSRC, f), work)
    for f in os.listdir(work):
        if f.endswith(".o"):
            os.utime(os.path.join(work, f))
    p = os.path.join(work, SRC)
    s = open(p).read()
    for old, new in MUTANTS[name]:
        assert s.count(old) == 1 and old != new, (name, old)
        s = s.replace(old, new)
    open(p, "w").write(s)
    r = subprocess.run(["make", "-C", work, "INC=" + os.path.join(ROOT, "include")], capture_output=True, text=True)
    ok = os.path.exists(os.path.join(work, "libsvdd_hip.so"))
    for f in os.listdir(work):
        if f != "libsvdd_hip.so":
            os.remove(os.path.join(work, f))
    print(name, "ok" if ok else "FAILED " + r.stderr[-600:], flush=True)
    return ok


def pytest_run(lib, files, budget):
    env = dict(os.environ, SVDD_HIP_LIB=lib)
    cmd = ["timeout", "-k", "10", str(budget), sys.executable, "-m", "pytest", *files, "-m", "gpu", "-q", "--no-header", "-p", "no:cacheprovider", "--tb=line"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True)
    failed = sorted(re.findall(r"^FAILED (\S+)", r.stdout, flags=re.M))
    tail = [ln for ln in r.stdout.splitlines() if re.search(r"\d+ (passed|failed)", ln)]
    rc = r.returncode
    if rc in (0, 1) and re.search(r"illegal memory access|HIP error|hipError|HSA_STATUS_ERROR|Memory access fault", r.stdout + r.stderr):
        rc = 134                                              # a GPU fault a test caught as an exception: pytest itself ends with 1
    return rc, failed, tail[-1].strip("= ") if tail else r.stdout[-300:] + r.stderr[-300:]


def main():
    cmd, names = sys.argv[1], sys.argv[2:] or list(MUTANTS)
    if cmd == "build":
        sys.exit(0 if all([build(n) for n in names]) else 1)
    for name, why in NOT_BUILT.items():
        print(f"## {name}: not built. {why}")
    for name in names:
        lib = os.path.join(WORK, name, "libsvdd_hip.so")
        print(f"## {name}: " + (" ; ".join(f"{o.strip()} -> {n.strip()}" for o, n in MUTANTS[name]) or "the tracked kernels"), flush=True)
        for label, files, budget in (("new", NEW, 300), ("before", BEFORE, 420)):
            rc, failed, tail = pytest_run(lib, files, budget)
            print(f"{label}: {'RED' if failed else 'green'} ({tail})")
            by = {}
            for f in failed:
                by.setdefault(f.split("::")[1].split("[")[0], []).append(f.split("[", 1)[1].rstrip("]") if "[" in f else "")
            for t, ids in by.items():
                print(f"   {t}: {len(ids)} red: " + " ".join(ids[:12]) + (" ..." if len(ids) > 12 else ""), flush=True)
            if rc not in (0, 1):                                  # a time limit, an abort, a fault: nothing more is started on the GPU
                print(f"stopped: pytest ended with status {rc}")
                sys.exit(rc)


if __name__ == "__main__":
    main()
