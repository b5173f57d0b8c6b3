"""Do the tests of the one-sequence-per-workgroup kernels on the headline path — the one-launch backbone and its split-precision
twin, the incremental stem (csrc/svdd_seg_body.h, backbone_list_kernel), the windowed value-net tower (windows, parts, _lp windows)
— have teeth? One change of a value, of a comparison or of an index that stays inside the allocated extents at a time (no address
leaves a buffer or the LDS image, no vector access is misaligned, no barrier, wait count or launch shape is touched), in patched
copies of the library loaded through SVDD_HIP_LIB (the tracked sources are never edited): which tests turn red
-> profiles/stem_tower_teeth.txt.
    python tools/stem_tower_teeth.py build [name ...]   (CPU: hipcc cross-compiles) -> build/teeth/<name>/libsvdd_hip.so
    python tools/stem_tower_teeth.py run [name ...]     (GPU) -> the report on stdout
"parent" = the stem and tower tests as they stood before tests/test_lengths_gpu.py; "new" = that file. A mutant is run against the
tests that launch the kernel it changes (its family: the -k expressions below) — the other tests of both sets never execute the
changed code and cannot change colour; `control` runs everything. NOT_BUILT lists mutations named for the record but never
compiled, with the reason.

Family `short*` (-> profiles/short_tile_teeth.txt): the kernels that put SEVERAL sequences into one workgroup tile (L <= 104) —
backbone_kernel<false>'s interleaved schedule, first-layer lookup, entry body, owned slots and padding rows, the stacked towers'
position test and the round-2 lp backbone's row bookkeeping. "parent" = the tests that ran this code before
tests/test_short_lengths_gpu.py; "new" = that file.
    python tools/stem_tower_teeth.py run $(python tools/stem_tower_teeth.py names short)"""
import concurrent.futures
import os
import re
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "svdd_amd", "csrc")
WORK = os.path.join(ROOT, "build", "teeth")
NETS, LPBB, SEG, DEVH = "svdd_nets.hip", "svdd_lp_backbone.hip", "svdd_seg_body.h", "svdd_device.h"
_LIVE = "      for (int r = 0; r < TW_RT; ++r) if (lo < 16 * r + 16 && hi > 16 * r) m |= 1 << r;"
_SHORT = _LIVE.replace("hi > 16 * r)", "hi > 16 * r + 1)")
_BB = "      const int lo = d < 0 ? -d : 0, hi = d > 0 ? tile_rows - d : tile_rows;\n      if (lo >= hi) return 0;\n      int m = 0;\n"
_SPLIT = "      const int d = (t - 4) * sdil[layer];\n      const int lo = d < 0 ? -d : 0, hi = d > 0 ? L - d : L;\n      if (lo >= hi) return 0;\n      int m = 0;\n"
_LP1 = "      if (SPT1) {\n  " + _LIVE
_LP2 = "      const int lo = d < 0 ? -d : 0, hi = d > 0 ? R - d : R;\n      if (lo >= hi) return 0;\n      int m = 0;\n"
_PAD = ("const bool in = row >= 0 && row < L;", "const bool in = row >= 0;")
_PAD1 = ("img[ri * BB_AP + c] = (row >= 0 && row < L) ? fmaxf(v, 0.0f) : 0.0f;", "img[ri * BB_AP + c] = (row >= 0) ? fmaxf(v, 0.0f) : 0.0f;")
_READ = ("f[s][ct][e] = (SEG_MINE(s) && row >= 0 && row < L) ? src[row * BB_C + col0 + 16 * ct] : 0.0f;",
         "f[s][ct][e] = (SEG_MINE(s) && row >= 0 && row < TW_ROWS) ? src[row * BB_C + col0 + 16 * ct] : 0.0f;")
_OWN = "  const int nro = SPT1 ? 7 : __builtin_amdgcn_readfirstlane((nt - rh + 1) >> 1);"
_BODY = "  const int body = SPT1 ? 7 : (nt <= 4 ? 2 : nt <= 8 ? 4 : 7);"
_ZERO = "  if (!SPT1)                                              // rows of the slots nobody owns"
_TOK0 = "            const int tk = (p >= 0 && p < L) ? toks[row + (t - 4) * il] : -1;"
_APOS = "#define TW_ALOAD_APOS(V, POS, OFF) TW_ALOAD(V, (unsigned)((POS) + delta) < (unsigned)L ? (OFF) : a_hi + chk * (CH * 4))"
_LPROW = "tk = a.x[(int64_t)a.row_idx[blockIdx.x * spt + sq] * L + (e - sq * L)]; }"
_KEEP = "const int keep_hi = !(WIN) ? 0 : (nt == 0 ? 0 : (w1 >= L ? L : w1 - TW_EDGE));"
# name -> (family, objects to recompile, [(file, old, new)])
MUTANTS = {
    "control": ("all", [], []),
    # a (row tile, tap) pair alive for exactly ONE row is dropped ------------------------------------------------------------
    "sched_one_row_short": ("backbone", ["svdd_nets.o"], [(NETS, _BB + _LIVE, _BB + _SHORT)]),                    # backbone_kernel
    # ... only at dilation 1 / only at the dilations 16 and 64 (the parent's lengths reach such a pair at dilation 4 alone: L = 105)
    "sched_one_row_short_dil1": ("backbone", ["svdd_nets.o"], [(NETS, _BB + _LIVE, _BB + _LIVE.replace("hi > 16 * r)", "hi > 16 * r + (sdil[layer] == 1))"))]),
    "sched_one_row_short_dil16up": ("backbone", ["svdd_nets.o"], [(NETS, _BB + _LIVE, _BB + _LIVE.replace("hi > 16 * r)", "hi > 16 * r + (sdil[layer] >= 16))"))]),
    "sched_one_row_short_split": ("split", ["svdd_nets.o"], [(NETS, _SPLIT + _LIVE, _SPLIT + _SHORT)]),           # backbone_split_kernel
    "sched_one_row_short_split_dil1": ("split", ["svdd_nets.o"], [(NETS, _SPLIT + _LIVE, _SPLIT + _LIVE.replace("hi > 16 * r)", "hi > 16 * r + (sdil[layer] == 1))"))]),
    "sched_one_row_short_split_dil16up": ("split", ["svdd_nets.o"], [(NETS, _SPLIT + _LIVE, _SPLIT + _LIVE.replace("hi > 16 * r)", "hi > 16 * r + (sdil[layer] >= 16))"))]),
    "sched_one_row_short_lp_dil1": ("lp", ["svdd_lp_backbone.o"], [(LPBB, _LP1, _LP1.replace("hi > 16 * r)", "hi > 16 * r + (sdil[layer] == 1))")),
                                                                   (LPBB, _LP2 + _LIVE, _LP2 + _LIVE.replace("hi > 16 * r)", "hi > 16 * r + (sdil[layer] == 1))"))]),
    "sched_one_row_short_lp_dil16up": ("lp", ["svdd_lp_backbone.o"], [(LPBB, _LP1, _LP1.replace("hi > 16 * r)", "hi > 16 * r + (sdil[layer] >= 16))")),
                                                                      (LPBB, _LP2 + _LIVE, _LP2 + _LIVE.replace("hi > 16 * r)", "hi > 16 * r + (sdil[layer] >= 16))"))]),
    "sched_one_row_short_lp": ("lp", ["svdd_lp_backbone.o"], [(LPBB, _LP1, _LP1.replace("hi > 16 * r)", "hi > 16 * r + 1)")),
                                                              (LPBB, _LP2 + _LIVE, _LP2 + _SHORT)]),               # both lp kernels
    "tapmask_one_row_short": ("stem", ["svdd_nets.o"], [(SEG, "min(L, L - d) > 16 * T) m |= 1 << t;", "min(L, L - d) > 16 * T + 1) m |= 1 << t;")]),
    # the segment kernels' padding rows ------------------------------------------------------------------------------------
    "seg_pad_not_zero": ("stem", ["svdd_nets.o"], [(SEG,) + _PAD]),              # LayerNorm'd image rows >= L become beta-valued
    "seg_layer1_pad_not_zero": ("stem", ["svdd_nets.o"], [(SEG,) + _PAD1]),      # layer 1: f_0 of the rows >= L is not zero
    "seg_reads_rows_past_L": ("stem", ["svdd_nets.o"], [(SEG,) + _READ]),        # f of rows L .. 207 is read from the plane
    "seg_reads_rows_past_L+seg_pad_not_zero": ("stem", ["svdd_nets.o"], [(SEG,) + _READ, (SEG,) + _PAD]),
    # backbone_list_kernel: the memory-safe stand-in of list_word_path_any_pointer ----------------------------------------------
    "list_byte_path_drops_last": ("stem", ["svdd_nets.o"], [(NETS, "for (int e = 0; e < 8 && 8 * w8 + e < L; ++e) {", "for (int e = 0; e < 8 && 8 * w8 + e < L - 1; ++e) {")]),
    # the windowed tower -----------------------------------------------------------------------------------------------------
    "parts_reach_short": ("tower", ["svdd_nets.o"], [(NETS, "const int h = R + 2 * (nl - tid);", "const int h = R + 2 * (nl - tid) - 1;")]),
    "parts_store_past_L": ("tower", ["svdd_nets.o"], [(NETS, "if (row < c.L) {", "if (row < min(c.L + 1, TW_ROWS)) {")]),
    "win_keep_one_short": ("tower", ["svdd_nets.o", "svdd_lp_tower.o"], [(DEVH, _KEEP, _KEEP.replace("w1 - TW_EDGE));", "w1 - TW_EDGE) - 1);"))]),
    # ---- the shared-tile kernels (L <= 104): family short* ------------------------------------------------------------------
    # backbone_kernel<false> only (the one-sequence form keeps its schedule): a one-row (row tile, tap) pair is dropped
    "short_sched_one_row": ("short", ["svdd_nets.o"], [(NETS, _BB + _LIVE, _BB + _LIVE.replace("hi > 16 * r)", "hi > 16 * r + !SPT1)"))]),
    "short_sched_one_row_dil1": ("short", ["svdd_nets.o"], [(NETS, _BB + _LIVE, _BB + _LIVE.replace("hi > 16 * r)", "hi > 16 * r + (!SPT1 && sdil[layer] == 1))"))]),
    "short_sched_one_row_dil16up": ("short", ["svdd_nets.o"], [(NETS, _BB + _LIVE, _BB + _LIVE.replace("hi > 16 * r)", "hi > 16 * r + (!SPT1 && sdil[layer] >= 16))"))]),
    # ... the lo side: a negative tap whose first live row is the LAST row of a row tile (lo = 16 r + 15: dilation 1, odd s k)
    "short_sched_one_row_lo": ("short", ["svdd_nets.o"], [(NETS, _BB + _LIVE, _BB + _LIVE.replace("lo < 16 * r + 16", "lo < 16 * r + 15 + SPT1"))]),
    # the first-layer lookup steps one ROW per tap instead of il rows (row + (t - 4) stays inside [0, tile_rows) wherever p is inside [0, L))
    "short_lookup_il_1": ("short", ["svdd_nets.o"], [(NETS, _TOK0, _TOK0.replace("(t - 4) * il]", "(t - 4)]"))]),
    "short_body_4_at_nt_9": ("short", ["svdd_nets.o"], [(NETS, _BODY, _BODY.replace("nt <= 8 ? 4", "nt <= 9 ? 4"))]),
    "short_nro_one_less": ("short", ["svdd_nets.o"], [(NETS, _OWN, _OWN.replace("(nt - rh + 1) >> 1", "(nt - rh) >> 1"))]),
    "short_unowned_rows_not_zeroed": ("short", ["svdd_nets.o"], [(NETS, _ZERO, _ZERO.replace("if (!SPT1) ", "if (false)  "))]),
    # the stacked towers: a tap may reach position L = row 0 of the next sequence of the tile (the row exists: at most the zero row TW_ROWS)
    "short_tower_apos_L_plus_1": ("short_tower", ["svdd_nets.o"], [(NETS, _APOS, _APOS.replace("< (unsigned)L ?", "< (unsigned)(L + 1) ?"))]),
    # the round-2 lp backbone with a row index list: every sequence of a tile but the last reads its tokens at position 0
    # (e - (sq + 1) L clamped into [0, L): inside the sequence's row of x)
    "short_lp_stacked_row_of_next": ("short_lp", ["svdd_lp_backbone.o"], [(LPBB, _LPROW, _LPROW.replace("(e - sq * L)]", "max(e - min(sq + 1, spt - 1) * L, 0)]"))]),
}
NOT_BUILT = {
    "short_ragged_tile_reads_row_n": "backbone_kernel<false> without the `seq0 + q < nvalid` test of the token gather: a ragged last tile reads the tokens of "
                                     "rows n .. (and row_idx[count ..]), which lie behind the allocations of the tests (x holds exactly n rows, row_idx exactly "
                                     "count entries): not built. It could not change a result either: the interleaved sequences of a tile never meet — a "
                                     "tap is a row offset of a multiple of spt, LayerNorm is per row, and the output loop has its own `seq0 + q >= nvalid` "
                                     "test — so what the rows of a sequence that does not exist hold is never read for a row that is written.",
    "list_word_path_any_pointer": "backbone_list_kernel taking the 8-token compare whatever the three token pointers are: a 64-bit load and a 64-bit "
                                  "store at an address that is no multiple of 8, a misaligned vector access, which this tool does not compile. Its "
                                  "stand-in is list_byte_path_drops_last.",
    "tight_w1_no_clip": "svdd_candidate_windows_tight without the min(L, ..): w1 = w0 + 16 ceil((hi + 28 - w0) / 16) gives up to 15 row tiles "
                        "(L = 208, changes at 0 and 207: w1 = 240), and the window kernels compute nt = (w1 - w0) / 16 tiles in an LDS image of "
                        "TW_RT = 13 tiles: addresses past the image, so the mutant is not built.",
}
INCR = ["tests/test_backbone_incremental_gpu.py", "tests/test_backbone_incr2_gpu.py", "tests/test_backbone_incr3_gpu.py", "tests/test_backbone_incr4_gpu.py"]
NETK, LPT = "tests/test_net_kernels_gpu.py", "tests/test_lp_gpu.py"
TOWER = ["tests/test_tower_parts_gpu.py", "tests/test_tower_tight_windows_gpu.py"]
NEW = "tests/test_lengths_gpu.py"
SHORT, FUSED, SKIP = "tests/test_short_lengths_gpu.py", "tests/test_fused_gpu.py", "tests/test_skip_gpu.py"
_PARENT_K = "incr or tower_parts or tight_windows or backbone_f32 or backbone_save or backbone_lp or conv_tower or candidate_windows or value_net"
# family -> (parent files, parent -k, new -k)
FAMILIES = {
    "all": (INCR + TOWER + [NETK, LPT], _PARENT_K, "not zzz"),
    "backbone": (INCR + [NETK], "incr or chain or taps or decode or rows or parity or residen or backbone_f32 or backbone_save", "backbone_forward or stem"),
    "split": ([NETK], "several_workgroups", "backbone_forward"),
    "lp": ([NETK, LPT], "backbone_lp", "backbone_lp"),
    "stem": (INCR, "not zzz", "stem"),
    "tower": (TOWER + [NETK, LPT], "tower or windows or value_net or parts", "tower"),
    # (parent files, parent -k, new -k, the new file)
    "short": ([NETK, FUSED, SKIP], "backbone_f32 or sequences_per_tile or one_launch_backbone or compacted or short_sequences or config3", "backbone_f32", SHORT),
    "short_tower": ([NETK, FUSED, SKIP], "conv_tower_f32 or value_net or tower_vs or short_sequences or config3", "conv_tower_f32", SHORT),
    "short_lp": ([NETK, LPT, FUSED, SKIP], "backbone_lp or sequences_per_tile or compacted or short_sequences", "backbone_lp and f16x3 and not bf16x3", SHORT),
}


def build(name):
    family, objs, edits = MUTANTS[name]
    work = os.path.join(WORK, name)
    shutil.rmtree(work, ignore_errors=True)
    os.makedirs(work)
    for f in os.listdir(CSRC):
        if f.endswith((".hip", ".h")) or f == "Makefile" or (f.endswith(".o") and f not in objs):
            shutil.copy(os.path.join(CSRC, f), work)
    for fn, old, new in edits:
        p = os.path.join(work, fn)
        s = open(p).read()
        assert s.count(old) == 1 and old != new, (name, fn, old, s.count(old))
        open(p, "w").write(s.replace(old, new))
    for f in os.listdir(work):                                    # the copied objects are up to date: only `objs` are compiled
        if f.endswith(".o"):
            os.utime(os.path.join(work, f))
    r = subprocess.run(["make", "-C", work, "-j2", "INC=" + os.path.join(ROOT, "include")], capture_output=True, text=True)
    ok = os.path.exists(os.path.join(work, "libsvdd_hip.so"))
    for f in os.listdir(work):
        if f != "libsvdd_hip.so":
            os.remove(os.path.join(work, f))
    print(name, "ok" if ok else "FAILED " + r.stderr[-600:], flush=True)
    return ok


def pytest_run(lib, files, k, budget):
    env = dict(os.environ, SVDD_HIP_LIB=lib)
    cmd = ["timeout", "-k", "10", str(budget), sys.executable, "-m", "pytest", *files, "-m", "gpu", "-q", "--no-header", "-p", "no:cacheprovider",
           "-k", k, "--tb=line"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True)
    failed = sorted(re.findall(r"^FAILED (\S+)", r.stdout, flags=re.M))
    tail = [ln for ln in r.stdout.splitlines() if re.search(r"\d+ (passed|failed)", ln)]
    rc = r.returncode
    if rc in (0, 1) and re.search(r"illegal memory access|HIP error|hipError|HSA_STATUS_ERROR|Memory access fault", r.stdout + r.stderr):
        rc = 134                                              # a GPU fault a test caught as an exception: pytest itself ends with 1
    return rc, failed, tail[-1].strip("= ") if tail else r.stdout[-300:] + r.stderr[-300:]


def main():
    cmd, names = sys.argv[1], sys.argv[2:] or [n for n in MUTANTS if not MUTANTS[n][0].startswith("short")]
    if cmd == "names":                                        # the mutants of the families that start with the given word
        print(" ".join(n for n in MUTANTS if MUTANTS[n][0].startswith(names[0]) and MUTANTS[n][1]))
        return
    if cmd == "build":
        assert all(os.path.exists(os.path.join(CSRC, o)) for n in names for o in MUTANTS[n][1]), "build the library first: the untouched objects are reused"
        with concurrent.futures.ThreadPoolExecutor(4) as pool:
            sys.exit(0 if all(list(pool.map(build, names))) else 1)
    for name, why in NOT_BUILT.items():
        print(f"## {name}: not built. {why}")
    for name in names:
        family, _, edits = MUTANTS[name]
        files, pk, nk, new = (FAMILIES[family] + (NEW,))[:4]
        lib = os.path.join(WORK, name, "libsvdd_hip.so")
        print(f"## {name} [{family}]: " + (" ; ".join(f"{o.strip()} -> {n.strip()}" for _, o, n in edits) or "the tracked kernels"), flush=True)
        for label, fs, k, budget in (("new", [new], nk, 240), ("parent", files, pk, 420)):
            rc, failed, tail = pytest_run(lib, fs, k, budget)
            print(f"{label}: {'RED' if failed else 'green'} ({tail})")
            by = {}
            for f in failed:
                by.setdefault(f.split("::")[1].split("[")[0], []).append(f.split("[", 1)[1].rstrip("]") if "[" in f else "")
            for t, ids in by.items():
                print(f"   {t}: {len(ids)} red: " + " ".join(ids[:40]) + (" ..." if len(ids) > 40 else ""), flush=True)
            if rc not in (0, 1):                                  # a time limit, an abort, a fault: nothing more is started on the GPU
                print(f"stopped: pytest ended with status {rc}")
                sys.exit(rc)


if __name__ == "__main__":
    main()
