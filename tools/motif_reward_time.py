"""Timing of motif-guided SVDD-PM decoding (svdd_amd/motifs.py MotifReward / GuidedReward, svdd_motif_reward) on synthetic
nets: B = 256, L = 200, M = 10, 128 steps, Philox, the fused ConvGRU reward net, 16 seeded random motifs of widths 6 .. 20 with their
p = 1e-4 thresholds, a hit weight and a margin weight on every motif. In one process, every decode after one warm-up, between
synchronisations:
  (a) the guided decode: controlled_sample_tweedie(GuidedReward(reward, mr)) through the skipping loop;
  (b) the same decode under the reward net alone (the un-guided-reward PM decode): the extra time per step is (a) - (b);
  (c) the same guided decode composed from what the library had before svdd_motif_reward: a callable that takes the candidates'
      one-hot x0-hat rows, packs them (svdd_pack_tokens), calls motifs.scan_rows and folds the [n, M] tables in torch, handed to
      controlled_sample_tweedie — which has to take its generic loop (a full backbone on all B M candidates, no work skipping).
      Whether its tokens equal (a)'s is checked before anything is timed, and reported;
  (d) svdd_motif_reward alone at the loop's shape (n = B M rows, the device count at the decode's mean number of live candidates and
      at n), device events over back-to-back launches: its share of a step of (a);
  (e) (d) for every row tile: `build` makes copies of the library with SVDD_MOTIF_REWARD_ROWS = 8, 32, 64 under build/motif_reward_rows/
      (the tracked sources are not edited); the run starts one child process per copy (SVDD_HIP_LIB) and reports its kernel times.
Usage: python tools/motif_reward_time.py build                 (no GPU needed: compiles the copies)
       timeout -k 10 900 python tools/motif_reward_time.py [--rounds 3] [--out profiles/motif_reward_time.txt] [--note TEXT ...]"""
import argparse, json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CSRC = os.path.join(ROOT, "svdd_amd", "csrc")
VARIANTS = os.path.join(ROOT, "build", "motif_reward_rows")
TILES = (8, 32, 64)

ap = argparse.ArgumentParser()
ap.add_argument("mode", nargs="?", default="run", choices=["run", "build", "kernel"])
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--launches", type=int, default=200)
ap.add_argument("--live", type=int, default=0, help="kernel mode: the device count (0: all rows)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motif_reward_time.txt"))
ap.add_argument("--note", action="append", default=[])
args = ap.parse_args()


def variant_lib(rows):
    return os.path.join(VARIANTS, f"rows{rows}", "libsvdd_hip.so")


if args.mode == "build":
    subprocess.check_call(["make", "-C", CSRC, "-j", "8"])                  # the other translation units' objects, as they are
    others = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".o") and f != "svdd_motifs.o")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC]
    for rows in TILES:
        d = os.path.dirname(variant_lib(rows))
        os.makedirs(d, exist_ok=True)
        obj = os.path.join(d, "svdd_motifs.o")
        subprocess.check_call([hipcc, *flags, f"-DSVDD_MOTIF_REWARD_ROWS={rows}", "-c", "-o", obj, os.path.join(CSRC, "svdd_motifs.hip")])
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", variant_lib(rows), obj, *others])
        print("built", variant_lib(rows))
    sys.exit(0)

import numpy as np
import torch
from svdd_amd import motifs, ops

B, L, M, S, DEV, NMOTIFS = 256, 200, 10, 128, "cuda:0", 16
rng = np.random.default_rng(0)
widths = rng.integers(6, 21, NMOTIFS)
mset = motifs.MotifSet.from_pfms([rng.dirichlet([0.5] * 4, int(w)) for w in widths])
mr = motifs.MotifReward(mset, hit_weight=rng.uniform(-2, 2, NMOTIFS), margin_weight=rng.uniform(0.0, 0.01, NMOTIFS))


def kernel_ms(live):
    """Median time of one svdd_motif_reward launch on n = B M random rows under a device count of `live`."""
    n = B * M
    tok = torch.from_numpy(np.random.default_rng(1).integers(0, 4, (n, L)).astype(np.uint8)).to(DEV)
    count = torch.tensor([live], dtype=torch.int32, device=DEV)
    base = torch.zeros(n, device=DEV)
    for _ in range(10):
        mr.term_tokens(tok, count=count, base=base, out=base)
    ts = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(args.launches):
            mr.term_tokens(tok, count=count, base=base, out=base)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) / args.launches)
    return sorted(ts)[len(ts) // 2]


if args.mode == "kernel":                                       # a child of the run: the library is the one SVDD_HIP_LIB names
    live = args.live or B * M
    print(json.dumps({"live_ms": kernel_ms(live), "all_ms": kernel_ms(B * M), "checksum": float(mr.term(
        np.random.default_rng(1).integers(0, 4, (B * M, L))).double().sum())}))
    sys.exit(0)

import time
from svdd_amd import synthetic

model, _, _, reward = synthetic.build("dna", DEV)
model.rng_mode, model.philox_seed = "philox", 0
fused = model.reward_callable(reward)
tables = mset.to_device(DEV)
hc, cap, mc, fl = (torch.from_numpy(a.astype(np.int64)).to(DEV) for a in (mr.hit_coef, mr.hit_cap, mr.margin_coef, mr.margin_floor))
thr = torch.from_numpy(mset.threshold.astype(np.int64)).to(DEV)


def composed(onehot):
    """The guided reward from the public pieces there were before svdd_motif_reward: onehot [n, 4, L] -> [n, 1, 1]."""
    tok = onehot.argmax(1).to(torch.uint8)
    row_hits, best, _, _ = motifs.scan_rows(tok, mset)
    T = (hc * torch.minimum(row_hits.long(), cap) + mc * torch.maximum(torch.minimum(best.long() - thr, torch.zeros_like(thr)), -fl)).sum(1)
    out = fused(onehot).float().clone()
    out[:, 0, 0] += T.to(torch.float32) * mr.unit
    return out


def decode(rf):
    return model.controlled_sample_tweedie(rf, num_steps=S, eval_sp_size=B, sample_M=M, options="True")


def timed(rf, rounds):
    ts = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        decode(rf)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts = sorted(ts)
    return ts[len(ts) // 2], ts


guided = motifs.GuidedReward(reward, mr)
model.skip_stats = {}
x_a = decode(guided)                                              # also (a)'s warm-up
stats, model.skip_stats = model.skip_stats, None
assert stats.get("kind") == "pm", "the guided decode did not take the skipping loop"
x_b = decode(reward)
x_c = decode(composed)
same = bool(torch.equal(x_a, x_c))                                # reported, whatever it is
live = max(1, round(stats["live_candidates"] / S))
term_a, term_b = float(mr.term(x_a).double().mean()), float(mr.term(x_b).double().mean())

ms = {}
ms["a"], all_a = timed(guided, args.rounds)
ms["b"], all_b = timed(reward, args.rounds)
ms["c"], all_c = timed(composed, args.rounds)
k_live, k_all = kernel_ms(live), kernel_ms(B * M)
fmt = lambda v, ts: f"{v:9.2f} ms [{ts[0]:.2f} .. {ts[-1]:.2f}] = {v / S:7.4f} ms / step"    # noqa: E731
lines = [f"Motif-guided SVDD-PM timing: B = {B}, L = {L}, M = {M}, {S} steps, Philox, fp32, fused ConvGRU reward net; {NMOTIFS} seeded random motifs "
         f"of widths 6 .. 20 (p = 1e-4 thresholds, {int(mset.reachable.sum())} reachable), both strands, hit and margin weights on all of them",
         f"device: {torch.cuda.get_device_name(0)}; whole decodes, wall clock between synchronisations, one warm-up each, median [min .. max]", "",
         f"  (a) guided decode, skipping loop (svdd_motif_reward):            {fmt(ms['a'], all_a)}",
         f"  (b) reward net alone (the un-guided-reward PM decode):           {fmt(ms['b'], all_b)}",
         f"  (c) guided decode composed from pack + scan_rows + torch fold,",
         f"      generic PM loop (the only way before svdd_motif_reward):     {fmt(ms['c'], all_c)}",
         f"  tokens of (a) and (c) equal: {same} ({int((x_a != x_c).sum())} of {x_a.numel()} differ);   (c) : (a) = {ms['c'] / ms['a']:.2f}",
         f"  (a) - (b) = {(ms['a'] - ms['b']) / S * 1e3:.1f} us / step extra for the motif term",
         f"  mean motif term of the decoded batch: guided {term_a:.4f}, reward net alone {term_b:.4f}",
         f"  live candidates per step (mean): {live} of {B * M}", "",
         f"  (d) svdd_motif_reward alone, n = {B * M}, {args.launches} back-to-back launches, device events, median of 5:",
         f"      count = {live}: {k_live * 1e3:8.1f} us = {k_live / (ms['a'] / S) * 100:.2f} % of a step of (a);   count = n: {k_all * 1e3:8.1f} us", ""]
lines.append("  (e) the same per row tile (copies of the library built with SVDD_MOTIF_REWARD_ROWS, one child process each):")
for rows in TILES:
    lib = variant_lib(rows)
    if not os.path.exists(lib):
        lines.append(f"      {rows:3d} rows: no build (python tools/motif_reward_time.py build)")
        continue
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "kernel", "--live", str(live), "--launches", str(args.launches)],
                         env=dict(os.environ, SVDD_HIP_LIB=lib), capture_output=True, text=True, timeout=300)
    if res.returncode != 0:
        lines.append(f"      {rows:3d} rows: the child failed ({res.returncode}): {res.stderr.strip().splitlines()[-1] if res.stderr.strip() else ''}")
        break                                                     # nothing more is started on the device after a failure
    r = json.loads(res.stdout.strip().splitlines()[-1])
    lines.append(f"      {rows:3d} rows / workgroup ({-(-B * M // rows):4d} workgroups): count = {live}: {r['live_ms'] * 1e3:8.1f} us;   "
                 f"count = n: {r['all_ms'] * 1e3:8.1f} us;   checksum {r['checksum']!r}")
lines += [""] + args.note
text = "\n".join(lines) + "\n"
print(text)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text)
