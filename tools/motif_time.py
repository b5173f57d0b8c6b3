"""Timing of the PWM motif scan (svdd_amd/motifs.py) on synthetic data, in one process: 512 seeded random motifs of widths
6 .. 20 with their p = 1e-4 thresholds against 2048 designs of L = 200 and against a seeded random set of 2^19 rows, both strands.
Three arms, run in turn round after round (interleaved) after one warm-up each, every run between two device events:
  (a) svdd_pack_tokens + svdd_motif_scan, totals only (hits and rows_hit);
  (b) the same with the per-row outputs (row_hits, row_best) as well;
  (c) the same totals composed from torch ops: conv1d over one-hot rows with integer-valued fp32 weights padded to 32 columns (exact:
      every |sum| is below 2^24), the reverse strand as further output channels, then >= threshold and sums, in row chunks sized so
      that the conv output stays under 1 GiB. Asserted EQUAL to (a) before anything is timed.
Median, minimum and maximum over the rounds are reported.
Run it under a time limit: timeout -k 10 900 python tools/motif_time.py
Usage: python tools/motif_time.py [--rounds 7] [--big_rounds 3] [--out profiles/motif_time.txt] [--note TEXT ...]"""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import torch.nn.functional as F
from svdd_amd import motifs, ops

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--big_rounds", type=int, default=3)
ap.add_argument("--designs", type=int, default=2048)
ap.add_argument("--big_rows", type=int, default=1 << 19)
ap.add_argument("--motifs", type=int, default=512)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motif_time.txt"))
ap.add_argument("--note", action="append", default=[])
args = ap.parse_args()

L, M, DEV = 200, args.motifs, "cuda:0"
rng = np.random.default_rng(0)
widths = rng.integers(6, 21, M)
mset = motifs.MotifSet.from_pfms([rng.dirichlet([0.5] * 4, int(w)) for w in widths])
tables = mset.to_device(DEV)
sets = {"designs": rng.integers(0, 4, (args.designs, L)).astype(np.uint8), "big": rng.integers(0, 4, (args.big_rows, L)).astype(np.uint8)}
for x in sets.values():                                  # consensus sites in every 16th row, so that the totals are not only chance hits
    for r in range(0, x.shape[0], 16):
        m = r // 16 % M
        x[r, 7:7 + widths[m]] = mset.pwm[m, :widths[m]].argmax(1)
sets = {name: torch.from_numpy(x).to(DEV) for name, x in sets.items()}

# the composition's weights: [2M, 4, 32], forward then reverse strand (column w - 1 - i, token 3 - t), zero beyond the width
pwm = torch.from_numpy(mset.pwm.astype(np.float32))
wf = pwm.permute(0, 2, 1).clone()
wr = torch.zeros_like(wf)
for m, w in enumerate(widths):
    wf[m, :, w:] = 0
    wr[m, :, :w] = pwm[m, :w].flip(0).flip(1).T
weight = torch.cat([wf, wr]).to(DEV)
thr = torch.from_numpy(mset.threshold.astype(np.float32)).to(DEV).repeat(2)[None, :, None]
valid = (torch.arange(L, device=DEV)[None, :] <= (L - torch.from_numpy(widths).to(DEV))[:, None]).repeat(2, 1)[None]    # [1, 2M, L]
CHUNK = max(1, (1 << 30) // (2 * M * L * 4))


def scan(x, rows_too):
    N = x.shape[0]
    hits = torch.zeros(M, dtype=torch.int64, device=DEV)
    rows_hit = torch.zeros_like(hits)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    row_hits = torch.empty((N, M), dtype=torch.int32, device=DEV) if rows_too else None
    row_best = torch.empty((N, M), dtype=torch.int64, device=DEV) if rows_too else None
    ops.motif_scan(ops.pack_tokens(x, err=err), L, tables, True, hits, rows_hit, row_hits, row_best)
    return hits, rows_hit


def composed(x):
    hits = torch.zeros(M, dtype=torch.int64, device=DEV)
    rows_hit = torch.zeros_like(hits)
    for r0 in range(0, x.shape[0], CHUNK):
        onehot = F.one_hot(x[r0:r0 + CHUNK].long(), 4).permute(0, 2, 1).float()
        hit = (F.conv1d(F.pad(onehot, (0, 31)), weight) >= thr) & valid                   # [n, 2M, L]
        hits += hit.sum((0, 2)).view(2, M).sum(0)
        rows_hit += (hit[:, :M].any(2) | hit[:, M:].any(2)).sum(0)
    return hits, rows_hit


def once(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    f()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(ts):
    ts = sorted(ts)
    return f"{ts[len(ts) // 2]:9.3f} ms [{ts[0]:.3f} .. {ts[-1]:.3f}]", ts[len(ts) // 2]


lines = [f"Motif-scan timing: {M} seeded random motifs of widths 6 .. 20 (p = 1e-4 thresholds, {int(mset.reachable.sum())} reachable), L = {L}, both "
         f"strands; the arms run in turn, round after round, after one warm-up each; device events; median [minimum .. maximum]",
         f"device: {torch.cuda.get_device_name(0)}; conv1d row chunk {CHUNK} rows ([rows, {2 * M}, {L}] fp32 under 1 GiB)", ""]
for name, rounds in (("designs", args.rounds), ("big", args.big_rounds)):
    x = sets[name]
    N = x.shape[0]
    (ha, ra), (hb, rb) = scan(x, False), composed(x)                 # also the warm-up of both
    assert torch.equal(ha, hb) and torch.equal(ra, rb), "the kernel and the torch composition disagree"
    assert torch.equal(scan(x, True)[0], ha) and int(ha.sum()) > 0
    arms = {"a": lambda: scan(x, False), "b": lambda: scan(x, True), "c": lambda: composed(x)}
    ts = {k: [] for k in arms}
    for _ in range(rounds):
        for k, f in arms.items():
            ts[k].append(once(f))
    lookups = float(sum(N * (L - int(w) + 1) * int(w) * 2 for w in widths))
    (sa, ma), (sb, _), (sc, mc) = stats(ts["a"]), stats(ts["b"]), stats(ts["c"])
    lines += [f"{N} rows x {L}: {lookups:.3e} table look-ups, {int(ha.sum())} hits, {rounds} rounds; totals equal: True",
              f"  (a) svdd_pack_tokens + svdd_motif_scan, totals only:        {sa} = {lookups / ma / 1e6:.1f} G look-ups/s",
              f"  (b) the same with row_hits and row_best [{N}, {M}]:      {sb}",
              f"  (c) torch conv1d over one-hot rows, >= threshold, sums:     {sc}",
              f"  (a) : (c) = {ma / mc:.4f} ((c) is {mc / ma:.1f} x (a))", ""]
lines += args.note
text = "\n".join(lines) + "\n"
print(text)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text)
