"""Timing of diverse library selection (svdd_amd/quality.py select_diverse) on synthetic data, in one process: N = 65,536
planted-family designs of L = 200 (2048 random founders; a row is a founder with 0 .. 12 substitutions, 15 % exact copies, 25 % of
the rows reverse-complemented), min_dist = 20. Median and minimum of --reps calls timed with device events after one warm-up each:
  (a) quality.select_diverse with k = None and k = 1000, one strand and both, at the default block_rows;
  (b) the share of svdd_within and of svdd_greedy_pick in (a), from their named profile slots (a run of its own);
  (c) the block_rows sweep that fixes the default;
  (d) svdd_within alone next to svdd_hamming_nn on the same pairs (--pair_rows queries against all N rows);
  (e) the same selection composed from the earlier public pieces: torch comparisons on the unpacked tokens in the same blocks and
      the serial walk on the host, one round trip per block; asserted EQUAL to (a), one timed run.
Run it under a time limit: timeout -k 10 900 python tools/select_time.py
Usage: python tools/select_time.py [--reps 3] [--rows 65536] [--out profiles/select_time.txt] [--note TEXT ...]"""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from svdd_amd import _lib, ops, quality

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--rows", type=int, default=65536)
ap.add_argument("--founders", type=int, default=2048)
ap.add_argument("--pair_rows", type=int, default=8192)
ap.add_argument("--sweep", default="256,512,1024,2048,4096")
ap.add_argument("--torch_chunk", type=int, default=128)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select_time.txt"))
ap.add_argument("--note", action="append", default=[])
args = ap.parse_args()

N, F, L, MAX_SUB, MIN_DIST, K = args.rows, args.founders, 200, 12, 20, 1000
DEV = "cuda:0"
SLOT_WITHIN, SLOT_PICK = 13, 14                                    # enum SvddProfileSlot (csrc/svdd_host.h)
gen = torch.Generator().manual_seed(0)
founders = torch.randint(0, 4, (F, L), generator=gen)
fam = torch.randint(0, F, (N,), generator=gen)
nsub = torch.randint(0, MAX_SUB + 1, (N,), generator=gen)
nsub[torch.rand(N, generator=gen) < 0.15] = 0                      # exact copies
where = torch.rand(N, L, generator=gen).argsort(1).argsort(1) < nsub[:, None]        # nsub distinct positions per row
x = (founders[fam] + where * torch.randint(1, 4, (N, L), generator=gen)) % 4
flip = torch.rand(N, generator=gen) < 0.25
x[flip] = (3 - x[flip]).flip(1)
# a few high-reward modes: a founder's quality, minus a little per substitution, plus noise
scores = (torch.randn(F, generator=gen)[fam] - 0.05 * nsub + 0.1 * torch.randn(N, generator=gen)).float()
x, scores = x.to(torch.uint8).to(DEV), scores.to(DEV)


def timed(f, reps):
    """Median and minimum (ms) of f() over reps runs, each between two device events, after one warm-up."""
    f()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        f()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def composed(k, revcomp, T):
    """(e): the same blocks from torch ops on the unpacked tokens, the walk on the host -> (picked, rep) as select_diverse's."""
    order = torch.sort(scores, descending=True, stable=True).indices
    xs = x[order]
    cap = N if k is None else min(k, N)
    reps_tok = torch.empty((cap, L), dtype=torch.uint8, device=DEV)
    picked_rank, rep_pick, count = [], np.full(N, -1, np.int64), 0

    def close(a, b):
        out = torch.empty((a.shape[0], b.shape[0]), dtype=torch.bool, device=DEV)
        for c0 in range(0, a.shape[0], args.torch_chunk):
            c = a[c0:c0 + args.torch_chunk]
            d = (c[:, None, :] != b[None, :, :]).sum(-1)
            if revcomp:
                d = torch.minimum(d, ((3 - c).flip(1)[:, None, :] != b[None, :, :]).sum(-1))
            out[c0:c0 + args.torch_chunk] = d < MIN_DIST
        return out
    for r0 in range(0, N, T):
        blk = xs[r0:r0 + T]
        t = blk.shape[0]
        hit = close(blk, reps_tok[:count]) if count else torch.zeros((t, 1), dtype=torch.bool, device=DEV)
        col = torch.arange(hit.shape[1], device=DEV)
        first = torch.where(hit, col, N).min(1).values
        first = torch.where(first < N, first, -1).cpu().numpy()                                # the round trip
        own = close(blk, blk).cpu().numpy()
        sup, mine = np.full(t, -1, np.int64), []
        for i in range(t):
            if first[i] >= 0:
                rep_pick[r0 + i] = first[i]
            elif sup[i] >= 0:
                rep_pick[r0 + i] = sup[i]
            elif count < cap:
                rep_pick[r0 + i] = count
                new = own[i] & (sup < 0)
                new[:i + 1] = False
                sup[new] = count
                mine.append(i)
                picked_rank.append(r0 + i)
                count += 1
        if mine:
            reps_tok[count - len(mine):count] = blk[torch.as_tensor(mine, device=DEV)]
    picked = order[torch.as_tensor(picked_rank, dtype=torch.int64, device=DEV)]
    rep = torch.empty(N, dtype=torch.int64, device=DEV)
    rp = torch.as_tensor(rep_pick, device=DEV)
    rep[order] = torch.where(rp >= 0, picked[rp.clamp(min=0)], torch.full_like(rp, -1))
    return picked, rep


T0 = quality.SELECT_BLOCK_ROWS
res, sel = {}, {}
for k in (None, K):
    for rc in (False, True):
        res[k, rc] = timed(lambda: sel.__setitem__((k, rc), quality.select_diverse(x, scores, k, MIN_DIST, rc)), args.reps)

share = {}
for k, rc in ((None, False), (None, True)):
    torch.cuda.synchronize()
    for s in (SLOT_WITHIN, SLOT_PICK):
        _lib.profile_collect(s)
    _lib.profile_enable(True)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    quality.select_diverse(x, scores, k, MIN_DIST, rc)
    e1.record()
    e1.synchronize()
    _lib.profile_enable(False)
    share[k, rc] = (e0.elapsed_time(e1), _lib.profile_collect(SLOT_WITHIN), _lib.profile_collect(SLOT_PICK))

sweep = {}
for T in [int(t) for t in args.sweep.split(",")]:
    for rc in (False, True):
        got = []
        sweep[T, rc] = timed(lambda: got.append(quality.select_diverse(x, scores, None, MIN_DIST, rc, T)), args.reps)
        assert all(torch.equal(a, b) for a, b in zip(got[-1], sel[None, rc])), (T, rc)      # block_rows changes nothing

B = args.pair_rows
q, d = ops.pack_tokens(x[:B]), ops.pack_tokens(x)
q_rc = ops.pack_tokens((3 - x[:B]).flip(1).contiguous())
pairs = B * N
mw = (N + 31) // 32
first = torch.full((B,), ops.FIRST_INIT, dtype=torch.int32, device=DEV)
mask = torch.empty((B, mw), dtype=torch.int32, device=DEV)
key = torch.full((B,), ops.NN_KEY_INIT, dtype=torch.int64, device=DEV)
pair = {"svdd_hamming_nn, key only": timed(lambda: ops.hamming_nn(q, d, L, key, None), args.reps),
        "svdd_within, first only": timed(lambda: ops.within(q, d, L, MIN_DIST - 1, first=first), args.reps),
        "svdd_within, mask only": timed(lambda: ops.within(q, d, L, MIN_DIST - 1, mask=mask), args.reps),
        "svdd_within, first and mask": timed(lambda: ops.within(q, d, L, MIN_DIST - 1, first=first, mask=mask), args.reps),
        "svdd_within, both strands, first and mask": timed(lambda: ops.within(q, d, L, MIN_DIST - 1, q_rc=q_rc, first=first, mask=mask), args.reps)}

torch_ms, equal = {}, {}
for k, rc in ((None, False), (K, True)):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    picked, rep = composed(k, rc, T0)
    e1.record()
    e1.synchronize()
    torch_ms[k, rc] = e0.elapsed_time(e1)
    equal[k, rc] = torch.equal(picked, sel[k, rc].picked) and torch.equal(rep, sel[k, rc].rep)
    assert equal[k, rc], (k, rc)

name = lambda k, rc: f"k = {'None' if k is None else k}, {'both strands' if rc else 'one strand'}"     # noqa: E731
ms = lambda t: f"{t[0]:9.2f} ms [{t[1]:.2f}]"                                                           # noqa: E731
lines = [f"{torch.cuda.get_device_name(0)}; N = {N} planted-family designs (F = {F} founders, <= {MAX_SUB} substitutions), L = {L}, "
         f"min_dist = {MIN_DIST}; median [minimum] of {args.reps} runs after one warm-up, device events",
         f"(a) quality.select_diverse, block_rows = {T0} (sort, packing, gather and rep_dist included):"]
lines += [f"    {name(k, rc):28s} {ms(res[k, rc])}   picks {sel[k, rc].picked.numel():6d}   rows without a representative "
          f"{int((sel[k, rc].rep < 0).sum())}" for k, rc in res]
lines.append("(b) one profiled run: total, and the sums over the launches of the two profile slots")
lines += [f"    {name(k, rc):28s} total {t:8.2f} ms; svdd_within {w[0]:8.2f} ms in {w[1]} launches ({100 * w[0] / t:.0f} %); "
          f"svdd_greedy_pick {p[0]:8.2f} ms in {p[1]} launches ({100 * p[0] / t:.0f} %)" for (k, rc), (t, w, p) in share.items()]
lines.append("(c) block_rows sweep, k = None (every value gives the same selection: asserted):")
lines += [f"    block_rows {T:5d}   one strand {ms(sweep[T, False])}   both strands {ms(sweep[T, True])}" for T in sorted({t for t, _ in sweep})]
lines.append(f"(d) {B} queries against {N} rows = {pairs:.3e} pairs, radius {MIN_DIST - 1}:")
lines += [f"    {what:44s} {ms(t)} = {pairs / t[0] / 1e6:7.1f} G pairs/s" for what, t in pair.items()]
lines.append(f"(e) composed from torch comparisons on unpacked tokens (chunks of {args.torch_chunk} rows) and the walk on the host, blocks of {T0}, "
             "one timed run:")
lines += [f"    {name(k, rc):28s} {torch_ms[k, rc]:10.1f} ms = {torch_ms[k, rc] / res[k, rc][0]:.0f} x the kernels' {res[k, rc][0]:.2f} ms; "
          f"picked and rep equal: {equal[k, rc]}" for k, rc in torch_ms]
lines += args.note
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text)
