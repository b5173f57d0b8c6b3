"""Timing of diverse library selection under a minimum EDIT distance (svdd_amd/quality.py select_diverse_edit) on
synthetic data, in one process: N = 65,536 planted-family designs of L = 200 (2048 random founders; a row is a founder that is an
exact copy (15 %), a pure shift by 1 .. 3 bases at either end (20 %), or carries 0 .. 8 substitutions, insertions and deletions;
25 % of the rows reverse-complemented), min_dist = 20. Median and minimum of --reps calls timed with device events after one
warm-up each:
  (a) quality.select_diverse_edit with k = None and k = 1000, one strand and both, at the default block_rows;
  (b) the share of svdd_edit_within and of svdd_greedy_pick in (a), from their named profile slots (a run of its own);
  (c) the block_rows sweep that fixes the default;
  (d) svdd_edit_within alone next to svdd_edit_nn (key only, cap = min_dist - 1) and svdd_within on the same pairs (--pair_rows
      queries against all N rows), and what the second strand costs;
  (e) the same picks composed from what was public before: a host walk in rank order that discards a block's rows with
      quality.edit_nn(block, picks so far, cap = min_dist - 1) and settles the rest row by row, on the first --composed_rows rows,
      one strand; picks asserted EQUAL, one timed run;
  (f) how many of the planted shifted copies the Hamming selection (quality.select_diverse) keeps as picks of their own, and how
      many the edit selection keeps.
Run it under a time limit: timeout -k 10 900 python tools/select_edit_time.py
Usage: python tools/select_edit_time.py [--reps 3] [--rows 65536] [--out profiles/select_edit_time.txt] [--note TEXT ...]"""
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
ap.add_argument("--composed_rows", type=int, default=8192)
ap.add_argument("--sweep", default="256,512,1024,2048,4096")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select_edit_time.txt"))
ap.add_argument("--note", action="append", default=[])
args = ap.parse_args()

N, F, L, MAX_EDIT, MIN_DIST, K = args.rows, args.founders, 200, 8, 20, 1000
DEV = "cuda:0"
SLOT_PICK, SLOT_EDIT_WITHIN = 14, 15                               # enum SvddProfileSlot (csrc/svdd_host.h)
rng = np.random.default_rng(0)
founders = rng.integers(0, 4, (F, L))
fam = rng.integers(0, F, N)
kind = rng.random(N)
is_copy, is_shift = kind < 0.15, (kind >= 0.15) & (kind < 0.35)
ne = rng.integers(0, MAX_EDIT + 1, N)
ne[is_copy | is_shift] = 0
etype, epos = rng.integers(0, 3, (N, MAX_EDIT)), rng.integers(0, L, (N, MAX_EDIT))       # 0 substitution, 1 insertion, 2 deletion
live = np.arange(MAX_EDIT)[None, :] < ne[:, None]
row_of = np.broadcast_to(np.arange(N)[:, None], (N, MAX_EDIT))
step = np.zeros((N, L), np.int64)                                  # position l reads the founder at l + the running sum of step
np.add.at(step, (row_of[live & (etype == 2)], epos[live & (etype == 2)]), 1)
np.add.at(step, (row_of[live & (etype == 1)], epos[live & (etype == 1)]), -1)
off = np.cumsum(step, 1)
off[is_shift] += (rng.integers(1, 4, N) * np.where(rng.random(N) < 0.5, 1, -1))[is_shift, None]
src = np.arange(L)[None, :] + off
x = np.where((src >= 0) & (src < L), founders[fam[:, None], np.clip(src, 0, L - 1)], rng.integers(0, 4, (N, L)))
ins = live & (etype == 1)
x[row_of[ins], epos[ins]] = rng.integers(0, 4, int(ins.sum()))     # the inserted base
sub = live & (etype == 0)
x[row_of[sub], epos[sub]] = (x[row_of[sub], epos[sub]] + rng.integers(1, 4, int(sub.sum()))) % 4
flip = rng.random(N) < 0.25
x[flip] = (3 - x[flip])[:, ::-1]
# a few high-reward modes: a founder's quality, minus a little per edit, plus noise
scores = (rng.standard_normal(F)[fam] - 0.05 * ne + 0.1 * rng.standard_normal(N)).astype(np.float32)
x, scores = torch.from_numpy(x.astype(np.uint8)).to(DEV), torch.from_numpy(scores).to(DEV)
is_shift = torch.from_numpy(is_shift).to(DEV)


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


def composed(xs, ss, T):
    """(e): the picks from quality.edit_nn alone (one strand) -> picked i64, in pick order."""
    n = xs.shape[0]
    order = torch.sort(ss, descending=True, stable=True).indices
    xr = xs[order]
    picks = []                                                     # ranks
    for r0 in range(0, n, T):
        blk = xr[r0:r0 + T]
        t = blk.shape[0]
        settled = np.zeros(t, bool)
        if picks:
            settled = (quality.edit_nn(blk, xr[torch.as_tensor(picks, device=DEV)], cap=MIN_DIST - 1)[0] >= 0).cpu().numpy()
        mine = []
        for i in np.nonzero(~settled)[0]:
            if mine and int(quality.edit_nn(blk[i:i + 1], blk[torch.as_tensor(mine, device=DEV)], cap=MIN_DIST - 1)[0][0]) >= 0:
                continue
            mine.append(int(i))
        picks += [r0 + i for i in mine]
    return order[torch.as_tensor(picks, dtype=torch.int64, device=DEV)]


T0 = quality.SELECT_EDIT_BLOCK_ROWS
res, sel = {}, {}
for k in (None, K):
    for rc in (False, True):
        res[k, rc] = timed(lambda: sel.__setitem__((k, rc), quality.select_diverse_edit(x, scores, k, MIN_DIST, rc)), args.reps)

share = {}
for k, rc in ((None, False), (None, True)):
    torch.cuda.synchronize()
    for s in (SLOT_EDIT_WITHIN, SLOT_PICK):
        _lib.profile_collect(s)
    _lib.profile_enable(True)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    quality.select_diverse_edit(x, scores, k, MIN_DIST, rc)
    e1.record()
    e1.synchronize()
    _lib.profile_enable(False)
    share[k, rc] = (e0.elapsed_time(e1), _lib.profile_collect(SLOT_EDIT_WITHIN), _lib.profile_collect(SLOT_PICK))

sweep = {}
for T in [int(t) for t in args.sweep.split(",")]:
    for rc in (False, True):
        got = []
        sweep[T, rc] = timed(lambda: got.append(quality.select_diverse_edit(x, scores, None, MIN_DIST, rc, T)), args.reps)
        assert all(torch.equal(a, b) for a, b in zip(got[-1], sel[None, rc])), (T, rc)      # block_rows changes nothing

B = args.pair_rows
q, d = ops.pack_tokens(x[:B]), ops.pack_tokens(x)
pairs = B * N
mw = (N + 31) // 32
first = torch.full((B,), ops.FIRST_INIT, dtype=torch.int32, device=DEV)
mask = torch.empty((B, mw), dtype=torch.int32, device=DEV)


def fresh_key():
    return torch.full((B,), ops.NN_KEY_INIT, dtype=torch.int64, device=DEV)


R = MIN_DIST - 1
pair = {"svdd_within (Hamming), first and mask": timed(lambda: ops.within(q, d, L, R, first=first, mask=mask), args.reps),
        f"svdd_edit_nn, key only, cap = {R}, fresh key": timed(lambda: ops.edit_nn(q, d, L, L, R, fresh_key(), None), args.reps),
        "svdd_edit_within, first only": timed(lambda: ops.edit_within(q, d, L, R, first=first), args.reps),
        "svdd_edit_within, mask only": timed(lambda: ops.edit_within(q, d, L, R, mask=mask), args.reps),
        "svdd_edit_within, first and mask": timed(lambda: ops.edit_within(q, d, L, R, first=first, mask=mask), args.reps),
        "svdd_edit_within, both strands, first and mask": timed(lambda: ops.edit_within(q, d, L, R, True, first=first, mask=mask), args.reps)}
second = pair["svdd_edit_within, both strands, first and mask"][0] / pair["svdd_edit_within, first and mask"][0]

C = min(args.composed_rows, N)
small = quality.select_diverse_edit(x[:C], scores[:C], None, MIN_DIST, False)
small_ms = timed(lambda: quality.select_diverse_edit(x[:C], scores[:C], None, MIN_DIST, False), args.reps)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
torch.cuda.synchronize()
e0.record()
picked = composed(x[:C], scores[:C], T0)
e1.record()
e1.synchronize()
composed_ms = e0.elapsed_time(e1)
equal = torch.equal(picked, small.picked)
assert equal

kept = {}
for rc in (False, True):
    ham = quality.select_diverse(x, scores, None, MIN_DIST, rc)
    kept[rc] = (int(is_shift[ham.picked].sum()), ham.picked.numel(), int(is_shift[sel[None, rc].picked].sum()), sel[None, rc].picked.numel())

name = lambda k, rc: f"k = {'None' if k is None else k}, {'both strands' if rc else 'one strand'}"     # noqa: E731
ms = lambda t: f"{t[0]:9.2f} ms [{t[1]:.2f}]"                                                           # noqa: E731
lines = [f"{torch.cuda.get_device_name(0)}; N = {N} planted-family designs (F = {F} founders; 15 % copies, 20 % shifts by 1 .. 3, else <= "
         f"{MAX_EDIT} substitutions / insertions / deletions; 25 % reverse-complemented), L = {L}, min_dist = {MIN_DIST} edits; median "
         f"[minimum] of {args.reps} runs after one warm-up, device events",
         f"(a) quality.select_diverse_edit, block_rows = {T0} (sort, packing, gather and rep_dist included):"]
lines += [f"    {name(k, rc):28s} {ms(res[k, rc])}   picks {sel[k, rc].picked.numel():6d}   rows without a representative "
          f"{int((sel[k, rc].rep < 0).sum())}" for k, rc in res]
lines.append("(b) one profiled run: total, and the sums over the launches of the two profile slots")
lines += [f"    {name(k, rc):28s} total {t:8.2f} ms; svdd_edit_within {w[0]:8.2f} ms in {w[1]} launches ({100 * w[0] / t:.0f} %); "
          f"svdd_greedy_pick {p[0]:8.2f} ms in {p[1]} launches ({100 * p[0] / t:.0f} %)" for (k, rc), (t, w, p) in share.items()]
lines.append("(c) block_rows sweep, k = None (every value gives the same selection: asserted):")
lines += [f"    block_rows {T:5d}   one strand {ms(sweep[T, False])}   both strands {ms(sweep[T, True])}" for T in sorted({t for t, _ in sweep})]
lines.append(f"(d) {B} queries against {N} rows = {pairs:.3e} pairs, radius {R}:")
lines += [f"    {what:48s} {ms(t)} = {pairs / t[0] / 1e6:8.2f} G pairs/s" for what, t in pair.items()]
lines.append(f"    the second strand: both strands = {second:.2f} x one strand")
lines.append(f"(e) the first {C} rows, one strand: composed from quality.edit_nn and a walk on the host (blocks of {T0}, one timed run) "
             f"{composed_ms:.1f} ms = {composed_ms / small_ms[0]:.0f} x select_diverse_edit's {small_ms[0]:.2f} ms; picks equal: {equal} "
             f"({small.picked.numel()} picks)")
lines.append(f"(f) planted shifted copies ({int(is_shift.sum())} of the {N} rows) among the picks, k = None:")
lines += [f"    {'both strands' if rc else 'one strand':14s} Hamming selection {h} of {hp} picks; edit selection {e} of {ep} picks"
          for rc, (h, hp, e, ep) in kept.items()]
lines += args.note
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text)
