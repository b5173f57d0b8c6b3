"""Timing of the edit-distance kernel (svdd_amd/quality.py edit_nn) on synthetic data, in one process: B = 2048 designs
of L = 200 against a seeded random database of N = 2^19 rows, a few of the designs being database rows shifted by 1 .. 8. Median
and minimum of --reps calls timed with device events after one warm-up each:
  (a) quality.edit_nn with cap = 20, seeded from the Hamming pass and not, and with the full cap (packing included);
  (b) quality.pairwise_edit_hist with cap = 20 and with the full cap;
  (c) svdd_edit_nn alone on packed rows: with the histogram at the full cap no pair can be left early, so this is the cost of the
      recurrence itself, reported per pair and database column; with the key only, what the early exit leaves of it;
  (d) on the first --torch_rows database rows, the same key and histogram composed from torch ops on the unpacked tokens (the
      table column by column for all pairs of a chunk at once, the in-column chain by cummin), asserted EQUAL to the kernel's.
Run it under a time limit: timeout -k 10 900 python tools/edit_time.py
Usage: python tools/edit_time.py [--reps 3] [--torch_rows 2048] [--out profiles/edit_time.txt] [--note TEXT ...]"""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from svdd_amd import ops, quality

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--designs", type=int, default=2048)
ap.add_argument("--db_rows", type=int, default=1 << 19)
ap.add_argument("--torch_rows", type=int, default=2048)
ap.add_argument("--torch_chunk", type=int, default=256)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edit_time.txt"))
ap.add_argument("--note", action="append", default=[])
args = ap.parse_args()

B, N, L, CAP = args.designs, args.db_rows, 200, 20
DEV = "cuda:0"
gen = torch.Generator().manual_seed(0)
x = torch.randint(0, 4, (B, L), generator=gen).to(torch.uint8)
db = torch.randint(0, 4, (N, L), generator=gen).to(torch.uint8)
PLANTED = {}                                            # design -> (database row, shift)
for n in range(32):                                     # 32 designs are database rows moved by 1 .. 8 positions, random fill
    i, s = (B // 32) * n + 3, 1 + n % 8
    j = (N // 32) * n + 5 if n % 4 else 37 * n + 11     # every fourth inside the first --torch_rows rows
    x[i] = torch.cat([db[j][s:], torch.randint(0, 4, (s,), generator=gen).to(torch.uint8)])
    PLANTED[i] = (j, s)
x, db = x.to(DEV), db.to(DEV)


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


def fresh_key():
    return torch.full((B,), ops.NN_KEY_INIT, dtype=torch.int64, device=DEV)


def fresh_hist(cap):
    return torch.zeros(cap + 2, dtype=torch.int64, device=DEV)


def composed(rows):
    """(d): key and histogram at the full cap from torch ops on unpacked tokens, the first `rows` database rows chunk by chunk."""
    key = torch.full((B,), torch.iinfo(torch.int64).max, dtype=torch.int64, device=DEV)
    hist = fresh_hist(L)
    ar = torch.arange(L + 1, dtype=torch.int32, device=DEV)
    for r0 in range(0, rows, args.torch_chunk):
        c = db[r0:min(r0 + args.torch_chunk, rows)]
        col = ar.expand(B, c.shape[0], L + 1).contiguous()
        for j in range(L):
            t = torch.empty_like(col)
            t[..., 0] = j + 1
            t[..., 1:] = torch.minimum(col[..., :-1] + (x[:, None, :] != c[None, :, j, None]), col[..., 1:] + 1)
            col = torch.cummin(t - ar, dim=-1).values + ar
        d = col[..., L].long()
        key = torch.minimum(key, ((d << 32) | (r0 + torch.arange(c.shape[0], device=DEV))).min(1).values)
        hist += torch.bincount(d.reshape(-1), minlength=L + 2)
    return key, hist


q, d = ops.pack_tokens(x), ops.pack_tokens(db)
pairs = B * N
res = {}
res["nn20_seeded"] = timed(lambda: quality.edit_nn(x, db, cap=CAP), args.reps)
res["nn20_plain"] = timed(lambda: quality.edit_nn(x, db, cap=CAP, seed_hamming=False), args.reps)
res["nn_full"] = timed(lambda: quality.edit_nn(x, db), args.reps)
res["nn_full_plain"] = timed(lambda: quality.edit_nn(x, db, seed_hamming=False), args.reps)
res["hist20"] = timed(lambda: quality.pairwise_edit_hist(x, db, cap=CAP), args.reps)
res["hist_full"] = timed(lambda: quality.pairwise_edit_hist(x, db), args.reps)
res["k_hist_full"] = timed(lambda: ops.edit_nn(q, d, L, L, L, None, fresh_hist(L)), args.reps)
res["k_key20"] = timed(lambda: ops.edit_nn(q, d, L, L, CAP, fresh_key(), None), args.reps)
res["k_key_full"] = timed(lambda: ops.edit_nn(q, d, L, L, L, fresh_key(), None), args.reps)
res["hamming"] = timed(lambda: ops.hamming_nn(q, d, L, fresh_key(), None), args.reps)

# the results: seeded == unseeded, the planted copies are found at twice their shift or less, hist and key agree with each other
a, b = quality.edit_nn(x, db, cap=CAP), quality.edit_nn(x, db, cap=CAP, seed_hamming=False)
assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), "seeding changed the result"
full = quality.edit_nn(x, db)
assert bool(((a[0] < 0) | ((a[0] == full[0]) & (a[1] == full[1]))).all()) and bool((full[0][a[0] < 0] > CAP).all())
for i, (j, s) in PLANTED.items():
    assert 0 <= int(a[0][i]) <= 2 * s and (int(a[1][i]) == j or int(a[0][i]) < 2 * s), (i, j, s, int(a[0][i]), int(a[1][i]))
near = int((a[0] >= 0).sum())
h20, hfull = quality.pairwise_edit_hist(x, db, cap=CAP), quality.pairwise_edit_hist(x, db)
assert int(h20.sum()) == pairs == int(hfull.sum()) and torch.equal(h20[:CAP + 1], hfull[:CAP + 1]) and int(hfull[L + 1]) == 0
hd = quality.hamming_nn(x, db)[0]
missed = int(((a[0] >= 0) & (hd > CAP)).sum())

R = args.torch_rows
dR = d[:R].contiguous()
t_med, t_min = timed(lambda: composed(R), 1)
kk, kh = ops.edit_nn(q, dR, L, L, L, fresh_key(), fresh_hist(L))
ck, ch = composed(R)
assert torch.equal(kk, ck) and torch.equal(kh, ch), "the kernel and the torch composition disagree"
s_med, s_min = timed(lambda: ops.edit_nn(q, dR, L, L, L, fresh_key(), fresh_hist(L)), args.reps)

ms = lambda k: f"{res[k][0]:10.2f} ms [{res[k][1]:.2f}]"                                    # noqa: E731
cols = pairs * L
full_ms = res["k_hist_full"][0]
lines = [f"Edit-distance timing: B = {B} designs, L = {L}, seeded random database of N = {N} rows = {pairs:.3e} pairs, {cols:.3e} pair-columns; "
         f"{len(PLANTED)} designs are database rows shifted by 1 .. 8; median of {args.reps} (minimum in brackets), device events, one warm-up each",
         f"device: {torch.cuda.get_device_name(0)}", "",
         f"(a) quality.edit_nn, cap = {CAP}, seeded by the Hamming pass:   {ms('nn20_seeded')}",
         f"    quality.edit_nn, cap = {CAP}, not seeded:                  {ms('nn20_plain')}   (seeded : not = {res['nn20_seeded'][0] / res['nn20_plain'][0]:.3f})",
         f"    quality.edit_nn, full cap ({L}), seeded:                  {ms('nn_full')}",
         f"    quality.edit_nn, full cap ({L}), not seeded:              {ms('nn_full_plain')}   (seeded : not = {res['nn_full'][0] / res['nn_full_plain'][0]:.3f})",
         f"(b) quality.pairwise_edit_hist, cap = {CAP}:                    {ms('hist20')}",
         f"    quality.pairwise_edit_hist, full cap:                    {ms('hist_full')}   (cap {CAP} : full = {res['hist20'][0] / res['hist_full'][0]:.3f})",
         f"(c) svdd_edit_nn alone, histogram at the full cap (no pair left early): {ms('k_hist_full')} = {full_ms * 1e9 / cols:.4f} ps per "
         f"pair-column, {full_ms / 1e3 * 1e9 / pairs:.3f} s per 1e9 pairs",
         f"    svdd_edit_nn alone, key only, cap = {CAP}, fresh key:   {ms('k_key20')}   (: the full recurrence = {res['k_key20'][0] / full_ms:.3f})",
         f"    svdd_edit_nn alone, key only, full cap, fresh key:  {ms('k_key_full')}   (: the full recurrence = {res['k_key_full'][0] / full_ms:.3f})",
         f"    svdd_hamming_nn alone, key only (the seed pass):     {ms('hamming')}",
         f"(d) the first {R} database rows ({B * R:.3e} pairs), key and histogram at the full cap: svdd_edit_nn {s_med:.2f} ms [{s_min:.2f}], torch ops on "
         f"unpacked tokens in chunks of {args.torch_chunk} rows {t_med:.1f} ms (one timed run): torch is {t_med / s_med:.0f} x; nn_key and histogram equal: True",
         "",
         f"results: {near} of {B} designs have a database row within {CAP} edits (all {len(PLANTED)} planted ones, each at most twice its shift away); "
         f"{missed} of them have their nearest row by Hamming beyond {CAP}; seeded and unseeded keys equal; histograms sum to B N", ""]
lines += args.note
text = "\n".join(lines) + "\n"
print(text)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text)
