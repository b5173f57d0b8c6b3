"""Timing of the sample-quality kernels (svdd_amd/quality.py) on synthetic data, in one process: B = 2048 designs of
L = 200 against a seeded random database of N = 2^19 rows. Median and minimum of --reps calls timed with device events after one
warm-up each:
  (a) nearest neighbour + histogram of all B N pairs through svdd_pack_tokens (both sides, every call) and svdd_hamming_nn;
  (b) the same two results composed from torch ops on the unpacked tokens (x[:, None] != db[None], summed; min over keys;
      bincount), in database chunks of --torch_chunk rows so that the [B, chunk, L] comparison fits; asserted EQUAL to (a);
  (c) svdd_kmer_counts of the database at k = 3 and k = 6 against torch.bincount on unfolded windows (in row chunks), asserted equal.
Run it under a time limit: timeout -k 10 900 python tools/quality_time.py
Usage: python tools/quality_time.py [--reps 5] [--torch_reps 3] [--out profiles/quality_time.txt] [--note TEXT ...]"""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from svdd_amd import ops, quality

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--torch_reps", type=int, default=3)
ap.add_argument("--designs", type=int, default=2048)
ap.add_argument("--db_rows", type=int, default=1 << 19)
ap.add_argument("--torch_chunk", type=int, default=4096)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quality_time.txt"))
ap.add_argument("--note", action="append", default=[])
args = ap.parse_args()

B, N, L = args.designs, args.db_rows, 200
DEV = "cuda:0"
gen = torch.Generator().manual_seed(0)
x = torch.randint(0, 4, (B, L), generator=gen).to(torch.uint8).to(DEV)
db = torch.randint(0, 4, (N, L), generator=gen).to(torch.uint8).to(DEV)
db[N // 3] = x[5]                                       # one memorised design, so that the minimum is not only far ties
db[N // 2] = db[7] = x[9]


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


def kernels():
    """(a): pack both sides, one svdd_hamming_nn over the whole database -> (nn_key, hist)."""
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    q, d = ops.pack_tokens(x, err=err), ops.pack_tokens(db, err=err)
    key = torch.full((B,), ops.NN_KEY_INIT, dtype=torch.int64, device=DEV)
    hist = torch.zeros(L + 1, dtype=torch.int64, device=DEV)
    return ops.hamming_nn(q, d, L, key, hist)


def kernel_alone():
    q, d = ops.pack_tokens(x), ops.pack_tokens(db)
    key = torch.full((B,), ops.NN_KEY_INIT, dtype=torch.int64, device=DEV)
    hist = torch.zeros(L + 1, dtype=torch.int64, device=DEV)
    both = timed(lambda: ops.hamming_nn(q, d, L, key, hist), args.reps)
    only_key = timed(lambda: ops.hamming_nn(q, d, L, key, None), args.reps)
    pack = timed(lambda: (ops.pack_tokens(x, err=torch.zeros(1, dtype=torch.int32, device=DEV)),
                          ops.pack_tokens(db, err=torch.zeros(1, dtype=torch.int32, device=DEV))), args.reps)
    return both, only_key, pack


def composed():
    """(b): the same key and histogram from torch ops on unpacked tokens, database chunk by chunk."""
    key = torch.full((B,), torch.iinfo(torch.int64).max, dtype=torch.int64, device=DEV)
    hist = torch.zeros(L + 1, dtype=torch.int64, device=DEV)
    for r0 in range(0, N, args.torch_chunk):
        c = db[r0:r0 + args.torch_chunk]
        d = (x[:, None, :] != c[None, :, :]).sum(-1)                                     # [B, chunk] i64
        key = torch.minimum(key, ((d << 32) | (r0 + torch.arange(c.shape[0], device=DEV))).min(1).values)
        hist += torch.bincount(d.reshape(-1), minlength=L + 1)
    return key, hist


def kmer_torch(k, rows=1 << 16):
    w = 4 ** torch.arange(k - 1, -1, -1, device=DEV)
    counts = torch.zeros(4 ** k, dtype=torch.int64, device=DEV)
    for r0 in range(0, N, rows):
        bins = (db[r0:r0 + rows].unfold(1, k, 1).long() * w).sum(-1)
        counts += torch.bincount(bins.reshape(-1), minlength=4 ** k)
    return counts


def kmer_kernel(k):
    counts = torch.zeros(4 ** k, dtype=torch.int64, device=DEV)
    return ops.kmer_counts(db, k, counts)[0]


a_med, a_min = timed(kernels, args.reps)
(h_med, h_min), (k_med, k_min), (p_med, p_min) = kernel_alone()
b_med, b_min = timed(composed, args.torch_reps)
(ka, ha), (kb, hb) = kernels(), composed()
assert torch.equal(ka, kb) and torch.equal(ha, hb), "the kernels and the torch composition disagree"
dist, idx = ops.nn_decode(ka)
assert int(dist[5]) == 0 and int(idx[5]) == N // 3 and int(dist[9]) == 0 and int(idx[9]) == 7 and int(ha.sum()) == B * N
pairs = B * N
lines = [f"Sample-quality timing: B = {B} designs, L = {L}, seeded random database of N = {N} rows = {pairs:.3e} pairs, {pairs * L:.3e} base "
         f"comparisons; median of {args.reps} ({args.torch_reps} for the torch compositions) (minimum in brackets), device events, one warm-up each",
         f"device: {torch.cuda.get_device_name(0)}", "",
         f"(a) svdd_pack_tokens (both sides) + svdd_hamming_nn, key and histogram: {a_med:10.2f} ms [{a_min:.2f}] = {pairs / a_med / 1e6:.1f} G pairs/s",
         f"    svdd_hamming_nn alone: key + histogram {h_med:.2f} ms [{h_min:.2f}], key only {k_med:.2f} ms [{k_min:.2f}]; packing alone {p_med:.3f} ms [{p_min:.3f}]",
         f"(b) torch ops on unpacked tokens, database chunks of {args.torch_chunk} rows:    {b_med:10.2f} ms [{b_min:.2f}]",
         f"    (a) : (b) = {a_med / b_med:.4f} ((b) is {b_med / a_med:.1f} x (a)); nn_key and histogram equal: True"]
for k in (3, 6):
    assert torch.equal(kmer_kernel(k), kmer_torch(k)), f"k-mer counts disagree at k = {k}"
    c_med, c_min = timed(lambda: kmer_kernel(k), args.reps)
    t_med, t_min = timed(lambda: kmer_torch(k), args.torch_reps)
    lines.append(f"(c) k = {k}: svdd_kmer_counts of the {N} database rows {c_med:8.3f} ms [{c_min:.3f}] = {N * L / c_med / 1e6:.1f} GB/s of tokens; "
                 f"torch unfold + bincount {t_med:8.2f} ms [{t_min:.2f}] ({t_med / c_med:.1f} x); counts equal: True")
lines.append("")
lines += args.note
text = "\n".join(lines) + "\n"
print(text)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text)
