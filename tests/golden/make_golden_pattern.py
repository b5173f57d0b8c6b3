"""Golden vectors of pattern scanning, recorded by RUNNING THE REFERENCE'S OWN NETS on CPU.

Run in the build container only (needs the reference, imported through tests/golden/_ref_import.py like make_golden.py):

    python tests/golden/make_golden_pattern.py g42 g43

The reference's design.evolve(method="pattern") enumerates its mutants with grelu's MotifScanDataset, which is not installed in
the build container and cannot be run. This script is therefore a RESTATEMENT of that enumeration, not a recording of it (DESIGN
4r; as make_golden_ism.py restated ISMDataset): sequence, then start position, then pattern (the pattern index runs fastest), each
mutant the sequence with x[pos : pos + w] overwritten by the pattern — a replacement, the length stays L. It calls the reference's
`head(embedding(.))` (Enformer.ConvGRUTrunk / ConvHead, eval mode) on every mutant, ONE AT A TIME, a mutant that equals its parent
included, so that no batching or short cut of this project's choosing enters the recorded numbers. Per file:

  x          [B, L] u8: the sequences (torch.randint under `seed`)
  positions  [P] i32, ascending start positions
  patterns   [K, 32] u8 zero padded, widths [K] i32; the LAST pattern is a slice of x[0], so that one mutant is a copy
  copy_at    i32: the index into positions at which that pattern is already there in row 0
  parent     [B] f32: head(embedding(onehot(x[b])))
  table      [B, P, K] f32: entry (b, j, k) = the score of x[b] with pattern k written at positions[j]

  g42_pattern_tiny.npz   the 8-channel value net of make_golden.py (tiny_value), L = 50, B = 4, patterns of widths 1, 4 and 9,
                         9 positions (0 and L - 9 among them)
  g43_pattern_full.npz   the full-size seed-44 value net (synthetic.build's classes and order), L = 200, B = 2, patterns of widths 6,
                         13 and 32, 24 positions (0 and L - 32 among them); parameter checksums as in g37

No evolve trajectory is recorded: at a near-tie of two mutants' scores the pick would depend on rounding, so the trajectory is held
exactly by the evolve_patterns_ref tests instead (tests/pattern_ref.py).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import full_nets, save, tiny_value  # noqa: E402


def record(emb, head, B, L, positions, widths, copy_at, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 4, (B, L), generator=g)
    pats = [torch.randint(0, 4, (w,), generator=g) for w in widths[:-1]]
    pats.append(x[0, positions[copy_at]:positions[copy_at] + widths[-1]].clone())       # already there in row 0
    score = lambda row: float(head(emb(torch.nn.functional.one_hot(row[None], 4).float())).reshape(-1)[0])   # noqa: E731
    table = np.empty((B, len(positions), len(pats)), np.float32)
    parent = np.empty(B, np.float32)
    with torch.no_grad():
        for b in range(B):
            parent[b] = score(x[b])
            for j, pos in enumerate(positions):
                for k, pat in enumerate(pats):                                  # sequence, position, pattern
                    row = x[b].clone()
                    row[pos:pos + len(pat)] = pat
                    assert len(row) == L
                    table[b, j, k] = score(row)
    assert table[0, copy_at, -1] == parent[0]                                   # the same call on the same tokens
    eff = np.abs(table - parent[:, None, None])
    print(f"B={B} L={L} P={len(positions)} K={len(pats)}: mean |mutant - parent| {eff.mean():.3e}, max {eff.max():.3e}, parent {parent}")
    packed = np.zeros((len(pats), 32), np.uint8)
    for k, pat in enumerate(pats):
        packed[k, :len(pat)] = pat.numpy()
    return dict(seed=seed, x=x.to(torch.uint8), positions=np.asarray(positions, np.int32), patterns=packed,
                widths=np.asarray(widths, np.int32), copy_at=np.int32(copy_at), parent=parent, table=table)


def g42():
    emb, head = tiny_value()
    save("g42_pattern_tiny.npz", **record(emb, head, 4, 50, [0, 1, 7, 15, 16, 30, 33, 40, 41], [1, 4, 9], 4, 62))


def g43():
    _, emb, head = full_nets(length=200)
    arrs = {n_ + "_param_sums": np.array([float(p.double().sum()) for p in mod.state_dict().values()])
            for n_, mod in (("embedding", emb), ("head", head))}
    pos = [0, 1, 5, 15, 16, 17, 31, 32, 48, 63, 64, 80, 95, 96, 100, 111, 112, 127, 128, 143, 150, 160, 167, 168]
    save("g43_pattern_full.npz", net_seed=44, **arrs, **record(emb, head, 2, 200, pos, [6, 13, 32], 9, 63))


if __name__ == "__main__":
    torch.set_num_threads(int(os.environ.get("SVDD_GOLDEN_THREADS", "8")))
    for arg in sys.argv[1:]:
        {"g42": g42, "g43": g43}[arg]()
