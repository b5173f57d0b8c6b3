"""Golden vectors of in-silico mutagenesis, recorded by RUNNING THE REFERENCE'S OWN NETS on CPU.

Run in the build container only (needs the reference, imported through tests/golden/_ref_import.py like make_golden.py):

    python tests/golden/make_golden_ism.py g36 g37

The reference's score.ISM_predict and design.evolve(method="ism") enumerate the mutants with grelu's ISMDataset, which is not
installed in the build container. This script therefore RESTATES the enumeration order of ISMDataset(..., drop_ref=True) —
sequence, then position, then allele in ACGT order with the sequence's own base skipped — and calls the reference's
`head(embedding(.))` (Enformer.ConvGRUTrunk / ConvHead, eval mode) on every mutant, ONE AT A TIME, so that no batching of this
project's choosing enters the recorded numbers. Per file:

  x          [B, L] u8: the sequences (torch.randint under `seed`)
  positions  [P] i32, ascending
  parent     [B] f32: head(embedding(onehot(x[b])))
  ism        [B, P, 4] f32: entry (b, j, a) = the score of x[b] with base a at positions[j]; the entry of the sequence's own base is
             parent[b]

  g36_ism_tiny.npz   the 8-channel value net of make_golden.py (tiny_value), L = 50, B = 4, 9 positions (0 and L - 1 among them)
  g37_ism_full.npz   the full-size seed-44 value net (synthetic.build's classes and order), L = 200, B = 2, all 200 positions;
                     parameter checksums as in g35

No evolve trajectory is recorded: at a near-tie of two mutants' scores the pick would depend on rounding, so the trajectory is held
exactly by the evolve_ref tests instead (tests/ism_ref.py).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import full_nets, save, tiny_value  # noqa: E402


def record(emb, head, B, L, positions, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 4, (B, L), generator=g)
    score = lambda row: float(head(emb(torch.nn.functional.one_hot(row[None], 4).float())).reshape(-1)[0])   # noqa: E731
    ism = np.empty((B, len(positions), 4), np.float32)
    parent = np.empty(B, np.float32)
    with torch.no_grad():
        for b in range(B):
            parent[b] = score(x[b])
            for j, pos in enumerate(positions):
                ism[b, j, int(x[b, pos])] = parent[b]
                for a in range(4):                                              # ACGT order, the sequence's own base skipped
                    if a == int(x[b, pos]):
                        continue
                    row = x[b].clone()
                    row[pos] = a
                    ism[b, j, a] = score(row)
    eff = np.abs(ism - parent[:, None, None])
    print(f"B={B} L={L} P={len(positions)}: mean |mutant - parent| {eff.mean():.3e}, max {eff.max():.3e}, parent {parent}")
    return dict(seed=seed, x=x.to(torch.uint8), positions=np.asarray(positions, np.int32), parent=parent, ism=ism)


def g36():
    emb, head = tiny_value()
    save("g36_ism_tiny.npz", **record(emb, head, 4, 50, [0, 1, 7, 16, 17, 31, 32, 48, 49], 60))


def g37():
    _, emb, head = full_nets(length=200)
    arrs = {n_ + "_param_sums": np.array([float(p.double().sum()) for p in mod.state_dict().values()])
            for n_, mod in (("embedding", emb), ("head", head))}
    save("g37_ism_full.npz", net_seed=44, **arrs, **record(emb, head, 2, 200, list(range(200)), 61))


if __name__ == "__main__":
    torch.set_num_threads(int(os.environ.get("SVDD_GOLDEN_THREADS", "8")))
    for arg in sys.argv[1:]:
        {"g36": g36, "g37": g37}[arg]()
