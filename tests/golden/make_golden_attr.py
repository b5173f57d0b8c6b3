"""Golden vectors of gradient attributions, recorded by RUNNING THE REFERENCE'S OWN NETS on CPU in float64.

Run in the build container only (needs the reference, imported through tests/golden/_ref_import.py like make_golden.py):

    python tests/golden/make_golden_attr.py g38 g39

The reference's score.get_attributions wraps captum, which is not installed in the build container. Gradient and input x gradient
need nothing but autograd; for integrated gradients this script RESTATES captum's default rule — Gauss-Legendre nodes on [0, 1],
attr = (input - baseline) * sum_k w_k grad(baseline + alpha_k (input - baseline)) — around torch autograd through the reference's
`head(embedding(.))` (Enformer.ConvGRUTrunk / ConvHead, eval mode, cast to float64). The score is per row (the gradient of the sum
over the rows: a row's score depends on its own input only). Per file:

  x            [B, L] u8: the sequences (torch.randint under `seed`), a stretch of MASK (4) tokens in row 0: a zero one-hot row
  baseline     [L, 4] f32: the non-zero baseline (0.25 + seeded noise); the zero baseline is not stored
  alphas, weights  [S] f64: the quadrature
  gradient     [B, 4, L] f64: d score / d onehot at the one-hot
  inputxgradient  [B, 4, L] f64: onehot * gradient
  ig_zero, ig_base  [B, 4, L] f64: integrated gradients from the zero baseline / from `baseline`
  score_x [B], score_zero [B], score_base [B] f64: the scores of the inputs and of the two baselines
  delta_zero, delta_base  [B] f64: the completeness gap sum(attr) - (score_x - score_baseline)
  embedding_param_sums / head_param_sums: checksums of the nets' parameters, as in g37

  g38_attr_tiny.npz   the full-size seed-44 value net built for length 50 (the small shape: B = 2, L = 50, S = 5)
  g39_attr_full.npz   the same net built for length 200, B = 2, S = 50 (captum's default n_steps)

The input seeds. A ReLU whose float64 pre-activation lies within rounding of zero may be taken on either side by an fp32 evaluation,
and the gradient jumps there: tests/grad_ref.py calls a sequence with a tail pre-activation within 2e-6 of zero a tail-kink sequence
and lets a comparison exclude at most seq_cap(rows of the pass) of them. g39's 100 interpolants per table run as one pass of 128 rows
(cap 6). Its seed is the first from 63 on whose two tables both stay within that cap BY THE FLOAT64 REFERENCE ALONE (63: 6 and 11
sequences; 64: 3 and 5); tests/test_attr_cpu.py holds the cap for the recorded inputs. g38's ten interpolants have none.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import full_nets, save  # noqa: E402


def record(emb, head, B, L, S, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 4, (B, L), generator=g)
    x[0, L // 5: L // 5 + 7] = 4
    baseline = (0.25 + 0.05 * torch.randn(L, 4, generator=g)).float()
    emb, head = emb.double(), head.double()
    oh = (x[:, :, None] == torch.arange(4)).double()
    score = lambda t: head(emb(t)).reshape(t.shape[0], -1)[:, 0]                    # noqa: E731

    def grad_at(p):
        p = p.clone().requires_grad_(True)
        return torch.autograd.grad(score(p).sum(), p)[0]

    node, weight = np.polynomial.legendre.leggauss(S)
    alphas, weights = (1.0 + node) / 2.0, weight / 2.0
    out = dict(seed=seed, x=x.to(torch.uint8), baseline=baseline, alphas=alphas, weights=weights)
    g0 = grad_at(oh)
    out["gradient"], out["inputxgradient"] = g0.permute(0, 2, 1), (oh * g0).permute(0, 2, 1)
    with torch.no_grad():
        out["score_x"] = score(oh)
    for name, base in (("zero", torch.zeros(B, L, 4, dtype=torch.float64)), ("base", baseline.double().expand(B, L, 4))):
        acc = torch.zeros_like(oh)
        for a, w in zip(alphas, weights):
            acc = acc + float(w) * grad_at(base + float(a) * (oh - base))
        attr = ((oh - base) * acc).permute(0, 2, 1)
        with torch.no_grad():
            sb = score(base.contiguous())
        out["ig_" + name], out["score_" + name] = attr, sb
        out["delta_" + name] = attr.reshape(B, -1).sum(1) - (out["score_x"] - sb)
        print(f"B={B} L={L} S={S} baseline {name}: sum attr {attr.reshape(B, -1).sum(1).tolist()}, score_x - score_b "
              f"{(out['score_x'] - sb).tolist()}, gap {out['delta_' + name].tolist()}")
    return {k: (v.detach() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


def _full(name, L, S, seed):
    _, emb, head = full_nets(length=L)
    arrs = {n_ + "_param_sums": np.array([float(p.double().sum()) for p in mod.state_dict().values()])
            for n_, mod in (("embedding", emb), ("head", head))}
    save(name, net_seed=44, **arrs, **record(emb, head, 2, L, S, seed))


def g38():
    _full("g38_attr_tiny.npz", 50, 5, 62)


def g39():
    _full("g39_attr_full.npz", 200, 50, 64)


if __name__ == "__main__":
    torch.set_num_threads(int(os.environ.get("SVDD_GOLDEN_THREADS", "8")))
    for arg in sys.argv[1:]:
        {"g38": g38, "g39": g39}[arg]()
