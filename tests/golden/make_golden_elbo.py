"""Golden vectors of the ELBO scoring path, recorded by RUNNING THE REFERENCE on CPU.

Run in the build container only (needs the reference, imported through tests/golden/_ref_import.py like make_golden.py):

    python tests/golden/make_golden_elbo.py g30 g31

The reference's `Diffusion._loss(x0, attention_mask)` (diffusion_gosai.py:1759-1779) with its live configuration (SUBS, T = 0,
time conditioning off, antithetic sampling, sampling_eps 1e-3) calls `_forward_pass_diffusion` (:1709-1757), which draws t with
`_sample_t` (:1660-1669: torch.rand(n)) and the mask with `q_xt` (:738-749: torch.rand(n, L)) from torch's global CPU generator.
`_sample_t` and `q_xt` are wrapped to record what they return; sigma, dsigma and w = dsigma / expm1(sigma) are the reference's own
noise schedule evaluated on the recorded t. Only inputs and outputs are stored. Per case (prefix `<case>_`):

  seed          torch.manual_seed before the first _loss call
  x0            [B, L] u8 clean tokens; attention_mask is all ones
  t, sigma, dsigma, w   [2, B] fp32: the first and the second of two consecutive _loss calls
  move_chance   [2, B] fp32 (the reference's [B, 1], squeezed)
  xt            [2, B, L] u8
  nlls          [2, B, L] fp32 (Loss.nlls) ; loss [2] fp32 (Loss.loss, sum / count)
  next1         [2] fp32: torch.rand(2) right after ONE _loss call (from the seed)
  next2         [2] fp32: torch.rand(2) right after TWO consecutive calls

  g30_elbo_tiny.npz   tiny nets of make_golden.py (hidden 16 x 1 stack), L = 50: `rand` (B = 8) and `short` (B = 3), random x0
  g31_elbo_full.npz   full-size seed-44 nets (synthetic.build's classes and order): `dna_rand` (L = 200, B = 64, random x0), `dna_dec`
                      (L = 200, B = 64, x0 = the first 64 decoded rows of g24_decode_sample_c2.npz), `rna_rand` (L = 50, B = 64)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import full_nets, save, tiny_diffusion  # noqa: E402


def record_case(d, x0, seed):
    """Two consecutive _loss calls after manual_seed(seed), and one call alone (for the generator's end state)."""
    rec = {"t": [], "mc": [], "xt": []}
    orig_t, orig_q = d._sample_t, d.q_xt

    def sample_t(n, device):
        t = orig_t(n, device)
        rec["t"].append(t.clone())
        return t

    def q_xt(x, move_chance):
        xt = orig_q(x, move_chance)
        rec["mc"].append(move_chance.reshape(-1).clone())
        rec["xt"].append(xt.to(torch.uint8).clone())
        return xt

    d._sample_t, d.q_xt = sample_t, q_xt
    mask = torch.ones(x0.shape)
    try:
        with torch.no_grad():
            torch.manual_seed(seed)
            out1 = d._loss(x0, mask)
            next1 = torch.rand(2)
            torch.manual_seed(seed)
            rec = {"t": [], "mc": [], "xt": []}
            a = d._loss(x0, mask)
            b = d._loss(x0, mask)
            next2 = torch.rand(2)
    finally:
        del d._sample_t, d.q_xt
    assert torch.equal(out1.nlls, a.nlls)
    t = torch.stack(rec["t"])
    sigma, dsigma = d.noise(t)
    w = dsigma / torch.expm1(sigma)
    return dict(seed=seed, x0=x0.to(torch.uint8), t=t, sigma=sigma, dsigma=dsigma, w=w, move_chance=torch.stack(rec["mc"]),
                xt=torch.stack(rec["xt"]), nlls=torch.stack([a.nlls, b.nlls]), loss=torch.stack([a.loss, b.loss]),
                next1=next1, next2=next2)


def _random_x0(B, L, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 4, (B, L), generator=g)


def _save(name, cases):
    arrs = {}
    for case, r in cases.items():
        arrs.update({f"{case}_{k}": v for k, v in r.items()})
        m = r["xt"] == 4
        print(f"{case}: B={r['x0'].shape[0]} L={r['x0'].shape[1]} masked {float(m.float().mean()):.3f} loss {r['loss'].tolist()}")
    arrs["cases"] = np.array(list(cases))
    save(name, **arrs)


def g30():
    L = 50
    d = tiny_diffusion(L, 8)
    _save("g30_elbo_tiny.npz", {"rand": record_case(d, _random_x0(8, L, 300), 30),
                                "short": record_case(d, _random_x0(3, L, 301), 31)})


def g31():
    dec = torch.from_numpy(np.load(os.path.join(HERE, "g24_decode_sample_c2.npz"))["x0"][:64].astype(np.int64))
    d, _, _ = full_nets(length=200, steps=128)
    cases = {"dna_rand": record_case(d, _random_x0(64, 200, 310), 32),
             "dna_dec": record_case(d, dec, 33)}
    d50, _, _ = full_nets(length=50, steps=128)
    cases["rna_rand"] = record_case(d50, _random_x0(64, 50, 311), 34)
    _save("g31_elbo_full.npz", cases)


if __name__ == "__main__":
    torch.set_num_threads(int(os.environ.get("SVDD_GOLDEN_THREADS", "8")))
    for arg in sys.argv[1:]:
        {"g30": g30, "g31": g31}[arg]()
