"""Golden vectors of the classifier-guidance sampler, recorded by RUNNING THE REFERENCE on CPU.

Run in the build container only (needs the reference, imported through tests/golden/_ref_import.py like make_golden.py):

    python tests/golden/make_golden_classifier.py probe        # gradient magnitudes (to choose the guidance scales)
    python tests/golden/make_golden_classifier.py g27 g28      # single-threaded: 0.3 s and 0.9 s of reference decode
    python tests/golden/make_golden_classifier.py g29          # SVDD_GOLDEN_THREADS torch threads (default 8): 188 s on 8 cores

The sampler is `Diffusion.controlled_sample_classfier` (diffusion_gosai.py:1064-1104) with its step
`_ddpm_update_finetune_classfier` (:1332-1360) and `compute_gradient` (:1362-1371). Its step pads the gradient with
`torch.zeros(...).cuda()`; `torch.Tensor.cuda` is made a no-op for the call so that the reference runs on CPU. Only inputs and
outputs are stored. Per step:

  x            the state x_t the step starts from (u8)
  logits       the backbone's raw output on x_t, as a logical [B, L, 5] array
  grad         compute_gradient's result [B, L, 4] (d mean(head(embedding(onehot))) / d onehot)
  q            the UN-guided q_xs the step returns (its 3rd output), logical [B, L, 5]
  w            the guided weights handed to _sample_categorical: q + scale * cat(grad, 0)
  u            the uniforms rand_like(w) drew, logical [B, L, 5]; `u_strides` / `w_strides` record the memory order they were drawn
               in (the element strides of the two tensors: (5 L, 1, L) is [b][v][l], the reference CNN's permuted output)
  x0           the decoded tokens after noise removal

  g27_traj_classifier.npz       tiny nets of make_golden.py (tiny_diffusion / tiny_value), S = 6, B = 3, L = 50: everything per step
  g28_traj_classifier_full.npz  full-size nets (synthetic.build("dna")'s classes and order, seed 44), L = 200, B = 3, S = 4:
                                everything per step + parameter checksums
  g29_traj_classifier_c2.npz    full-size nets at B = 256, L = 200, S = 128. Lean: every state, losslessly as (`unmask_step`, `token`)
                                [B, L] — position (b, l) holds `token` in x_s for s > unmask_step and MASK before (a position never returns
                                to MASK: copy_flag) — plus x0 and, at the steps `keep_steps`, the first `keep_rows` rows of grad / q / w.
                                The uniforms are not stored: the test replays the mt19937 stream (one rand_like per step).

Each fixture also records the guidance scale, the number of guided weights that are negative and the number of draws at masked
positions that differ from the draw with the same uniforms at scale 0 (`n_negative`, `n_changed`, `n_masked_draws`).
"""
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import (RecBackbone, dg, full_nets, save, sched_rows, tiny_diffusion, tiny_value)  # noqa: E402


def _param_sums(**mods):
    return {k + "_param_sums": np.array([float(p.double().sum()) for p in m.state_dict().values()]) for k, m in mods.items()}


def record(d, emb, head, B, S, scale, seed, keep_steps=None, keep_rows=None):
    """Run the reference's controlled_sample_classfier and record every step (see the module docstring)."""
    rec = {"x": [], "xn": [], "q": [], "grad": [], "w": [], "u": [], "n_neg": 0, "n_changed": 0, "n_masked": 0,
           "u_strides": None, "w_strides": None}
    bb = RecBackbone(d.backbone)
    d.backbone = bb
    orig_sc, orig_rl, orig_cuda = dg._sample_categorical, torch.rand_like, torch.Tensor.cuda
    orig_step, orig_grad = d._ddpm_update_finetune_classfier, d.compute_gradient
    cur = {}

    def rl(t, *a, **k):
        r = orig_rl(t, *a, **k)
        cur["u"] = r.detach().clone()
        if rec["u_strides"] is None:
            rec["u_strides"] = r.stride()
        return r

    def sc(w):
        torch.rand_like = rl
        try:
            out = orig_sc(w)
        finally:
            torch.rand_like = orig_rl
        cur["w"] = w.detach().clone()
        if rec["w_strides"] is None:
            rec["w_strides"] = w.stride()
        return out

    def grad(x, e, h):
        g = orig_grad(x, e, h)
        cur["grad"] = g.detach().clone()
        return g

    def step(x, t, dt, e, h, gs):
        out = orig_step(x, t, dt, e, h, gs)
        x_next, x_in, q_xs, _ = out
        s = len(rec["x"])
        masked = (x_in == 4)
        w, u = cur["w"], cur["u"]
        gumbel = 1e-10 - (u + 1e-10).log()
        changed = (q_xs / gumbel).argmax(-1) != (w / gumbel).argmax(-1)          # vs scale 0 with the same uniforms
        rec["n_neg"] += int((w < 0).sum())
        rec["n_changed"] += int((changed & masked).sum())
        rec["n_masked"] += int(masked.sum())
        rec["x"].append(x_in.to(torch.uint8).clone())
        rec["xn"].append(x_next.to(torch.uint8).clone())
        if keep_steps is None or s in keep_steps:
            r = slice(None) if keep_rows is None else slice(0, keep_rows)
            rec["q"].append(q_xs.detach()[r].clone())
            rec["grad"].append(cur["grad"][r].clone())
            rec["w"].append(w[r].clone())
            if keep_steps is None:
                rec["u"].append(u.clone())
        return out

    dg._sample_categorical = sc
    torch.Tensor.cuda = lambda self, *a, **k: self
    d._ddpm_update_finetune_classfier, d.compute_gradient = step, grad
    t0 = time.time()
    try:
        torch.manual_seed(seed)
        x0 = d.controlled_sample_classfier(emb, head, eval_sp_size=B, guidance_scale=scale)
    finally:
        dg._sample_categorical, torch.Tensor.cuda = orig_sc, orig_cuda
        del d._ddpm_update_finetune_classfier, d.compute_gradient
        d.backbone = bb.inner
    secs = time.time() - t0
    assert len(rec["x"]) == S and len(bb.calls) == S + 1
    print(f"B={B} S={S} scale={scale}: {secs:.1f} s, u strides {rec['u_strides']}, w strides {rec['w_strides']}, "
          f"negative weights {rec['n_neg']}, changed draws {rec['n_changed']} / {rec['n_masked']} masked")
    rec["logits"] = [c[1] for c in bb.calls[:S]]
    rec["x0"], rec["secs"] = x0, secs
    return rec


def _common(rec, d, B, L, S, scale, seed):
    return dict(x0=rec["x0"].to(torch.uint8), seed=seed, scale=np.float64(scale), B=B, L=L, S=S, sched=sched_rows(d, S),
                u_strides=np.array(rec["u_strides"]), w_strides=np.array(rec["w_strides"]), n_negative=rec["n_neg"],
                n_changed=rec["n_changed"], n_masked_draws=rec["n_masked"], threads=torch.get_num_threads(),
                seconds=np.float64(rec["secs"]))


def g27(seed=27, scale=50.0):
    L, S, B = 50, 6, 3
    d = tiny_diffusion(L, S)
    emb, head = tiny_value()
    rec = record(d, emb, head, B, S, scale, seed)
    save("g27_traj_classifier.npz", xs=torch.stack(rec["x"]), x_next=torch.stack(rec["xn"]),
         logits=torch.stack(rec["logits"]).contiguous(), grad=torch.stack(rec["grad"]), q=torch.stack(rec["q"]).contiguous(),
         w=torch.stack(rec["w"]).contiguous(), u=torch.stack(rec["u"]).contiguous(), **_common(rec, d, B, L, S, scale, seed))


def g28(seed=28, scale=100.0):
    L, S, B = 200, 4, 3
    d, emb, head = full_nets(length=L, steps=S)
    rec = record(d, emb, head, B, S, scale, seed)
    save("g28_traj_classifier_full.npz", xs=torch.stack(rec["x"]), x_next=torch.stack(rec["xn"]),
         logits=torch.stack(rec["logits"]).contiguous(), grad=torch.stack(rec["grad"]), q=torch.stack(rec["q"]).contiguous(),
         w=torch.stack(rec["w"]).contiguous(), u=torch.stack(rec["u"]).contiguous(), net_seed=44,
         **_param_sums(backbone=d.backbone, embedding=emb, head=head), **_common(rec, d, B, L, S, scale, seed))


def g29(seed=0, scale=256.0, B=256, L=200, S=128, keep_steps=(0, 32, 96, 127), keep_rows=8):
    d, emb, head = full_nets(length=L, steps=S)
    rec = record(d, emb, head, B, S, scale, seed, keep_steps=keep_steps, keep_rows=keep_rows)
    xs = torch.stack(rec["x"] + [rec["xn"][-1]])                               # [S + 1, B, L]: x_0 .. x_S
    final = xs[-1]
    unmask = torch.full((B, L), S, dtype=torch.uint8)                          # the step whose draw unmasked the position (S: never)
    for s in range(S - 1, -1, -1):
        newly = (xs[s] == 4) & (xs[s + 1] != 4)
        unmask[newly] = s
    for s in range(S + 1):                                                     # the encoding is lossless
        assert torch.equal(torch.where(unmask < s, final, torch.full_like(final, 4)), xs[s])
    save("g29_traj_classifier_c2.npz", unmask_step=unmask, token=final, x0=rec["x0"].to(torch.uint8),
         keep_steps=np.array(keep_steps), keep_rows=keep_rows, grad=torch.stack(rec["grad"]), q=torch.stack(rec["q"]).contiguous(),
         w=torch.stack(rec["w"]).contiguous(), net_seed=44, **_param_sums(backbone=d.backbone, embedding=emb, head=head),
         **{k: v for k, v in _common(rec, d, B, L, S, scale, seed).items() if k != "x0"})


def probe():
    """Gradient magnitude at the prior and after a few un-guided steps: the scale at which guidance acts is ~ q / |grad|."""
    for name, (d, emb, head), B in (("tiny", (tiny_diffusion(50, 6),) + tiny_value(), 3),
                                    ("full", full_nets(length=200, steps=4), 3), ("full", full_nets(length=200, steps=4), 256)):
        L = d.config.model.length
        torch.manual_seed(0)
        x = torch.where(torch.rand(B, L) < 0.5, torch.randint(0, 4, (B, L)), torch.full((B, L), 4))
        g = d.compute_gradient(d.transform_samples(x).float(), emb, head)
        print(f"{name} B={B}: |grad| max {float(g.abs().max()):.3e} median {float(g.abs().median()):.3e}")


if __name__ == "__main__":
    torch.set_num_threads(int(os.environ.get("SVDD_GOLDEN_THREADS", "8")) if "g29" in sys.argv else 1)
    for arg in sys.argv[1:]:
        {"probe": probe, "g27": g27, "g28": g28, "g29": g29}[arg]()
