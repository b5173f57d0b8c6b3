"""Golden vectors of the value function's training data (Monte-Carlo and CD-Q rollouts), recorded by RUNNING THE REFERENCE on CPU.

Run in the build container only (needs the reference, imported through tests/golden/_ref_import.py like make_golden.py):

    python tests/golden/make_golden_cdq.py g34 g35

The reference builds the training set of its value net inside Enformer.BaseModel.forward (Enformer.py:163-267) from
Diffusion._sample (diffusion_gosai.py:820-886): `_sample(cdq=True)` draws 10 next states per step from the same q_xs and continues
from the last one; forward then regresses every intermediate state onto the mean of the value net's predictions on the NEXT step's
draws (CD-Q, :226-259), or every state of a plain `_sample()` rollout onto r(x_0) (Monte Carlo, :192-225). This script only calls
`_sample` and the nets, as forward does, and records inputs and outputs. The value net is evaluated in EVAL mode (the engine's
stated departure: DESIGN 4h); `y_cdq` is the reference's own `case_sum = case_sum + v ... case_sum / len(time_samples)` expression
(:235-238) on those eval-mode values. Per file:

  seed          torch.manual_seed before _sample(cdq=True)
  S, draws      steps and draws per step (the reference hard-codes 10, :846)
  all_mid       [S, draws, B, L] u8: all_time_mid_x ; mid [S - 1, B, L] u8: mid_x ; final [B, L] u8: x_0
  values        [S, draws, B] f32: head(embedding(transform_samples(draw).float())).squeeze(2) per draw (step 0 included, unused)
  y_cdq         [S - 1, B] f32: the CD-Q target of mid[i - 1] from values[i], i = 1 .. S - 1
  reward        [B] f32: reward_model(onehot(x_0).float().transpose(1, 2))[:, 0]
  next          [2] f32: torch.rand(2) right after the run
  mc_seed, mc_mid [S - 1, B, L], mc_final [B, L], mc_reward [B], mc_next [2]: the same from _sample(cdq=False)

  g34_cdq_tiny.npz   tiny nets of make_golden.py (hidden 16 x 1 stack; 8-channel value net, also the reward model), L = 50, B = 8,
                     S = 8, seed 50
  g35_cdq_full.npz   full-size seed-44 nets and reward model (synthetic.build's classes and order), L = 200, B = 3, S = 32, seed 51;
                     parameter checksums as in g33
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import RewardWrap, full_nets, full_reward, save, tiny_diffusion, tiny_value  # noqa: E402

DRAWS = 10                                                                      # `for j in range(10)`, diffusion_gosai.py:846


def record(d, emb, head, reward, B, S, seed):
    u8 = lambda t: t.to(torch.uint8)                                            # noqa: E731
    r_of = lambda x: reward(d.transform_samples(x).float().transpose(1, 2)).detach()[:, 0].reshape(B)   # noqa: E731
    with torch.no_grad():
        torch.manual_seed(seed)
        x0, mid, all_mid = d._sample(num_steps=S, eval_sp_size=B, cdq=True)
        nxt = torch.rand(2)
        assert len(mid) == S - 1 and len(all_mid) == S and all(len(a) == DRAWS for a in all_mid)
        values = [[head(emb(d.transform_samples(c).float())).squeeze(2) for c in step] for step in all_mid]      # [B, 1] each
        y = []
        for time, vs in enumerate(values):                                      # Enformer.py:232-247
            if time == 0:
                continue
            case_sum = 0
            for v in vs:
                case_sum = case_sum + v.detach().clone()
            y.append((case_sum / len(vs)).reshape(B))
        torch.manual_seed(seed + 100)
        mc_x0, mc_mid = d._sample(num_steps=S, eval_sp_size=B)
        mc_nxt = torch.rand(2)
        out = dict(seed=seed, S=S, draws=DRAWS, all_mid=u8(torch.stack([torch.stack(a) for a in all_mid])), mid=u8(torch.stack(mid)),
                   final=u8(x0), values=torch.stack([torch.stack([v.reshape(B) for v in vs]) for vs in values]), y_cdq=torch.stack(y),
                   reward=r_of(x0), next=nxt, mc_seed=seed + 100, mc_mid=u8(torch.stack(mc_mid)), mc_final=u8(mc_x0),
                   mc_reward=r_of(mc_x0), mc_next=mc_nxt)
    assert all(torch.equal(mid[i], all_mid[i][-1]) for i in range(S - 1)) and int(x0.max()) <= 3
    spread = float((out["y_cdq"][1:] - out["y_cdq"][:-1]).abs().mean())
    print(f"B={B} S={S}: y_cdq mean |step-to-step difference| {spread:.3e}, values std over draws {float(out['values'][1:].std(1).mean()):.3e}")
    return out


def g34():
    L, B, S = 50, 8, 8
    d = tiny_diffusion(L, S)
    emb, head = tiny_value()
    save("g34_cdq_tiny.npz", **record(d, emb, head, RewardWrap(emb, head).eval(), B, S, 50))


def g35():
    L, B, S = 200, 3, 32
    d, emb, head = full_nets(length=L, steps=S)
    emb_r, head_r = full_reward()
    arrs = {n_ + "_param_sums": np.array([float(p.double().sum()) for p in mod.state_dict().values()])
            for n_, mod in (("backbone", d.backbone), ("embedding", emb), ("head", head), ("reward_embedding", emb_r),
                            ("reward_head", head_r))}
    save("g35_cdq_full.npz", net_seed=44, **arrs, **record(d, emb, head, RewardWrap(emb_r, head_r).eval(), B, S, 51))


if __name__ == "__main__":
    torch.set_num_threads(int(os.environ.get("SVDD_GOLDEN_THREADS", "8")))
    for arg in sys.argv[1:]:
        {"g34": g34, "g35": g35}[arg]()
