"""Golden vectors of decoding from a given state and of re-mask refinement, recorded by RUNNING THE REFERENCE on CPU.

Run in the build container only (needs the reference, imported through tests/golden/_ref_import.py like make_golden.py):

    python tests/golden/make_golden_refine.py g32 g33

The reference has the two halves: the noising `q_xt` (diffusion_gosai.py:738-749) and per-step updates that take any (x, t, dt)
(`_ddpm_update_finetune_controlled`, :1174-1228; `_ddpm_update_finetune`, :1147-1172). This script only drives them, the way the
reference's own sampler loops do (:1036-1060), from a seeded start state at t_start over linspace(t_start, eps, S + 1) with
dt = (t_start - eps) / S, and records inputs and outputs. A frozen mask is applied as where(frozen, x0, q_xt(x0, move_chance)).
Two rounds: the result of round 0 is re-noised and decoded again (every new row is kept: accept = "always").
Per case (prefix `<case>_`):

  seed          torch.manual_seed before round 0's q_xt
  guided        1: _ddpm_update_finetune_controlled with M candidates; 0: _ddpm_update_finetune
  t_start, S, M, eps
  x0            [B, L] u8 clean start tokens ; frozen [B, L] u8 (1 = never re-masked)
  move_chance   fp32 scalar = 1 - exp(-sigma(t_start)) (the reference's noise schedule, fp32 torch ops)
  xt            [2, B, L] u8: the re-masked state each round starts from
  states        [2, S + 1, B, L] u8: x before every step, and before the noise removal
  final         [2, B, L] u8: the round's x_0 (:1049-1060)
  next          [2] fp32: torch.rand(2) right after the second round

  g32_refine_tiny.npz   tiny nets of make_golden.py (hidden 16 x 1 stack; 8-channel value net), L = 50, B = 8, S = 8, M = 4:
                        `mc_t03` / `mc_t10` (guided, t_start 0.3 / 1.0), `un_t03` (un-guided, t_start 0.3)
  g33_refine_full.npz   full-size seed-44 nets (synthetic.build's classes and order), L = 200, B = 3, t_start 0.3, S = 39, M = 10
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import full_nets, save, tiny_diffusion, tiny_value  # noqa: E402

MASK = 4


def _start(B, L, seed, frozen_p=0.3):
    g = torch.Generator().manual_seed(seed)
    x0 = torch.randint(0, 4, (B, L), generator=g)
    frozen = torch.rand((B, L), generator=g) < frozen_p
    frozen[0] = False                                       # a row with nothing frozen ...
    frozen[-1, : L // 2] = True                             # ... and one with a frozen flank
    return x0, frozen


def record_case(d, emb, head, x0, frozen, seed, t_start, S, M, guided, eps=1e-5, rounds=2):
    B, L = x0.shape
    sigma, _ = d.noise(torch.tensor([[t_start]], dtype=torch.float32))
    move_chance = 1 - torch.exp(-sigma)                                        # [1, 1], as :1725-1729
    timesteps = torch.linspace(t_start, eps, S + 1)
    dt = (t_start - eps) / S
    xts, states, finals = [], [], []
    x = x0.clone()
    with torch.no_grad():
        torch.manual_seed(seed)
        for _ in range(rounds):
            x = torch.where(frozen, x, d.q_xt(x, move_chance))
            xts.append(x.clone())
            st = []
            for i in range(S):
                st.append(x.clone())
                t = timesteps[i] * torch.ones(B, 1)
                if guided:
                    x, _, _, _ = d._ddpm_update_finetune_controlled(x, t, dt, emb, head, repeats=M)
                else:
                    x, _, _, _ = d._ddpm_update_finetune(x, t, dt)
            st.append(x.clone())
            t = timesteps[-1] * torch.ones(B, 1)                                # noise removal, :1049-1060
            x = d.forward(x, d.noise(t)[0])[:, :, :-1].argmax(dim=-1)
            states.append(torch.stack(st))
            finals.append(x.clone())
        nxt = torch.rand(2)
    u8 = lambda t: t.to(torch.uint8)                                            # noqa: E731
    for r in range(rounds):                                                     # what the feature relies on, in the reference itself
        keep = xts[r] != MASK
        assert torch.equal(finals[r][keep], xts[r][keep]) and int(finals[r].max()) <= 3
        assert torch.equal(xts[r][frozen], (x0 if r == 0 else finals[r - 1])[frozen])
    return dict(seed=seed, guided=int(guided), t_start=np.float64(t_start), S=S, M=M, eps=np.float64(eps), x0=u8(x0), frozen=u8(frozen),
                move_chance=move_chance.reshape(()), xt=u8(torch.stack(xts)), states=u8(torch.stack(states)),
                final=u8(torch.stack(finals)), next=nxt)


def _save(name, cases):
    arrs = {}
    for case, r in cases.items():
        arrs.update({f"{case}_{k}": v for k, v in r.items()})
        print(f"{case}: B={r['x0'].shape[0]} L={r['x0'].shape[1]} S={r['S']} move_chance {float(r['move_chance']):.6f} "
              f"masked per round {[int((x == MASK).sum()) for x in r['xt']]}")
    arrs["cases"] = np.array(list(cases))
    save(name, **arrs)


def g32():
    L, B, S, M = 50, 8, 8, 4
    d = tiny_diffusion(L, S)
    emb, head = tiny_value()
    x0, frozen = _start(B, L, 320)
    _save("g32_refine_tiny.npz", {"mc_t03": record_case(d, emb, head, x0, frozen, 40, 0.3, S, M, True),
                                  "mc_t10": record_case(d, emb, head, x0, frozen, 41, 1.0, S, M, True),
                                  "un_t03": record_case(d, emb, head, x0, frozen, 42, 0.3, S, M, False)})


def g33():
    L, B, M = 200, 3, 10
    d, emb, head = full_nets(length=L, steps=128)
    x0, frozen = _start(B, L, 330)
    arrs = {n_ + "_param_sums": np.array([float(p.double().sum()) for p in mod.state_dict().values()])
            for n_, mod in (("backbone", d.backbone), ("embedding", emb), ("head", head))}
    case = record_case(d, emb, head, x0, frozen, 43, 0.3, 39, M, True)
    case.update(arrs, net_seed=44)
    _save("g33_refine_full.npz", {"mc_t03": case})


if __name__ == "__main__":
    torch.set_num_threads(int(os.environ.get("SVDD_GOLDEN_THREADS", "8")))
    for arg in sys.argv[1:]:
        {"g32": g32, "g33": g33}[arg]()
