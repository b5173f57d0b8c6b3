"""Timing of the value function's training data (Diffusion.value_targets) at the C2 shape: B = 256, L = 200, 128 steps, ConvGRU value
net, fp32, Philox, 10 draws per step, in one process:
  (a) one value_targets("cdq") call: one backbone launch and one propose per step, the value net on the B * 10 candidates through
      _value_scores (candidate windows where they apply), one svdd_value_target launch per step;
  (b) the same training set composed from pieces that were public before this feature: the backbone forward, ops.propose with 10
      draws, ONE value_callable call per draw as the reference does (Enformer.py:236-237), the reference's `case_sum = case_sum + v`
      / len(...) in torch, transform_samples per state, the noise removal and the reward;
  (c) one value_targets("mc") call;
  (d) the torch forward and backward of one training step on (a)'s set (the modules in train mode, MSE loss, no optimiser step);
  and the new kernel alone: 128 svdd_value_target launches at this shape, as a share of (a).
(a) and (b) must produce the same states; their targets agree to the value net's batch-composition round-off (printed).
Usage: python tools/value_targets_time.py [--reps 5] [--out profiles/value_targets_time.txt] [--note TEXT ...]"""
import argparse, copy, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from svdd_amd import ops, synthetic

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--steps", type=int, default=128)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "value_targets_time.txt"))
ap.add_argument("--note", action="append", default=[])
args = ap.parse_args()

B, L, M, S = args.batch, 200, 10, args.steps
DEV = "cuda:0"
model, emb, head, reward = synthetic.build("dna", DEV)
model.rng_mode, model.philox_seed = "philox", 0


def timed(fn, reps):
    """Median and minimum wall clock (ms) of fn() over reps runs, each between two device synchronisations, after one warm-up."""
    fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def cdq():
    return model.value_targets(emb, head, reward, mode="cdq", draws=M, num_steps=S, eval_sp_size=B)


def mc():
    return model.value_targets(emb, head, reward, mode="mc", num_steps=S, eval_sp_size=B)


@torch.no_grad()
def composed():
    """(b): the reference's recipe on the pieces that existed before value_targets -> (states u8 [S, B, L], onehot [S B, L, 4], y [S B])."""
    fn = model.value_callable(emb, head)
    sched = model._schedule(S, 1e-5)[0]
    x = torch.full((B, L), 4, dtype=torch.uint8, device=DEV)
    states, onehots, ys = [], [], []
    for i in range(S):
        logits = model._backbone_logits(x)
        cand, onehot, _ = ops.propose(logits, x, sched[i, 2], sched[i, 1], M, model._rng(i, M, B, L, logits))
        if i > 0:
            oh = onehot.view(B, M, L, 4)
            case_sum = 0
            for j in range(M):
                case_sum = case_sum + fn(oh[:, j].contiguous()).reshape(B).float()
            ys.append(case_sum / M)
        x = cand[:, M - 1].contiguous()
        if i != S - 1:
            states.append(x)
            onehots.append(ops.transform_samples(x))
    x0 = model._noise_removal(x).to(torch.uint8)
    states.append(x0)
    onehots.append(ops.transform_samples(x0))
    ys.append(model.reward_callable(reward)(ops.transform_samples(x0, transposed=True)).reshape(B).float())
    return torch.stack(states), torch.cat(onehots), torch.cat(ys)


a_med, a_min = timed(cdq, args.reps)
b_med, b_min = timed(composed, args.reps)
c_med, c_min = timed(mc, args.reps)
vt = cdq()
st_b, oh_b, y_b = composed()
same_states = bool(torch.equal(vt.states, st_b)) and bool(torch.equal(vt.onehot, oh_b))
y_diff = float((vt.y - y_b).abs().max())

cand = torch.randint(0, 5, (B, M, L), dtype=torch.uint8, device=DEV)
scores = torch.randn(B, M, device=DEV)
xn, ohn, tg = torch.empty((B, L), dtype=torch.uint8, device=DEV), torch.empty((B, L, 4), device=DEV), torch.empty(B, device=DEV)


def kernel_alone():
    for _ in range(S):
        ops.value_target(scores, cand, x_next=xn, onehot_next=ohn, target=tg)


k_med, k_min = timed(kernel_alone, args.reps)

emb_t, head_t = copy.deepcopy(emb).train(), copy.deepcopy(head).train()
for p in list(emb_t.parameters()) + list(head_t.parameters()):
    p.requires_grad_(True)


def train_step():
    for p in list(emb_t.parameters()) + list(head_t.parameters()):
        p.grad = None
    loss = torch.nn.functional.mse_loss(head_t(emb_t(vt.onehot)).view(-1), vt.y)
    loss.backward()


try:
    d_med, d_min = timed(train_step, max(2, args.reps // 2))
    d_line = (f"(d) forward + backward of one training step on (a)'s {S * B} rows (torch modules, train mode): {d_med:9.2f} ms [{d_min:.2f}]; "
              f"(a) : (d) = {a_med / d_med:.2f}")
except RuntimeError as e:                                    # reported, not hidden: the vendor libraries have batch limits of their own
    d_line = f"(d) forward + backward of one training step on (a)'s {S * B} rows: FAILED in the torch modules: {str(e).splitlines()[0]}"

rows = S * B
lines = [f"value_targets timing: B = {B}, L = {L}, {S} steps, {M} draws per step, ConvGRU value net, fp32, Philox; median of {args.reps} "
         f"(minimum in brackets), wall clock between device synchronisations, one warm-up each",
         f"device: {torch.cuda.get_device_name(0)}", "",
         f"(a) value_targets('cdq'): {a_med:9.2f} ms [{a_min:.2f}] = {a_med / S:.3f} ms per step; {(S - 1) * M * B} candidate rows scored, {rows} training rows",
         f"(b) composed from the earlier public pieces (one value call per draw, torch mean): {b_med:9.2f} ms [{b_min:.2f}] = {b_med / S:.3f} ms per step",
         f"    (a) : (b) = {a_med / b_med:.3f} ((b) is {b_med / a_med:.2f} x (a)); same states and one-hot rows: {same_states}; max |y(a) - y(b)| = {y_diff:.2e}",
         f"(c) value_targets('mc'):  {c_med:9.2f} ms [{c_min:.2f}] = {c_med / S:.3f} ms per step",
         d_line,
         f"    svdd_value_target alone, {S} launches at this shape: {k_med:.3f} ms [{k_min:.3f}] = {1e3 * k_med / S:.1f} us per launch (launch overhead "
         f"included) = {100 * k_med / a_med:.2f} % of (a)"]
lines += [""] + args.note if args.note else []
text = "\n".join(lines) + "\n"
print(text)
with open(args.out, "w") as f:
    f.write(text)
