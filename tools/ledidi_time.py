"""Timing of Ledidi design (Diffusion.ledidi) at B = 256, L = 200, S = 10, fp32, ConvGRU value net, 100 iterations without early
stopping, under replayed uniforms, in one process. Every figure is the time per call from a device-synchronised window of whole calls
that lasts more than a second (one call of (a), six of (b), two of (c)), the arms alternated round after round after one warm-up
each; per arm the rounds' minimum .. maximum are printed.
  (a) Diffusion.ledidi: per iteration and pass forward_tokens, mean_score_input_grad, one svdd_ledidi_step launch;
  (b) the scoring passes of (a) alone (forward_tokens on the same chunks): what the exact scores cost beside the gradient pass;
  (c) the same loop composed from pieces that were public before this feature: torch ops for the Gumbel-softmax samples on the same
      uniforms, forward_grad + torch autograd, ONE torch.optim.AdamW over all designs, best tracking on the host with a read-back
      per iteration. Whether its picks agree with (a)'s is printed;
  (d) Diffusion.evolve from the same starts (10 iterations, the reference's rule) beside (a) at l = 0.1 and at l = 0.001: score gain
      and edits of each.
`--profile` runs (a) once for `rocprofv3 --kernel-trace --stats`; `--stats FILE.csv` appends that run's kernel table (launches per
iteration, svdd_ledidi_step's share) to the report.
Usage: python tools/ledidi_time.py [--rounds 3] [--out profiles/ledidi_time.txt] [--profile] [--stats kernel_stats.csv] [--note TEXT ...]"""
import argparse, csv, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--iters", type=int, default=100)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ledidi_time.txt"))
ap.add_argument("--profile", action="store_true")
ap.add_argument("--stats", default=None)
ap.add_argument("--note", action="append", default=[])
args = ap.parse_args()
B, L, S, ITERS = args.batch, 200, 10, args.iters


def stats_lines(path):
    """The kernel table of a rocprofv3 --kernel-trace --stats run of `--profile`."""
    rows = list(csv.DictReader(open(path)))
    name = lambda r: r.get("Name") or r.get("KernelName") or ""                       # noqa: E731
    calls = lambda r: int(float(r.get("Calls") or r.get("Count") or 0))               # noqa: E731
    ns = lambda r: float(r.get("TotalDurationNs") or r.get("TotalDuration") or 0.0)   # noqa: E731
    total_ns, total_calls = sum(ns(r) for r in rows), sum(calls(r) for r in rows)
    led = [r for r in rows if "ledidi_step" in name(r)]
    out = [f"rocprofv3 --kernel-trace --stats of one call of (a) ({ITERS} iterations, a run of its own): {total_calls} kernel launches = "
           f"{total_calls / ITERS:.1f} per iteration, {total_ns / 1e6:.1f} ms of kernel time = {total_ns / 1e6 / ITERS:.3f} ms per iteration"]
    for r in led:
        out.append(f"  svdd_ledidi_step: {calls(r)} launches, {ns(r) / 1e6:.2f} ms = {ns(r) / max(calls(r), 1) / 1e3:.1f} us each = "
                   f"{100 * ns(r) / total_ns:.2f} % of the kernel time")
    for r in sorted(rows, key=ns, reverse=True)[:6]:
        out.append(f"  {100 * ns(r) / total_ns:6.2f} %  {calls(r):7d} x  {name(r)[:110]}")
    return out


if args.stats and not os.path.exists(args.out):
    sys.exit(f"{args.out} does not exist: run the timing first")
if args.stats:
    with open(args.out, "a") as f:
        f.write("\n".join(stats_lines(args.stats)) + "\n")
    print("\n".join(stats_lines(args.stats)))
    sys.exit(0)

import torch
import torch.nn.functional as F
from svdd_amd import ops, synthetic
from svdd_amd.diffusion import design_pick

DEV = "cuda:0"
model, emb, head, reward = synthetic.build("dna", DEV)
fn = model._classifier_fused_value(emb, head, L)
assert fn is not None, "the fused route must apply at this shape"
x = torch.randint(0, 4, (B, L), generator=torch.Generator().manual_seed(0)).to(torch.uint8).to(DEV)
noise = torch.rand((ITERS, B, S, L, 4), generator=torch.Generator().manual_seed(1)).to(DEV)
KW = dict(max_iter=ITERS - 1, batch_size=S, early_stopping_iter=ITERS + 1, noise=noise)


def window(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def run_ledidi():
    return model.ledidi(x, emb, head, **KW)


if args.profile:
    run_ledidi()
    torch.cuda.synchronize()
    sys.exit(0)

PER = model.ATTR_CHUNK_ROWS // S                                          # designs per pass
CHUNKS = [(d0, min(PER, B - d0)) for d0 in range(0, B, PER)]
REPEAT = {"a": 1, "b": 6, "c": 2}                                         # calls per window: every window lasts more than a second


@torch.no_grad()
def run_scores():
    tok = x[:, None, :].expand(B, S, L).reshape(B * S, L).contiguous()
    for _ in range(ITERS):
        for d0, nd in CHUNKS:
            fn.forward_tokens(tok[d0 * S:(d0 + nd) * S])


def run_composed(tau=1.0, l=0.1, eps=1e-4):
    X = ops.transform_samples(x)
    logit0 = torch.log(X + eps)
    w = torch.zeros((B, L, 4), device=DEV, requires_grad=True)
    opt = torch.optim.AdamW([w], lr=1.0)
    with torch.no_grad():
        score0 = fn.forward_tokens(x).reshape(B)
    best_total = (-score0).tolist()
    best_iter, best_x = [-1] * B, [None] * B
    for i in range(ITERS):
        opt.zero_grad(set_to_none=True)
        g = -torch.log(1e-10 - torch.log(noise[i] + 1e-10))
        y = torch.softmax(((logit0 + w)[:, None] + g) / tau, dim=-1)
        tok = y.argmax(-1)
        hard = F.one_hot(tok, 4).to(y.dtype)
        x_hat = hard + (y - y.detach())
        sc = fn.forward_grad(x_hat.reshape(B * S, L, 4)).reshape(B, S)
        total = -sc.mean(dim=1) + l * ((x_hat - X[:, None]).abs().sum(dim=(1, 2, 3)) / (2 * S))
        total.sum().backward()
        opt.step()
        for b, t in enumerate(total.tolist()):                              # the host's best tracking: one read-back per iteration
            if t < best_total[b]:
                best_total[b], best_iter[b], best_x[b] = t, i, tok[b]
    return best_total, best_iter, best_x


arms = {"a": run_ledidi, "b": run_scores, "c": run_composed}
for f in arms.values():
    f()                                                                     # warm-up
times = {k: [] for k in arms}
for _ in range(args.rounds):
    for k, f in arms.items():
        times[k].append(window(lambda: [f() for _ in range(REPEAT[k])])[0] / REPEAT[k])
res = run_ledidi()
c_total, c_iter, c_x = run_composed()
bi = res.best_iter.tolist()
same_iter = sum(int(a == b) for a, b in zip(bi, c_iter))
same_x = sum(int(a == b and (a < 0 or bool(torch.equal(res.x_best[k], c_x[k].to(torch.uint8))))) for k, (a, b) in enumerate(zip(bi, c_iter)))
tok_l, sc_l, ed_l = design_pick(res)
res0 = model.ledidi(x, emb, head, l=0.001, **KW)                           # the same call with an edit weight the score gains can pay
tok_0, sc_0, ed_0 = design_pick(res0)
model.evolve(x, emb, head, max_iter=10)                                    # warm-up
ev = [window(lambda: model.evolve(x, emb, head, max_iter=10)) for _ in range(3)]
t_ev, (x_ev, sc_ev, tr_ev) = min(t for t, _ in ev), ev[-1][1]
ed_ev = (x_ev.to(torch.uint8) != x).sum(1)
rng = lambda v: f"{min(v) / ITERS:.3f} .. {max(v) / ITERS:.3f} ms per iteration ({min(v):.0f} .. {max(v):.0f} ms per call)"   # noqa: E731
lines = [f"Ledidi timing: B = {B} designs, L = {L}, S = {S} samples, fp32, ConvGRU value net, {ITERS} iterations, no early stopping, replayed "
         f"uniforms, {len(CHUNKS)} passes of at most 1024 rows per iteration; {args.rounds} rounds, arms alternated, "
         f"device-synchronised windows of {REPEAT['a']} / {REPEAT['b']} / {REPEAT['c']} whole calls of (a) / (b) / (c) (each more than a second), "
         "times per call",
         f"device: {torch.cuda.get_device_name(0)}", "",
         f"(a) Diffusion.ledidi:                                   {rng(times['a'])}",
         f"    its gradient passes run on {sum(1 << (nd * S - 1).bit_length() for _, nd in CHUNKS)} rows for {B * S} samples (a power of two per pass)",
         f"(b) forward_tokens on the same chunks alone:            {rng(times['b'])} = {100 * min(times['b']) / min(times['a']):.1f} % of (a)",
         f"(c) composed: torch Gumbel-softmax + forward_grad autograd + AdamW + host best tracking: {rng(times['c'])}",
         f"    (c) : (a) = {min(times['c']) / min(times['a']):.2f} (minimum against minimum)",
         f"    picks: {same_iter} of {B} designs have the same best iteration in (a) and (c), {same_x} of {B} the same best samples too "
         "((c) scores through forward_grad, whose bits are not forward_tokens')",
         f"(d) from the same {B} starts: ledidi (l = 0.1, {ITERS} iterations, design_pick): score gain {float((sc_l - res.score0).mean()):.4e}, "
         f"edits {float(ed_l.float().mean()):.1f} per design, {int((res.best_iter >= 0).sum())} designs improved; at l = 0.001: score gain "
         f"{float((sc_0 - res0.score0).mean()):.4e}, edits {float(ed_0.float().mean()):.1f}, {int((res0.best_iter >= 0).sum())} improved; evolve (10 iterations, global rule, {t_ev:.0f} ms at the fastest of 3 calls of about half a second after a warm-up, {tr_ev['iters']} run): score gain "
         f"{float((sc_ev - res.score0).mean()):.4e}, edits {float(ed_ev.float().mean()):.1f} per design", ""]
lines += args.note
text = "\n".join(lines) + "\n"
print(text)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text)
