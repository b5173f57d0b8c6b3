"""Timing of gradient attributions (Diffusion.attributions) at B = 256, L = 200, fp32, ConvGRU value net, in one process. The median
of --reps calls timed with device events after one warm-up:
  (a) one inputxgradient call: svdd_attr_path, one mean_score_input_grad pass of 256 rows, svdd_attr_fold;
  (b) one integratedgradients call at 50 steps: 12,800 (row, step) pairs in passes of ATTR_CHUNK_ROWS rows;
  (c) the new kernels alone: the svdd_attr_path and svdd_attr_fold launches of (a) and of (b) on preallocated buffers, as a share;
  (d) the IG table of (b) composed from pieces that were public before this feature, in the same passes: the interpolants built
      with torch ops, mean_score_input_grad, the multiply-accumulate and the final product with torch ops;
  (e) the same table through forward_grad and torch autograd (the gradient of the sum of a pass's scores), same passes.
There is no earlier implementation of the call to compare with: (d) is the comparison. Printed with it: whether (b) and (d) give the
same bits, and the largest deviation of (e) from (b).
Usage: python tools/attr_time.py [--reps 5] [--out profiles/attr_time.txt] [--note TEXT ...]"""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from svdd_amd import ops, synthetic

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attr_time.txt"))
ap.add_argument("--note", action="append", default=[])
args = ap.parse_args()

B, L, S = args.batch, 200, args.steps
DEV = "cuda:0"
model, emb, head, reward = synthetic.build("dna", DEV)
fn = model._classifier_fused_value(emb, head, L)
assert fn is not None, "the fused route must apply at this shape"
x = torch.randint(0, 4, (B, L), generator=torch.Generator().manual_seed(0)).to(torch.uint8).to(DEV)
CHUNK = model.ATTR_CHUNK_ROWS
_, _, alphas, weights, _ = model._attr_inputs(x, "integratedgradients", None, S, None, None, False)


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


def passes(total):
    """(r0, rows, rows of the pass as launched) of attributions' fused route."""
    out, r0 = [], 0
    while r0 < total:
        left = total - r0
        n_pass = min(CHUNK, 1 << (left - 1).bit_length())
        out.append((r0, min(n_pass, left), n_pass))
        r0 += min(n_pass, left)
    return out


@torch.no_grad()
def composed(grad_of):
    """The IG table from the zero baseline with torch ops around grad_of(interpolants [n, L, 4]) -> the rows' gradients."""
    oh = ops.transform_samples(x)
    acc = torch.zeros((B, L, 4), device=DEV)
    for r0, n, n_pass in passes(B * S):
        r = torch.arange(r0, r0 + n, device=DEV)
        b, k = r // S, r % S
        xin = alphas[k][:, None, None] * oh[b]
        if n_pass > n:
            xin = torch.cat([xin, xin[:1].expand(n_pass - n, L, 4)])
        g = grad_of(xin, n_pass)[:n] * weights[k][:, None, None]
        acc.index_add_(0, b, g)
    return (oh * acc).permute(0, 2, 1).contiguous()


def grad_fused(xin, n_pass):
    return fn.mean_score_input_grad(xin) * float(n_pass)


def grad_autograd(xin, n_pass):
    with torch.enable_grad():
        xin = xin.detach().requires_grad_(True)
        return torch.autograd.grad(fn.forward_grad(xin).sum(), xin)[0]


def new_kernels_alone(steps):
    al, w = (alphas, weights) if steps > 1 else (torch.ones(1, device=DEV), torch.ones(1, device=DEV))
    plan = passes(B * steps)
    path = torch.empty((max(p[2] for p in plan), L, 4), device=DEV)
    grad = torch.randn((max(p[2] for p in plan), L, 4), device=DEV)
    acc, attr, rowsum = torch.empty((B, L, 4), device=DEV), torch.empty((B, 4, L), device=DEV), torch.empty(B, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)

    def do_path():
        for r0, n, n_pass in plan:
            ops.attr_path(x, al, r0, n, path[:n_pass], n_pad=n_pass - n, err=err)

    def do_fold():
        for r0, n, n_pass in plan:
            ops.attr_fold(grad, float(n_pass), w, x, r0, n, acc, attr, rowsum=rowsum)
    return len(plan), timed(do_path, args.reps), timed(do_fold, args.reps)


ig = lambda: model.attributions(x, emb, head, method="integratedgradients", n_steps=S)      # noqa: E731
a_med, a_min = timed(lambda: model.attributions(x, emb, head), args.reps)
b_med, b_min = timed(ig, args.reps)
n1, (p1, p1m), (f1, f1m) = new_kernels_alone(1)
nS, (pS, pSm), (fS, fSm) = new_kernels_alone(S)
d_med, d_min = timed(lambda: composed(grad_fused), args.reps)
e_med, e_min = timed(lambda: composed(grad_autograd), args.reps)
t_b, t_d, t_e = ig(), composed(grad_fused), composed(grad_autograd)
same = bool(torch.equal(t_b, t_d))
lines = [f"Attribution timing: B = {B}, L = {L}, fp32, ConvGRU value net, zero baseline; IG: {S} Gauss-Legendre steps = {B * S} (row, step) "
         f"pairs in {nS} passes of at most {CHUNK} rows; median of {args.reps} (minimum in brackets), device events, one warm-up each",
         f"device: {torch.cuda.get_device_name(0)}", "",
         f"(a) inputxgradient, one pass of {B} rows:                          {a_med:9.2f} ms [{a_min:.2f}]",
         f"(b) integratedgradients, {S} steps:                               {b_med:9.2f} ms [{b_min:.2f}] = {1e3 * b_med / (B * S):.2f} us per (row, step)",
         f"(c) new kernels alone: (a)'s {n1} pass: svdd_attr_path {p1:.3f} ms [{p1m:.3f}], svdd_attr_fold {f1:.3f} ms [{f1m:.3f}] = "
         f"{100 * (p1 + f1) / a_med:.2f} % of (a); (b)'s {nS} passes: svdd_attr_path {pS:.3f} ms [{pSm:.3f}], svdd_attr_fold {fS:.3f} ms [{fSm:.3f}] = "
         f"{100 * (pS + fS) / b_med:.2f} % of (b)",
         f"(d) composed: torch-built interpolants + mean_score_input_grad + torch fold: {d_med:9.2f} ms [{d_min:.2f}]",
         f"    (b) : (d) = {b_med / d_med:.3f} ((d) is {d_med / b_med:.2f} x (b)); same bits: {same}; largest |(b) - (d)| {float((t_b - t_d).abs().max()):.2e}",
         f"(e) composed with forward_grad + torch autograd instead of the pass:  {e_med:9.2f} ms [{e_min:.2f}] ((e) is {e_med / b_med:.2f} x (b)); "
         f"largest |(b) - (e)| {float((t_b - t_e).abs().max()):.2e} at max |(b)| {float(t_b.abs().max()):.2e}",
         ""]
lines += args.note
text = "\n".join(lines) + "\n"
print(text)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text)
