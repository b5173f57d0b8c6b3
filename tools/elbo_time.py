"""Rate of ELBO scoring (Diffusion.sequence_nll) at B = 256, L = 200 with the seed-44 random-init nets of synthetic.build("dna"):
K in {1, 8, 32} draws per sequence, fp32 and f16x3, replay and Philox, against a PyTorch-composed path (the CNN module on
MIOpen plus torch ops in the reference's order, diffusion_gosai.py:1660-1669, 738-749, 1709-1757, one draw of the whole batch at a
time).

    timeout -k 10 900 python tools/elbo_time.py [--reps 3] [--batch 256] [--draws 1 8 32]
    timeout -k 10 300 python tools/elbo_time.py --profile          # Philox fp32, K = 10 (2,560 rows): for rocprofv3 --kernel-trace --stats

One warm-up call, then --reps calls timed with device events; the median is reported as sequence-draws/s = B K / median. One JSON
line per configuration."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def composed(model, x0, K):
    """The reference's _forward_pass_diffusion K times in torch on the GPU (the PyTorch CNN module, no hand-written kernel)."""
    import torch
    n, L = x0.shape
    acc = torch.zeros(n, dtype=torch.float64, device=x0.device)
    bb = model.backbone
    for _ in range(K):
        e = torch.rand(n, device=x0.device)
        e = (e / n + torch.arange(n, device=x0.device) / n) % 1
        t = (1 - 1e-3) * e + 1e-3
        sigma, dsigma = model.noise(t)
        mc = 1 - torch.exp(-sigma[:, None])
        xt = torch.where(torch.rand(n, L, device=x0.device) < mc, 4, x0)
        logits = bb(xt, torch.zeros(n, device=x0.device)).clone()
        logits[:, :, 4] += -1000000.0
        logits = logits - torch.logsumexp(logits, dim=-1, keepdim=True)
        un = xt != 4
        logits[un] = -1000000.0
        logits[un, xt[un]] = 0
        lp = torch.gather(logits, -1, x0[:, :, None]).squeeze(-1)
        acc += (-lp * (dsigma / torch.expm1(sigma))[:, None]).sum(1, dtype=torch.float64)
    return acc / K


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--draws", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--profile", action="store_true", help="only Philox fp32 at K = 10, 5 calls (for rocprofv3)")
    args = ap.parse_args()

    import torch
    from svdd_amd import synthetic
    model = synthetic.build("dna", "cuda:0")[0]
    B = args.batch
    x0 = torch.randint(0, 4, (B, 200), device="cuda:0", generator=torch.Generator("cuda:0").manual_seed(1))
    if args.profile:
        model.rng_mode, model.philox_seed = "philox", 0
        for _ in range(6):
            model.sequence_nll(x0, n_draws=10)
        torch.cuda.synchronize()
        print(json.dumps({"profile": "philox f32 K=10 B=%d: 6 calls" % B}), flush=True)
        return
    for K in args.draws:
        for prec in ("f32", "f16x3"):
            for mode in ("philox", "replay"):
                model.rng_mode, model.philox_seed, model.precision = mode, 0, prec
                ms = timed(lambda: model.sequence_nll(x0, n_draws=K), args.reps)
                print(json.dumps({"path": "sequence_nll", "precision": prec, "rng": mode, "B": B, "L": 200, "K": K, "ms": round(ms, 3),
                                  "seq_draws_per_s": round(B * K / ms * 1e3, 1)}), flush=True)
        model.precision = "f32"
        with torch.no_grad():
            ms = timed(lambda: composed(model, x0, K), args.reps)
        print(json.dumps({"path": "torch_composed", "precision": "f32", "B": B, "L": 200, "K": K, "ms": round(ms, 3),
                          "seq_draws_per_s": round(B * K / ms * 1e3, 1)}), flush=True)


if __name__ == "__main__":
    main()
