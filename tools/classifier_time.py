"""Wall clock of a C2-shaped classifier-guidance decode (Diffusion.controlled_sample_classfier: B = 256, L = 200, 128 steps, the
ConvGRU value net, fp32, random-init nets of synthetic.build("dna")) and the kernel launches of one diffusion step.

    timeout -k 10 600 python tools/classifier_time.py [--reps 5] [--steps 128] [--batch 256] [--scale 256] [--rng philox|replay] [--no_launch_count]

One warm-up decode, then --reps timed decodes (each line printed as it completes, so a time limit still leaves the finished ones),
then the median: seq/s = B / median, ms per step = median / steps. Launches per step: kernel dispatches recorded by torch.profiler in a
decode of 6 steps minus those of a decode of 3 steps, divided by 3 (the prior's and the noise removal's launches cancel), listed by
kernel name. A decode that leaves the fused gradient path exits with status 2."""
import argparse
import collections
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def kernel_counts(decode):
    """{kernel name: dispatches} of one call of decode() (torch.profiler's device-side kernel events)."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        decode()
        torch.cuda.synchronize()
    counts = collections.Counter()
    for ev in prof.events():
        if ev.device_type == torch.autograd.DeviceType.CUDA:
            counts[ev.name] += 1
    return counts


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--scale", type=float, default=256.0)
    ap.add_argument("--rng", default="philox", choices=["philox", "replay"])
    ap.add_argument("--no_launch_count", action="store_true", help="skip the torch.profiler pass (e.g. under rocprofv3)")
    args = ap.parse_args()

    import torch
    from svdd_amd import synthetic
    model, emb, head, _ = synthetic.build("dna", "cuda:0")
    model.rng_mode, model.philox_seed = args.rng, 0
    B, S = args.batch, args.steps

    def decode(steps):
        torch.manual_seed(0)
        x = model.controlled_sample_classfier(emb, head, num_steps=steps, eval_sp_size=B, guidance_scale=args.scale)
        torch.cuda.synchronize()
        return x

    decode(8)
    if not model._classifier_fused_last:
        print("the value net's gradient did not take the fused path", flush=True)
        sys.exit(2)
    times = []
    for r in range(args.reps):
        t0 = time.perf_counter()
        decode(S)
        times.append(time.perf_counter() - t0)
        print(f"rep {r}: {times[-1] * 1e3:.1f} ms ({B / times[-1]:.1f} seq/s)", flush=True)
    med = statistics.median(times)
    print(f"classifier guidance, B={B} L=200 steps={S} scale={args.scale} rng={args.rng} fp32 ConvGRU value net: "
          f"median {med * 1e3:.1f} ms = {B / med:.1f} seq/s, {med / S * 1e3:.3f} ms per step (reps {args.reps})", flush=True)

    if args.no_launch_count:
        return
    c3, c6 = kernel_counts(lambda: decode(3)), kernel_counts(lambda: decode(6))
    if not c6:
        print("launches per step: n/a (the profiler recorded no kernel events)", flush=True)
        return
    per = {k: (c6[k] - c3.get(k, 0)) / 3 for k in c6 if c6[k] != c3.get(k, 0)}
    print(f"launches per step: {sum(per.values()):g}", flush=True)
    for k, v in sorted(per.items(), key=lambda kv: -kv[1]):
        print(f"  {v:g} x {k[:110]}", flush=True)


if __name__ == "__main__":
    main()
