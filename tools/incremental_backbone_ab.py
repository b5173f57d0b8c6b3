"""A/B: the incremental stem of the backbone (Diffusion.incremental_backbone, svdd_backbone_incr_f32) against the one-launch kernel
at the headline configuration (SVDD-MC, B = 256, L = 200, M = 10, 128 steps, fp32), in one process.
  1. per step, on the tokens of a real trajectory (state_trace): the summed launches of one incremental forward (work list +
     one segment launch per leading dilation-1 layer + the tail) against one launch of backbone_kernel, at early, middle and
     late steps, for work items of at most 2 and 4 row tiles, with the share of the stem's tile-layers the step marked;
  2. whole decodes: incremental_backbone "off" / "auto" alternating, wall clock and the backbone's profile slot.
Usage: python tools/incremental_backbone_ab.py [decodes per leg, default 3]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from svdd_amd import _lib, fused, synthetic

B, L, M, S = 256, 200, 10, 128
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
model, emb, head, _ = synthetic.build("dna", "cuda:0")
model.rng_mode, model.philox_seed = "philox", 0
run = lambda: model.controlled_sample(emb, head, num_steps=S, eval_sp_size=B, sample_M=M)

model.state_trace = []
run(); torch.cuda.synchronize()
states = [s.to("cuda:0").contiguous() for s in model.state_trace]
model.state_trace = None
fb = model._fused_backbone()
pk = fb.ol_pack()
stem = fb.incremental_stem(B, L)


def timed(fn, n=5):
    ts = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        pre = fn(None)
        torch.cuda.synchronize()
        e0.record(); fn(pre); e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return sorted(ts)[len(ts) // 2]


out = torch.empty((B, L, 5), device="cuda:0")
print(f"per step (us, median of 5): one launch | incremental, items <= 2 | items <= 4 | marked share of {B * 13 * stem.lead} tile-layers")
for i in (1, 2, 8, 32, 64, 96, 120, 126):
    if i + 1 >= len(states):
        continue
    a, b = states[i], states[i + 1]
    one = timed(lambda pre: fused.backbone_cnn(b, pk, out=out) if pre is not None else 1)
    ref = fused.backbone_cnn(b, pk).clone()
    res = []
    for mi in (2, 4):
        def step(pre, mi=mi):
            if pre is None:                              # the planes of step i (not timed)
                stem.valid = False
                fused.backbone_cnn_incremental(a, pk, stem, out=out, max_item=mi)
                stem.stat.zero_()
                return 1
            fused.backbone_cnn_incremental(b, pk, stem, out=out, max_item=mi)
        res.append(timed(step))
        assert torch.equal(out, ref), "the incremental forward differs from the one-launch kernel"
    changed = int((a != b).sum())
    print(f"step {i:3d} ({changed:4d} tokens changed): {one:7.1f} | {res[0]:7.1f} | {res[1]:7.1f} | {int(stem.stat) / (B * 13 * stem.lead):.3f}")

for mi in (2, 4):
    fused.INCR_MAX_ITEM = mi
    for rep in range(2):
        for mode in ("off", "auto"):
            model.incremental_backbone = mode
            run(); torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(reps):
                x = run()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t) / reps
            model.skip_stats = {}
            _lib.profile_enable(True); run(); torch.cuda.synchronize(); _lib.profile_enable(False)
            bb = _lib.profile_collect(6)
            for k in (0, 1, 3, 5, 7): _lib.profile_collect(k)
            st, model.skip_stats = model.skip_stats, None
            share = (f" ; stem tile-layers {st['backbone_stem_tile_layers'] / st['backbone_stem_tile_layers_dense']:.3f} of the dense count"
                     if "backbone_stem_tile_layers" in st else "")
            print(f"items <= {mi} incremental_backbone={mode}: {dt * 1e3:.1f} ms/decode = {B / dt:.1f} seq/s ; backbone {bb[0]:.1f} ms in "
                  f"{bb[1]} forwards ({bb[0] / bb[1] * 1e3:.1f} us each){share}")
