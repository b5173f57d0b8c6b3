"""A/B: the incremental stem of the backbone (Diffusion.incremental_backbone; svdd_backbone_incr2_f32 with its size-ordered list,
svdd_backbone_incr_f32 with the slot-ordered one) against the one-launch kernel at the headline configuration (SVDD-MC, B = 256,
L = 200, M = 10, 128 steps, fp32), in one process.
  1. per step, on the tokens of a real trajectory (state_trace): the summed launches of one incremental forward (work list +
     one segment launch per leading dilation-1 layer + the tail) against one launch of backbone_kernel, for every setting, with the
     share of the stem's tile-layers the step marked; every forward is first compared with the one-launch logits (torch.equal);
  2. whole decodes: incremental_backbone "off", then every setting under "auto", the whole round repeated --rounds times: wall clock
     and the backbone's profile slot.
A setting is NAME or items:residency:list — items = most row tiles per work item (1, 2, 4); residency = segment workgroups per CU
(0 = no LDS padding: 4 for items <= 2, 6 for 1-tile items, 3 for <= 4); list = slot (the old entry, one workgroup per (row, slot))
ordered (the compact list, most tiles first) or tight (svdd_backbone_incr4_f32: the ordered list built in one launch by
backbone_list_kernel, tight items on backbone_seg_tight_kernel in the dilation-1 layers; items = 2). Names: today = 2:0:slot,
today4 = 4:0:slot, A = 2:0:ordered, A3 = 2:3:ordered, B = 2:2:ordered, C = 1:3:ordered, D = 1:4:ordered, E = 1:0:ordered, T = 2:0:tight.
--depth 8,10,12: the carried layers (Diffusion.incremental_depth; 8 = the dilation-1 layers, up to 12 = through the dilation-4 layers,
svdd_backbone_incr3_f32); every setting runs at every depth given, as NAME@depth. Default: 8.
Usage: python tools/incremental_backbone_ab.py [decodes per leg, default 3] [--settings today,A,A3,B,C,D,E] [--steps 1,8,32,...]
           [--rounds 2] [--no-decodes] [--depth 8,12]
       python tools/incremental_backbone_ab.py --profile SETTING --marks marks.json [--steps ...] [--reps 5] [--depth 12]
           (for rocprofv3 --kernel-trace: per step and repeat one full forward, then ONE incremental forward; marks.json gets the
           per-layer tile and item counts of every such forward, in launch order, for tools/stem_dispatch_trace.py)"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from svdd_amd import _lib, fused, synthetic

NAMED = {"today": "2:0:slot", "today4": "4:0:slot", "A": "2:0:ordered", "A3": "2:3:ordered", "B": "2:2:ordered", "C": "1:3:ordered",
         "D": "1:4:ordered", "E": "1:0:ordered", "T": "2:0:tight"}
ap = argparse.ArgumentParser()
ap.add_argument("reps", nargs="?", type=int, default=3)
ap.add_argument("--settings", default="today,A,A3,B,C,D,E")
ap.add_argument("--steps", default="1,8,32,64,96,120,126")
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--no-decodes", action="store_true")
ap.add_argument("--profile", default=None)
ap.add_argument("--marks", default=None)
ap.add_argument("--depth", default="8")
ap.add_argument("--reps-profile", "--reps", dest="preps", type=int, default=5)
args = ap.parse_args()


def parse(name):
    mi, res, lst = NAMED.get(name, name).split(":")
    assert int(mi) in (1, 2, 4) and lst in ("slot", "ordered", "tight") and (lst != "slot" or (int(mi) != 1 and int(res) == 0)), name
    assert lst != "tight" or int(mi) == 2, name
    return name, int(mi), int(res), lst != "slot", lst == "tight"


def legs(names, depths):
    """Every setting at every depth: (NAME or NAME@depth, items, residency, ordered, depth, tight). The deep planes need the ordered list."""
    out = []
    for s in names:
        name, mi, res, ordered, tight = parse(s)
        for d in depths:
            assert d == 8 or ordered, f"{name}: depth {d} needs an ordered setting"
            out.append((name if d == 8 else f"{name}@{d}", mi, res, ordered, d, tight))
    return out


def apply(setting):
    global stem
    _, mi, res, ordered, depth, tight = setting
    fused.INCR_MAX_ITEM, fused.INCR_ORDERED = mi, ordered
    fused.set_incr_residency(res)
    model.incremental_depth, model.incremental_items = depth, "tight" if tight else "aligned"
    if stem is None or stem.lead + stem.deep != depth or stem.tight != tight:
        stem = fb.incremental_stem(B, L, depth, tight=tight)


B, L, M, S = 256, 200, 10, 128
reps = args.reps
settings = legs((args.profile or args.settings).split(","), [int(d) for d in args.depth.split(",")])
steps = [int(s) for s in args.steps.split(",")]
model, emb, head, _ = synthetic.build("dna", "cuda:0")
model.rng_mode, model.philox_seed = "philox", 0
run = lambda: model.controlled_sample(emb, head, num_steps=S, eval_sp_size=B, sample_M=M)

model.state_trace = []
if args.profile:
    model.incremental_backbone = "off"                   # the trace then holds no stem launches but the ones made below
run(); torch.cuda.synchronize()
states = [s.to("cuda:0").contiguous() for s in model.state_trace]
model.state_trace = None
fb = model._fused_backbone()
pk = fb.ol_pack()
stem = None                                              # the carried state of the depth in hand (apply)
out = torch.empty((B, L, 5), device="cuda:0")


def marks(a, b, mi, tight=False):
    """Per carried layer k of the forward a -> b: marked tiles (the brute-force rule of tests/test_backbone_incremental_gpu.py:
    tile T is marked iff a changed position lies within 4 + sum_{i<k} 4 dil[i] of one of its positions), items of at most mi tiles, and the tiles on
    the fullest of 256 CUs when the non-empty items are dealt to the CUs in turn, in (row, slot) order and largest first. tight: the
    dilation-1 layers hold the tight items of svdd_backbone_incr4_f32 instead (tests/incr4_ref.py)."""
    if tight:
        from tests import incr4_ref
    a, b = a.cpu().numpy(), b.cpu().numpy()
    lo = 16 * np.arange(13)
    hi = np.minimum(lo + 15, L - 1)
    res = []
    for k in range(1, stem.lead + stem.deep + 1):
        reach, sizes = 4 + 4 * sum(pk["dil"][:k]), []
        for r in range(a.shape[0]):
            c = np.nonzero(a[r] != b[r])[0]
            if tight and k <= stem.lead:
                sizes += [n for _, n in incr4_ref.row_items(c.tolist(), L, reach, mi)[0]]
                continue
            m = ((c[:, None] >= lo[None] - reach) & (c[:, None] <= hi[None] + reach)).any(0) & (lo <= L - 1)
            t = 0
            while t < 13:
                if not m[t]:
                    t += 1
                    continue
                n = 1
                while n < mi and t + n < 13 and m[t + n]:
                    n += 1
                sizes.append(n)
                t += n
        deal = lambda seq: int(max(np.bincount(np.arange(len(seq)) % 256, weights=seq, minlength=256))) if len(seq) else 0
        res.append({"layer": k, "tiles": int(sum(sizes)), "items": len(sizes), "fullest_slot_order": deal(sizes),
                    "fullest_largest_first": deal(sorted(sizes, reverse=True))})
    return res


if args.profile:
    apply(settings[0])
    log = []
    for i in steps:
        a, b = states[i], states[i + 1]
        ref = fused.backbone_cnn(b, pk).clone()
        for rep in range(args.preps):
            stem.valid = False
            fused.backbone_cnn_incremental(a, pk, stem, out=out)
            fused.backbone_cnn_incremental(b, pk, stem, out=out)
            torch.cuda.synchronize()
            assert torch.equal(out, ref), "the incremental forward differs from the one-launch kernel"
        log.append({"step": i, "reps": args.preps, "changed": int((a != b).sum()), "layers": marks(a, b, settings[0][1], settings[0][5])})
    json.dump({"setting": settings[0][0], "spec": NAMED.get(settings[0][0], settings[0][0]), "forwards": log}, open(args.marks, "w"))
    print(f"profile run: setting {settings[0][0]}, steps {steps}, {args.preps} forwards each ; marks -> {args.marks}")
    sys.exit(0)


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


print("settings: " + " ; ".join(f"{n} = items <= {mi}, {'no LDS padding' if not res else f'{res} / CU'}, {'ordered' if o else 'slot'} list"
                                for n, mi, res, o, _, _ in settings))
print(f"per step (us, median of 5): one launch | " + " | ".join(f"{s[0]:>6s}" for s in settings) + f" | marked share of the carried tile-layers")
for i in steps:
    if i + 1 >= len(states):
        continue
    a, b = states[i], states[i + 1]
    one = timed(lambda pre: fused.backbone_cnn(b, pk, out=out) if pre is not None else 1)
    ref = fused.backbone_cnn(b, pk).clone()
    res = []
    for st in settings:
        apply(st)

        def step(pre):
            if pre is None:                              # the planes of step i (not timed)
                stem.valid = False
                fused.backbone_cnn_incremental(a, pk, stem, out=out)
                stem.stat.zero_()
                return 1
            fused.backbone_cnn_incremental(b, pk, stem, out=out)
        step(None); step(1); torch.cuda.synchronize()
        assert torch.equal(out, ref), f"{st[0]}: the incremental forward differs from the one-launch kernel"
        res.append(timed(step))
        assert torch.equal(out, ref), f"{st[0]}: the incremental forward differs from the one-launch kernel"
    changed = int((a != b).sum())
    print(f"step {i:3d} ({changed:4d} tokens changed): {one:7.1f} | " + " | ".join(f"{r:7.1f}" for r in res) +
          f" | {int(stem.stat.sum()) / (B * 13 * (stem.lead + stem.deep)):.3f}")

if args.no_decodes:
    sys.exit(0)
for rnd in range(args.rounds):
    for st in [None] + settings:
        if st is None:
            model.incremental_backbone = "off"
        else:
            model.incremental_backbone = "auto"
            apply(st)
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
        sk, model.skip_stats = model.skip_stats, None
        share = (f" ; stem tile-layers {sk['backbone_stem_tile_layers'] / sk['backbone_stem_tile_layers_dense']:.3f} of the dense count"
                 if "backbone_stem_tile_layers" in sk else "")
        if sk.get("backbone_deep_tile_layers_dense"):
            share += f" ; deep {sk['backbone_deep_tile_layers'] / sk['backbone_deep_tile_layers_dense']:.3f}"
        print(f"round {rnd + 1} {'one launch (off)' if st is None else 'setting ' + st[0]:>16s}: {dt * 1e3:.1f} ms/decode = {B / dt:.1f} seq/s ; "
              f"backbone {bb[0]:.1f} ms in {bb[1]} forwards ({bb[0] / bb[1] * 1e3:.1f} us each){share}")
