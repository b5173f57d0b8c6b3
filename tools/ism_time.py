"""Timing of in-silico mutagenesis (Diffusion.ism_scores / evolve) at the C2 shape: B = 256, L = 200, all 200 positions (153,600
mutants), ConvGRU value net, fp32 and f16x3, in one process. Per precision, the median of --reps calls timed with device events
after one warm-up:
  (a) one ism_scores call: per chunk of positions svdd_ism_mutants, the windowed tower on the mutants' row windows (the parents'
      tower output computed once), GRU, tail, svdd_ism_fold;
  (b) the same table composed from pieces that were public before this feature, in the same chunks: the mutants built with torch
      ops, FusedValueNet.forward_tokens on whole sequences, the table assembled with torch ops;
  (c) one evolve iteration (max_iter = 1, stop = "global"): (a)'s path folded into a per-row best, one svdd_evolve_apply launch,
      the read of the `stopped` word;
  (d) the three new kernels alone at this shape (the chunks' svdd_ism_mutants and svdd_ism_fold launches of one call, one
      svdd_evolve_apply), as a share of (a).
(a) and (b) must give the same bits (printed). Also printed: the largest deviation of ism_scores from the reference's recorded
tables g36 / g37 (tests/golden/make_golden_ism.py).
Usage: python tools/ism_time.py [--reps 5] [--out profiles/ism_time.txt] [--note TEXT ...]"""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from svdd_amd import ops, synthetic

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ism_time.txt"))
ap.add_argument("--note", action="append", default=[])
args = ap.parse_args()

B, L = args.batch, 200
DEV = "cuda:0"
model, emb, head, reward = synthetic.build("dna", DEV)
x = torch.randint(0, 4, (B, L), generator=torch.Generator().manual_seed(0)).to(torch.uint8).to(DEV)
pos_dev = torch.arange(L, dtype=torch.int32, device=DEV)


def timed(fn, reps):
    """Median and minimum (ms) of fn() over reps runs, each between two device events, after one warm-up."""
    fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def chunk_positions():
    kind = model._ism_kind(x, None, None)[1]
    return kind.P, kind.Pc


@torch.no_grad()
def composed():
    """(b): torch-built mutants, forward_tokens on whole sequences, torch-assembled table, in ism_scores' chunks -> [B, L, 4]."""
    fn = model.value_callable(emb, head)
    P, Pc = chunk_positions()
    parent = fn.forward_tokens(x).reshape(B)
    ism = parent[:, None, None].expand(B, P, 4).clone()
    k = torch.arange(3, device=DEV)
    rows = torch.arange(B, device=DEV)
    for p0 in range(0, P, Pc):
        pc = min(Pc, P - p0)
        pos = torch.arange(p0, p0 + pc, device=DEV)
        ref = x[:, pos].long()                                                  # [B, pc]
        alt = k[None, None, :] + (k[None, None, :] >= ref[:, :, None]).long()   # [B, pc, 3]: ACGT order, the row's own base skipped
        cand = x[:, None, None, :].repeat(1, pc, 3, 1)
        cand.scatter_(3, pos[None, :, None, None].expand(B, pc, 3, 1), alt[..., None].to(torch.uint8))
        sc = fn.forward_tokens(cand.view(B * pc * 3, L)).reshape(B, pc, 3)
        ism[rows[:, None, None], pos[None, :, None], alt] = sc
    return ism


def new_kernels_alone():
    """(d): one call's svdd_ism_mutants + svdd_ism_fold launches on preallocated buffers, and one svdd_evolve_apply."""
    P, Pc = chunk_positions()
    n = B * 3 * Pc
    cand = torch.empty((B, 3 * Pc, L), dtype=torch.uint8, device=DEV)
    onehot = torch.empty((n, L, 4), device=DEV)
    sc, parent = torch.randn(n, device=DEV), torch.randn(B, device=DEV)
    ism = torch.empty((B, P, 4), device=DEV)
    best = (torch.empty(B, device=DEV), torch.empty(B, dtype=torch.int32, device=DEV), torch.empty(B, dtype=torch.int32, device=DEV))
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    full = [p0 for p0 in range(0, P, Pc) if p0 + Pc <= P]                       # (a ragged last chunk is left out: same buffers)
    state = dict(x=x.clone(), cur=parent.clone(), bsf=torch.zeros(1, device=DEV), stopped=torch.zeros(1, dtype=torch.int32, device=DEV),
                 xb=x.clone(), sb=parent.clone())

    def mutants():
        for p0 in full:
            ops.ism_mutants(x, pos_dev[p0:p0 + Pc], cand=cand, onehot=onehot, err=err)

    def fold():
        for p0 in full:
            ops.ism_fold(sc, parent, x, pos_dev, p0, Pc, ism=ism, best=best)

    def apply():
        state["stopped"].zero_()
        ops.evolve_apply(best, state["x"], state["cur"], state["bsf"], state["stopped"], state["xb"], state["sb"])
    return len(full), timed(mutants, args.reps), timed(fold, args.reps), timed(apply, args.reps)


def golden_deviation(precision):
    from tests import e2e_parity
    from tests.conftest import load_golden
    out = {}
    g = load_golden("g37_ism_full.npz")
    model.precision = precision
    ism = model.ism_scores(torch.from_numpy(g["x"]).to(DEV), emb, head, positions=g["positions"].tolist()).cpu().numpy()
    out["g37"] = float(np.abs(ism - g["ism"]).max())
    if precision == "f32":
        g = load_golden("g36_ism_tiny.npz")
        tm, te, th = e2e_parity.tiny_engine(load_golden("nets_tiny.npz"), 50, 8, DEV)
        ism = tm.ism_scores(torch.from_numpy(g["x"]).to(DEV), te, th, positions=g["positions"].tolist()).cpu().numpy()
        out["g36"] = float(np.abs(ism - g["ism"]).max())
    return out


P, Pc = chunk_positions()
lines = [f"ISM timing: B = {B}, L = {L}, all {P} positions = {B * 3 * P} mutants in chunks of {Pc} positions ({B * 3 * Pc} rows), ConvGRU "
         f"value net; median of {args.reps} (minimum in brackets), device events, one warm-up each",
         f"device: {torch.cuda.get_device_name(0)}", ""]
for precision in ("f32", "f16x3"):
    model.precision = precision
    assert model._ism_route(emb, head, None, L)[1] is not None, "the windowed route must apply at this shape"
    a_med, a_min = timed(lambda: model.ism_scores(x, emb, head), args.reps)
    b_med, b_min = timed(composed, args.reps)
    c_med, c_min = timed(lambda: model.evolve(x, emb, head, max_iter=1), args.reps)
    same = bool(torch.equal(model.ism_scores(x, emb, head), composed()))
    nchunks, (m_med, m_min), (f_med, f_min), (e_med, e_min) = new_kernels_alone()
    dev_g = golden_deviation(precision)
    lines += [f"[{precision}]",
              f"(a) ism_scores (windowed tower):                          {a_med:9.2f} ms [{a_min:.2f}] = {1e3 * a_med / (B * 3 * P):.2f} us per mutant",
              f"(b) composed: torch-built mutants + forward_tokens, whole: {b_med:9.2f} ms [{b_min:.2f}]",
              f"    (a) : (b) = {a_med / b_med:.3f} ((b) is {b_med / a_med:.2f} x (a)); same bits: {same}",
              f"(c) one evolve iteration (max_iter = 1, global):           {c_med:9.2f} ms [{c_min:.2f}]",
              f"(d) new kernels alone, {nchunks} chunks: svdd_ism_mutants {m_med:.3f} ms [{m_min:.3f}], svdd_ism_fold {f_med:.3f} ms [{f_min:.3f}], "
              f"svdd_evolve_apply (one launch) {e_med:.3f} ms [{e_min:.3f}]; mutants + fold = {100 * (m_med + f_med) / a_med:.2f} % of (a), "
              f"all three = {100 * (m_med + f_med + e_med) / a_med:.2f} %",
              "    largest |ism_scores - reference's recorded table|: " + ", ".join(f"{k} {v:.2e}" for k, v in sorted(dev_g.items())) + " (bar 1e-4)",
              ""]
model.precision = "f32"
lines += args.note
text = "\n".join(lines) + "\n"
print(text)
with open(args.out, "w") as f:
    f.write(text)
