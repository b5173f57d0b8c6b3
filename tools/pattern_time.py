"""Timing of pattern scanning (Diffusion.pattern_scores / evolve_patterns) at B = 256, L = 200, 16 patterns of widths 6 .. 20 at all
181 valid start positions (741,376 mutants), ConvGRU value net, fp32 and f16x3, in one process. Per precision, the median of
--reps calls timed with device events after one warm-up:
  (a) one pattern_scores call: per chunk of positions svdd_pattern_mutants, the windowed tower on the rows around each mutant's
      changed positions (the parents' tower output computed once; copies compacted away), GRU, tail, svdd_pattern_fold;
  (b) the same table composed from pieces that were public before this feature, in the same chunks: the mutants built with torch
      ops, FusedValueNet.forward_tokens on whole sequences;
  (c) one evolve_patterns iteration (max_iter = 1, stop = "global"): (a)'s path folded into a per-row best, one svdd_pattern_apply
      launch, the read of the `stopped` word;
  (d) the three new kernels alone at this shape (the chunks' svdd_pattern_mutants and svdd_pattern_fold launches of one call, one
      svdd_pattern_apply), as a share of (a).
(a) and (b) must give the same bits (asserted). Also printed: the largest deviation of pattern_scores from the reference's recorded
tables g42 / g43 (tests/golden/make_golden_pattern.py).
Usage: python tools/pattern_time.py [--reps 5] [--out profiles/pattern_time.txt] [--note TEXT ...]"""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from svdd_amd import ops, synthetic

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pattern_time.txt"))
ap.add_argument("--note", action="append", default=[])
args = ap.parse_args()

B, L = args.batch, 200
DEV = "cuda:0"
model, emb, head, reward = synthetic.build("dna", DEV)
gen = torch.Generator().manual_seed(0)
x = torch.randint(0, 4, (B, L), generator=gen).to(torch.uint8).to(DEV)
WIDTHS = list(range(6, 21)) + [13]                                              # 16 patterns of widths 6 .. 20
PATTERNS = [torch.randint(0, 4, (w,), generator=gen).numpy().astype(np.uint8) for w in WIDTHS]
K = len(PATTERNS)


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


def inputs():
    kind = model._pattern_kind(x, PATTERNS, None, None, None, "pattern_time")[1]
    return kind.pos_dev, kind.pat_dev, kind.widths_dev, kind.P, kind.Pc


@torch.no_grad()
def composed():
    """(b): torch-built mutants, forward_tokens on whole sequences, in pattern_scores' chunks -> [B, P, K]."""
    fn = model.value_callable(emb, head)
    pos_dev, pat_dev, widths_dev, P, Pc = inputs()
    table = torch.empty((B, P, K), device=DEV)
    col = torch.arange(L, device=DEV)
    for p0 in range(0, P, Pc):
        pc = min(Pc, P - p0)
        start = pos_dev[p0:p0 + pc].long()
        off = col[None, None, :] - start[:, None, None]                         # [pc, 1, L]: offset of a column into the window
        inside = (off >= 0) & (off < widths_dev.long()[None, :, None])          # [pc, K, L]
        fill = torch.gather(pat_dev[None].expand(pc, K, 32), 2, off.clamp(0, 31).expand(pc, K, L))
        cand = torch.where(inside[None], fill[None], x[:, None, None, :])       # [B, pc, K, L]
        table[:, p0:p0 + pc] = fn.forward_tokens(cand.reshape(B * pc * K, L).contiguous()).reshape(B, pc, K)
    return table


def new_kernels_alone():
    """(d): one call's svdd_pattern_mutants + svdd_pattern_fold launches on preallocated buffers, and one svdd_pattern_apply."""
    pos_dev, pat_dev, widths_dev, P, Pc = inputs()
    n = B * K * Pc
    cand = torch.empty((B, K * Pc, L), dtype=torch.uint8, device=DEV)
    onehot = torch.empty((n, L, 4), device=DEV)
    sc, parent = torch.randn(n, device=DEV), torch.randn(B, device=DEV)
    table = torch.empty((B, P, K), device=DEV)
    best = (torch.empty(B, device=DEV), torch.empty(B, dtype=torch.int32, device=DEV), torch.empty(B, dtype=torch.int32, device=DEV))
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    full = [p0 for p0 in range(0, P, Pc) if p0 + Pc <= P]                       # (a ragged last chunk is left out: same buffers)
    state = dict(x=x.clone(), cur=parent.clone(), bsf=torch.zeros(1, device=DEV), stopped=torch.zeros(1, dtype=torch.int32, device=DEV),
                 xb=x.clone(), sb=parent.clone())

    def mutants():
        for p0 in full:
            ops.pattern_mutants(x, pos_dev[p0:p0 + Pc], pat_dev, widths_dev, cand=cand, onehot=onehot, err=err)

    def fold():
        for p0 in full:
            ops.pattern_fold(sc, parent, P, K, p0, Pc, table=table, best=best)

    def apply():
        state["stopped"].zero_()
        ops.pattern_apply(best, pos_dev, pat_dev, widths_dev, state["x"], state["cur"], state["bsf"], state["stopped"], state["xb"],
                          state["sb"])
    return len(full), timed(mutants, args.reps), timed(fold, args.reps), timed(apply, args.reps)


def golden_deviation(precision):
    from tests import e2e_parity
    from tests.conftest import load_golden

    def dev_of(m, e, h, g):
        pats = [g["patterns"][k, :w] for k, w in enumerate(g["widths"].tolist())]
        t = m.pattern_scores(torch.from_numpy(g["x"]).to(DEV), pats, e, h, positions=g["positions"].tolist()).cpu().numpy()
        return float(np.abs(t - g["table"]).max())
    model.precision = precision
    out = {"g43": dev_of(model, emb, head, load_golden("g43_pattern_full.npz"))}
    if precision == "f32":
        out["g42"] = dev_of(*e2e_parity.tiny_engine(load_golden("nets_tiny.npz"), 50, 8, DEV), load_golden("g42_pattern_tiny.npz"))
    return out


_, _, _, P, Pc = inputs()
lines = [f"Pattern timing: B = {B}, L = {L}, {K} patterns of widths {min(WIDTHS)} .. {max(WIDTHS)} at all {P} valid starts = {B * P * K} "
         f"mutants in chunks of {Pc} positions ({B * K * Pc} rows), ConvGRU value net; median of {args.reps} (minimum in brackets), "
         "device events, one warm-up each",
         f"device: {torch.cuda.get_device_name(0)}", ""]
for precision in ("f32", "f16x3"):
    model.precision = precision
    assert model._ism_route(emb, head, None, L)[1] is not None, "the windowed route must apply at this shape"
    a_med, a_min = timed(lambda: model.pattern_scores(x, PATTERNS, emb, head), args.reps)
    b_med, b_min = timed(composed, args.reps)
    c_med, c_min = timed(lambda: model.evolve_patterns(x, PATTERNS, emb, head, max_iter=1), args.reps)
    same = bool(torch.equal(model.pattern_scores(x, PATTERNS, emb, head), composed()))
    nchunks, (m_med, m_min), (f_med, f_min), (e_med, e_min) = new_kernels_alone()
    dev_g = golden_deviation(precision)
    lines += [f"[{precision}]",
              f"(a) pattern_scores (windowed tower):                       {a_med:9.2f} ms [{a_min:.2f}] = {1e3 * a_med / (B * P * K):.2f} us per mutant",
              f"(b) composed: torch-built mutants + forward_tokens, whole: {b_med:9.2f} ms [{b_min:.2f}]",
              f"    (a) : (b) = {a_med / b_med:.3f} ((b) is {b_med / a_med:.2f} x (a)); same bits: {same}",
              f"(c) one evolve_patterns iteration (max_iter = 1, global):  {c_med:9.2f} ms [{c_min:.2f}]",
              f"(d) new kernels alone, {nchunks} chunks: svdd_pattern_mutants {m_med:.3f} ms [{m_min:.3f}], svdd_pattern_fold {f_med:.3f} ms "
              f"[{f_min:.3f}], svdd_pattern_apply (one launch) {e_med:.3f} ms [{e_min:.3f}]; mutants + fold = "
              f"{100 * (m_med + f_med) / a_med:.2f} % of (a), all three = {100 * (m_med + f_med + e_med) / a_med:.2f} %",
              "    largest |pattern_scores - reference's recorded table|: " + ", ".join(f"{k} {v:.2e}" for k, v in sorted(dev_g.items()))
              + " (bar 1e-4)",
              ""]
    text = "\n".join(lines + args.note) + "\n"
    with open(args.out, "w") as f:                                              # written as it goes: a later failure keeps what was measured
        f.write(text)
    assert same, f"[{precision}] pattern_scores and the composed table differ"
model.precision = "f32"
print(text)
