"""Kernel level of one C2 decode (B = 256, L = 200, M = 10, 128 steps, Philox, fp32) for profiles/prior_seed_late_steps_trace.txt.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python tools/prior_seed_late_steps_trace.py --run
    python tools/prior_seed_late_steps_trace.py --read DIR/.../t_kernel_trace.csv

--run: three decodes in one process (the first fills the caches of the all-MASK row); environment variables SVDD_SEED_PRIOR=0 and
SVDD_LATE_STEPS_FROM=<fraction> give the two halves of the change alone. --read: the launches of the LAST decode (from the last
launch that starts a decode — backbone_seed_kernel, or the first-forward kernel backbone_kernel<true, false, 1> — to the end of
the trace): launches and time per kernel, the GRU launches longer than one round, the empty launches of the two-part sequence."""
import argparse
import csv
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(decodes):
    import torch
    from svdd_amd import synthetic
    model, emb, head, _ = synthetic.build("dna", "cuda:0")
    model.rng_mode, model.philox_seed = "philox", 0
    for _ in range(decodes):
        model.controlled_sample(emb, head, num_steps=128, eval_sp_size=256, sample_M=10)
        torch.cuda.synchronize()


def read(path, round_us):
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    starts = [i for i, r in enumerate(rows) if "backbone_seed_kernel" in r[2] or "backbone_kernel<true, false, 1>" in r[2]]
    first_fwd = sum(1 for r in rows if "backbone_kernel<true, false, 1>" in r[2])
    print(f"{len(rows)} launches in the trace, {len(starts)} decode starts, backbone_kernel<true, false, 1> launches: {first_fwd}")
    last = rows[starts[-1]:]
    print(f"last decode: {len(last)} launches, first start to last end {(last[-1][1] - last[0][0]) / 1e6:.3f} ms, "
          f"sum of kernel times {sum(e - s for s, e, _ in last) / 1e6:.3f} ms")
    per = {}
    for s, e, k in last:
        per.setdefault(k, []).append((e - s) / 1e3)
    for k, v in sorted(per.items(), key=lambda kv: -sum(kv[1]))[:16]:
        print(f"{k[:70]:70s} n={len(v):5d} median={statistics.median(v):9.2f} min={min(v):8.2f} max={max(v):8.2f} total={sum(v) / 1e3:8.2f}ms")
    for name in ("gru_pc_kernel", "gru_tower_parts_kernel", "conv_tower_parts_kernel"):
        v = [t for k, ts in per.items() if (name + "(") in k for t in ts]
        if v:
            print(f"{name}: {len(v)} launches, {sum(1 for t in v if t > round_us)} longer than {round_us:.0f} us, "
                  f"{sum(1 for t in v if t < 20)} under 20 us (empty: mean {statistics.mean([t for t in v if t < 20] or [0]):.2f} us)")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", action="store_true")
    ap.add_argument("--decodes", type=int, default=3)
    ap.add_argument("--read", metavar="CSV")
    ap.add_argument("--round-us", type=float, default=500.0, help="a GRU launch longer than this took more than one round")
    a = ap.parse_args()
    if a.run:
        run(a.decodes)
    if a.read:
        read(a.read, a.round_us)
