"""Per-launch figures of the incremental stem from a rocprofv3 --kernel-trace CSV of `tools/incremental_backbone_ab.py --profile
SETTING --marks marks.json [--depth D]`: per profiled step, the mean duration of the work-list launch(es), of each segment launch (one
per carried layer: 8 for the dilation-1 layers, up to 12 with the dilation-4 layers) by their order within a forward, of the tail kernel, and the idle time between consecutive launches of a forward — beside the marked
tiles and items per layer and the dispatch model (tiles on the fullest / the mean CU x 8.8 us per 16-row tile-layer).
--depth D: the carried layers the trace was taken with; every forward must then hold exactly D segment launches.
Usage: python tools/stem_dispatch_trace.py <kernel_trace.csv> <marks.json> [--depth D]"""
import csv
import json
import sys

TILE_US, CUS = 8.8, 256
depth = int(sys.argv[sys.argv.index("--depth") + 1]) if "--depth" in sys.argv else None
rows = sorted(csv.DictReader(open(sys.argv[1])), key=lambda r: int(r["Start_Timestamp"]))
marks = json.load(open(sys.argv[2]))
ev = [(r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in rows]
is_seg = lambda name: "backbone_seg_kernel" in name or "backbone_seg_tight_kernel" in name
starts = [i for i, e in enumerate(ev) if "backbone_worklist_kernel" in e[0] or "backbone_list_kernel" in e[0]]
forwards = []
for i in starts:                                         # work list [, order] (or the one list launch), the segment launches, the tail
    j = i + 1
    while j < len(ev) and ("backbone_order_kernel" in ev[j][0] or is_seg(ev[j][0])):
        j += 1
    assert j < len(ev) and "backbone_kernel" in ev[j][0], ev[j][0] if j < len(ev) else "trace ends inside a forward"
    forwards.append(ev[i:j + 1])
want = sum(f["reps"] for f in marks["forwards"])
assert len(forwards) == want, f"{len(forwards)} incremental forwards in the trace, {want} in {sys.argv[2]}"
us = lambda ns: ns / 1e3
mean = lambda v: sum(v) / len(v)
print(f"setting {marks['setting']} = {marks['spec']} (items : workgroups per CU, 0 = no LDS padding : list) ; model: {TILE_US} us per tile-layer on a CU, {CUS} CUs")
at = 0
for f in marks["forwards"]:
    fw = forwards[at:at + f["reps"]]
    at += f["reps"]
    nseg = sum(is_seg(e[0]) for e in fw[0])
    assert nseg == len(f["layers"]) and depth in (None, nseg), f"{nseg} segment launches, {len(f['layers'])} layers in the marks, --depth {depth}"
    head = [e for e in fw[0] if not is_seg(e[0])][:-1]
    print(f"\nstep {f['step']} ({f['changed']} tokens changed), mean of {f['reps']} forwards, us")
    for h, e in enumerate(head):
        print(f"  {e[0].replace('(anonymous namespace)::', '').split('(')[0][-44:]:>44s}  {mean([us(x[h][2] - x[h][1]) for x in fw]):7.1f}")
    tot_seg = tot_bal = tot_full = 0.0
    print("  layer  launch us | tiles  items | fullest CU: tiles  x 8.8 us | mean CU: tiles  x 8.8 us | launch - fullest | largest first: fullest tiles")
    for k in range(nseg):
        d = mean([us(x[len(head) + k][2] - x[len(head) + k][1]) for x in fw])
        m = f["layers"][k]
        full, bal = m["fullest_slot_order"] if marks["spec"].endswith("slot") else m["fullest_largest_first"], m["tiles"] / CUS
        tot_seg, tot_bal, tot_full = tot_seg + d, tot_bal + bal * TILE_US, tot_full + full * TILE_US
        dil4 = "Li4EEE" in fw[0][len(head) + k][0] or ", 4>" in fw[0][len(head) + k][0]      # the dilation-4 instantiation
        print(f"  {k + 1:4d}{'*' if dil4 else ' '}  {d:9.1f} | {m['tiles']:5d}  {m['items']:5d} | {full:17d}  {full * TILE_US:8.1f} | {bal:14.2f}  {bal * TILE_US:8.1f} | "
              f"{d - full * TILE_US:16.1f} | {m['fullest_largest_first']:5d}")
    tail = mean([us(x[-1][2] - x[-1][1]) for x in fw])
    gaps = [mean([us(x[q + 1][1] - x[q][2]) for x in fw]) for q in range(len(fw[0]) - 1)]
    span = mean([us(x[-1][2] - x[0][1]) for x in fw])
    print(f"  (* = dilation 4) segment launches {tot_seg:.1f} ; fullest-CU model {tot_full:.1f} ; balanced model {tot_bal:.1f} ; per launch above the balanced model "
          f"{(tot_seg - tot_bal) / nseg:.1f}, of which imbalance (fullest - mean) {(tot_full - tot_bal) / nseg:.1f}")
    print(f"  tail backbone_kernel<.., 2> {tail:.1f} ; idle between consecutive launches: mean {mean(gaps):.2f}, max {max(gaps):.2f}, sum {sum(gaps):.1f} ; "
          f"first start to last end {span:.1f}")
