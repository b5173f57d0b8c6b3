"""bench.py — decoded sequences/sec of the SVDD-MC hot path on MI355X (BASELINE.json metric).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A plain run sets up, warms up (W decodes), times K decodes and prints ONE JSON line with the headline only: metric, value,
unit, higher_is_better, dtype, ms_per_step (wall milliseconds of one timed decode), x0_sha1, config (+ per_rank for N > 1).
--dump-outputs DIR writes what the last timed decode returned to DIR/x0.npy (the decoded tokens of the whole batch as float32
[rows, L]; a fixed, seeded sample of rows if that would exceed 64 MB). Everything else below (rooflines from per-dispatch
events, split precisions, the other BASELINE configs, saturated sizes, precision evidence, CPU baselines) runs only with --full.

`python bench.py --gpus N` with N > 1 from a bare shell (no WORLD_SIZE in the environment) starts the N ranks itself:
the parent spawns `python -m torch.distributed.run --nproc-per-node N bench.py ...` as a CHILD process before it has
touched the GPU, relays rank 0's JSON line and exits with the child's code. `--dry-run` exercises the launch, the
rendezvous, the barrier / max-over-ranks timing and the one all-gather with a stand-in decode on the host (gloo; no GPU
needed): its line says "dry_run": true and carries no throughput.

One bench "step" = one full `Diffusion.controlled_sample` decode of one batch (config 2 of
BASELINE.json: DNA enhancer SVDD-MC, batch=256 per GPU, L=200, M=10, 128 diffusion steps,
random-init dilated-CNN backbone + ConvGRU value net, synthetic all-MASK prior), from the prior to
the final x_0 including the noise-removal forward and, for N>1, the one all-gather of the decoded
tokens. Inputs are generated on the device (nothing crosses PCIe in the timed region).
Weak scaling: every rank decodes its own 256 rows (global rows rank*256 .. rank*256+255).

With --full, the ONE JSON line (rank 0) is the compact record with extra objects:
  roofline      the dominant kernel of the job by time: backbone_kernel, the whole dilated-CNN backbone forward in
                one launch (svdd_backbone_cnn_f32; exact-fp32 MFMA, activations in LDS/registers). Useful FLOPs per
                launch (20 convs: 2*B*Cin*Cout*sum_t max(0, L-|t-4|*dil) - multiplications with zero padding are
                not counted - plus the first 9-tap conv and the two 1x1 convs) / its mean launch duration, against
                the 157.3 TFLOP/s dense fp32-MFMA peak. (When the batch is too small for that kernel the
                layer-wise conv1d_cl_static_kernel is reported instead.)
  roofline_sampler  the dominant kernel of the sampler itself, K1 propose: algorithmic bytes per launch
                B*L*(21 + 17*M) / mean launch duration, against the 8 TB/s HBM peak.
                All durations are measured inside the timed region with HIP start/stop events bound to each
                dispatch on its launch stream (hipExtLaunchKernelGGL, svdd_profile_*).
  cpu_baseline  the CPU oracle port of the same workload, timed on this box's host cores on a bounded
                sample (a few diffusion steps at full batch), extrapolated to a whole decode.
  alt_precision the SAME workload with the nets' matrix products on the 16-bit matrix cores (Diffusion.precision,
                csrc/svdd_lp_*.hip), one object per mode, each with its own timed decodes and the roofline of its
                dominant kernel against the dense bf16/f16 MFMA peak. Never the headline: `value` / `dtype` above are
                the exact-fp32 path. Token agreement with the fp32 decode and the error of every mode against an fp64 forward:
                profiles/r05_precision_agreement.json (tools/precision_agreement.py), summarised in `precision_evidence`.
  config3_pm / config5_*  BASELINE.json configs[2] (SVDD-PM, L = 50) and configs[4] (TDS shard + one 2048 population, DPS) as extra
                objects: whole-decode wall clock + the roofline of the dominant kernel on EXECUTED work.
  roofline.also every other kernel fraction of the run as a compact list (the driver's record keeps `roofline` in full).
  per_rank      (N > 1) every rank's decode time and the time of the one all-gather, so that a scaling run is diagnosable.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0      # MI355X_MICROARCH.md: 8 TB/s spec
FP32_PEAK_TFLOPS = 157.3
LP_PEAK_TFLOPS = 2500.0    # dense bf16 / f16 MFMA peak (MI355X_MICROARCH.md; the 5 PF headline figure is 2:1 sparse)


class _Legs:
    """Wall seconds of every leg of the run -> `leg_seconds` of the long record (the driver's command must stay under 150 s)."""

    def __init__(self):
        self.t, self.secs = time.perf_counter(), {}

    def mark(self, name):
        now = time.perf_counter()
        self.secs[name] = round(self.secs.get(name, 0.0) + now - self.t, 2)
        self.t = now


def _digest(tokens):
    import hashlib
    return hashlib.sha1(tokens.to(torch.uint8).cpu().numpy().tobytes()).hexdigest()[:16]


DUMP_LIMIT = 60_000_000    # bytes of array data of --dump-outputs: under 64 MB in all, .npy header included


def dump_outputs(out_dir, tokens):
    """--dump-outputs: the decoded tokens the timed path returned, as float32 DIR/x0.npy; above DUMP_LIMIT a fixed, seeded
    sample of rows (sorted), so that two builds given the same arguments can be compared output for output."""
    x = tokens.cpu().numpy().astype(np.float32)
    max_rows = max(1, DUMP_LIMIT // max(x[0].nbytes, 1))
    if x.shape[0] > max_rows:
        x = x[np.sort(np.random.default_rng(0).choice(x.shape[0], max_rows, replace=False))]
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "x0.npy"), x)


def host_cpu():
    """(model name, logical cores) of the box the CPU baseline ran on (stated next to every CPU number)."""
    model = "unknown"
    try:
        with open("/proc/cpuinfo") as f:
            for ln in f:
                if ln.startswith("model name"):
                    model = ln.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    return model, os.cpu_count()


def backbone_flops(n, L, H=128):
    """Useful FLOPs of the dilated-CNN backbone forward on n sequences of length L (models/dnaconv.py:176-210): the 20 dilated
    9-tap 128->128 convs without the multiplications with zero padding, + the 9-tap first conv on the one-hot + the two 1x1 convs."""
    conv = sum(2.0 * n * H * H * sum(max(0, L - abs(t - 4) * d) for t in range(9)) for d in (1, 1, 4, 16, 64) for _ in range(4))
    return conv + 2.0 * n * L * (5 * H * 9 + H * H + H * 5)


PROFILE_SLOTS = {"propose": 0, "select": 1, "conv1d": 2, "gru": 3, "epilogue_ln": 4, "conv_tower": 5, "backbone_cnn": 6,
                 "value_tail": 7, "tds_resample": 8, "backbone_grad": 10, "gru_train": 11, "gru_bptt": 12}


def timed_decodes(run, steps, check, warm=None):
    """One warm-up decode (`warm`: a SHORT decode of the same shapes instead — a few diffusion steps pack the weights, size the
    allocator's pools and settle the clocks; used where a whole decode takes seconds), then `steps` timed ones (wall clock, device
    synchronised on both sides); the LAST one with the per-dispatch HIP events on.
    -> (seconds per decode, {kernel: (total ms, launches)} of the last decode)."""
    from svdd_amd import _lib
    (warm or run)()
    torch.cuda.synchronize()
    for k in PROFILE_SLOTS.values():
        _lib.profile_collect(k)
    t0 = time.perf_counter()
    for k in range(steps):
        if k == steps - 1:
            _lib.profile_enable(True)
        out = run()
    torch.cuda.synchronize()
    el = (time.perf_counter() - t0) / steps
    _lib.profile_enable(False)
    check(out)
    return el, {name: _lib.profile_collect(k) for name, k in PROFILE_SLOTS.items()}


def _mfma_roofline(kernel, flops, ms, launches, peak=FP32_PEAK_TFLOPS, passes=1, **extra):
    tf = flops / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
    r = {"bound": "mfma", "kernel": kernel, "achieved": round(tf, 2), "peak": peak, "unit": "TFLOP/s", "frac": round(tf / peak, 5),
         "executed_flops_per_decode": round(flops), "kernel_ms_per_decode": round(ms, 3), "launches": launches, "traffic": None}
    if passes > 1:
        r["mfma_passes"], r["issued_frac"] = passes, round(tf * passes / peak, 5)
    r.update(extra)
    return r


def config3_leg(dev, steps=1, alt="f16x3", B=256, L=50, M=10, S=128):
    """BASELINE.json configs[2]: 5'UTR RNA SVDD-PM (controlled_sample_tweedie, diffusion_gosai.py:1105-1145, 1373-1460), batch 256,
    L = 50, M = 10, ConvGRU reward, 128 steps, fp32, Philox. `value` = wall clock of whole decodes. `roofline`: its dominant
    kernel, backbone_kernel on the LIVE candidates (exact work-skipping: a candidate that unmasked nothing is its parent), useful
    FLOPs of the sequences actually forwarded — counted on the device in one extra untimed decode of the same Philox stream
    (Diffusion.skip_stats) — over the kernel's summed HIP-event time in the timed decode, against the fp32-MFMA peak."""
    try:
        from svdd_amd import synthetic
        model, _, _, rew = synthetic.build("rna", dev)
        model.rng_mode, model.philox_seed = "philox", 0
        run = lambda: model.controlled_sample_tweedie(rew, num_steps=S, eval_sp_size=B, sample_M=M, options="True")   # noqa: E731

        def check(out):
            assert out.shape == (B, L) and int(out.max()) <= 3
        el, prof = timed_decodes(run, steps, check)
        model.skip_stats = {}
        run()
        torch.cuda.synchronize()
        st, model.skip_stats = model.skip_stats, None
        seqs_fwd = st["live_candidates"] + B                      # + the one forward on the all-MASK parents
        bb_ms, bb_n = prof["backbone_cnn"]
        res = {"workload": f"5'UTR RNA SVDD-PM (tweedie), batch={B}, L={L}, M={M}, {S} steps, ConvGRU reward (BASELINE.json configs[2])",
               "value": round(B / el, 3), "unit": "sequences/s", "n_gpus": 1, "steps": steps, "ms_per_step": round(el * 1e3, 3),
               "dtype": "f32", "data": "synthetic (random-init nets, all-MASK prior)",
               "roofline": _mfma_roofline("backbone_kernel (svdd_backbone_cnn_f32 on the compacted live candidates; several L=50 sequences per tile)",
                                          backbone_flops(seqs_fwd, L), bb_ms, bb_n,
                                          sequences_forwarded=int(seqs_fwd), nominal_sequences=B * (M + 1) * S + B),
               "executed": {"live_candidates": st["live_candidates"], "candidates": st["candidates"],
                            "changed_row_steps": st["changed_row_steps"], "row_steps": st["row_steps"]},
               "own_kernels_ms_per_decode": {k: round(v[0], 3) for k, v in prof.items() if v[1]}}
        if alt:
            model.precision = alt
            el2, prof2 = timed_decodes(run, 1, check)
            passes = 3 if alt.endswith("x3") else 1
            res["alt_precision"] = {alt: {"value": round(B / el2, 3), "unit": "sequences/s", "ms_per_step": round(el2 * 1e3, 3), "steps": 1,
                                          "roofline": _mfma_roofline("backbone_lp kernel on the compacted live candidates",
                                                                     backbone_flops(seqs_fwd, L), prof2["backbone_cnn"][0], prof2["backbone_cnn"][1],
                                                                     peak=LP_PEAK_TFLOPS, passes=passes)}}
            model.precision = "f32"
        del model, rew
        torch.cuda.empty_cache()
        return res
    except Exception as e:                                     # noqa: BLE001
        return {"error": f"{type(e).__name__}: {e}"}


def config5_leg(dev, steps=1, alt="f16x3", B=256, L=200, S=128, population=2048, dps_steps=1):
    """BASELINE.json configs[4]: the TDS / DPS baselines at L = 200 (diffusion_gosai.py:938-978, 1230-1284; 980-1019, 1286-1330).
      tds_shard       one rank's 256-particle population of the 2048 (per-shard populations), alpha 0.5
      tds_population  ONE 2048-particle population on one GPU (the exact algorithm at the config's batch)
      dps             gradient guidance at B = 256, guidance scale 10 (forward + backward through backbone and reward net per step)
    Each with wall-clock `value` and the roofline of its dominant kernel on executed work: TDS = backbone_kernel (with the exact
    reuse of _tds_step one forward per step); DPS = the dilated-conv kernel of the differentiable pass (both directions)."""
    out = {}
    try:
        from svdd_amd import synthetic
        model, _, _, rew = synthetic.build("dna", dev)
        model.rng_mode, model.philox_seed = "philox", 0

        def tds(b, name, n_steps, alt_mode):
            def run():
                np.random.seed(0)
                return model.controlled_sample_TDS(rew, 0.5, num_steps=S, eval_sp_size=b)

            def check(o):
                assert o.shape == (b, L) and int(o.max()) <= 3
            def warm():
                np.random.seed(0)
                return model.controlled_sample_TDS(rew, 0.5, num_steps=8, eval_sp_size=b)
            short = warm if b > B else None                # the 2048-particle population: 2.3 s per decode
            el, prof = timed_decodes(run, n_steps, check, warm=short)
            bb_ms, bb_n = prof["backbone_cnn"]
            leg = {"workload": f"DNA enhancer TDS / SMC, {b} particles, L={L}, {S} steps, alpha=0.5, ConvGRU reward (BASELINE.json configs[4])",
                   "value": round(b / el, 3), "unit": "sequences/s", "n_gpus": 1, "steps": n_steps, "ms_per_step": round(el * 1e3, 3),
                   "dtype": "f32",
                   "roofline": _mfma_roofline(f"backbone_kernel (svdd_backbone_cnn_f32, {b} sequences per launch)",
                                              backbone_flops(b, L) * bb_n, bb_ms, bb_n, avg_launch_us=round(bb_ms / max(bb_n, 1) * 1e3, 2)),
                   "own_kernels_ms_per_decode": {k: round(v[0], 3) for k, v in prof.items() if v[1]}}
            if alt_mode:
                model.precision = alt_mode
                el2, _ = timed_decodes(run, 1, check, warm=short)
                leg["alt_precision"] = {alt_mode: {"value": round(b / el2, 3), "unit": "sequences/s", "ms_per_step": round(el2 * 1e3, 3), "steps": 1}}
                model.precision = "f32"
            out[name] = leg
        tds(B, "tds_shard", steps, alt)
        tds(population, "tds_population", 1, alt)

        # DPS: not under no_grad (it back-propagates); Philox for the categorical draw
        def run_dps():
            return model.controlled_sample_DPS(rew, 10.0, num_steps=S, eval_sp_size=B)

        def check(o):
            assert o.shape == (B, L) and int(o.max()) <= 3
        el, prof = timed_decodes(run_dps, dps_steps, check)
        H = 128
        conv_ms, conv_n = prof["conv1d"]
        conv_flops = backbone_flops(B, L) - 2.0 * B * L * (5 * H * 9 + H * H + H * 5)          # the 20 dilated convs of one pass
        out["dps"] = {"workload": f"DNA enhancer DPS (gradient guidance), batch={B}, L={L}, {S} steps, guidance scale 10, ConvGRU reward (BASELINE.json configs[4])",
                      "value": round(B / el, 3), "unit": "sequences/s", "n_gpus": 1, "steps": dps_steps, "ms_per_step": round(el * 1e3, 3),
                      "dtype": "f32", "own_kernels_ms_per_decode": {k: round(v[0], 3) for k, v in prof.items() if v[1]}}
        # how much of the decode's wall clock the hand-written kernels account for (the rest: torch element-wise ops of the
        # autograd graph between them, and launch gaps) — VERDICT r05 weak #7
        own = sum(v[0] for v in prof.values() if v[1])
        out["dps"]["attributed_frac"] = round(own / (el * 1e3), 4)
        g_ms, g_n = prof["backbone_grad"]
        f_ms, f_n = prof["backbone_cnn"]
        if g_n:
            # one launch each way (round 5): the gradient kernel is the dominant one; its useful FLOPs are the forward's (every
            # product of the forward has one transposed twin: 20 dilated convs, the 1x1 128 -> 128, the 128 -> 5 and the first conv)
            out["dps"]["roofline"] = _mfma_roofline(
                "backbone_grad_kernel (svdd_backbone_cnn_grad_f32: d loss / d onehot(x_t) through 2 x 1x1 + 20 x [ReLU', transposed dilated "
                "conv, LayerNorm backward, residual] + the first conv's transpose, one launch)",
                backbone_flops(B, L) * g_n, g_ms, g_n, avg_launch_us=round(g_ms / g_n * 1e3, 2))
            out["dps"]["rooflines"] = {"forward_save": _mfma_roofline(
                "backbone_kernel<save> (svdd_backbone_cnn_save_f32: the inference kernel's bits + x-hat / rstd / ReLU decisions saved; also serves q_xs)",
                backbone_flops(B, L) * f_n, f_ms, f_n, avg_launch_us=round(f_ms / max(f_n, 1) * 1e3, 2))}
        elif conv_n:
            out["dps"]["roofline"] = _mfma_roofline(
                "conv1d_cl_static_kernel<128,128,9,dil,200> (the 20 dilated convs of the differentiable backbone pass, forward and backward-data)",
                conv_flops / 20.0 * conv_n, conv_ms, conv_n, avg_launch_us=round(conv_ms / conv_n * 1e3, 2))
        del model, rew
        torch.cuda.empty_cache()
    except Exception as e:                                     # noqa: BLE001
        out["error"] = f"{type(e).__name__}: {e}"
    return out


def roofline_also(line):
    """Every other kernel fraction of this run in one compact list INSIDE `roofline` (the driver's record keeps `roofline` in full
    and only the names of the other objects): {kernel, where, bound, frac[, issued_frac], us | ms_per_decode}. Each entry is
    recomputable from the object of the line it names (`from`)."""
    also = []

    def add(src, kernel, where, r, ms_key="kernel_ms_per_decode"):
        if not isinstance(r, dict) or "frac" not in r:
            return
        e = {"kernel": kernel, "where": where, "bound": r.get("bound") or ("hbm" if r.get("unit") == "GB/s" else "mfma"), "frac": r["frac"], "from": src}
        if "issued_frac" in r:
            e["issued_frac"] = r["issued_frac"]
        if r.get(ms_key) is not None:
            e["ms_per_decode"] = r[ms_key]
        elif r.get("avg_launch_us") is not None:
            e["avg_launch_us"] = r["avg_launch_us"]
        elif r.get("gemm_ms_per_forward") is not None:
            e["ms_per_forward"] = r["gemm_ms_per_forward"]
        also.append(e)
    rv = line.get("roofline_value_net") or {}
    for key, name in (("conv_tower", "conv_tower2_kernel"), ("gru", "gru_pc_kernel"), ("tail", "value_tail_kernel")):
        if key in rv:
            add(f"roofline_value_net.{key}.decode", name, "C2 decode, executed rows", rv[key].get("decode"))
            add(f"roofline_value_net.{key}.dense", name, "2560 whole sequences", rv[key].get("dense"))
    add("roofline_sampler", "propose_kernel (K1)", "C2 decode (launch-bound size)", line.get("roofline_sampler"))
    add("roofline_sampler_saturated", "propose_kernel (K1)", "saturated, B=16384", line.get("roofline_sampler_saturated"))
    for i, r in enumerate(line.get("roofline_select_saturated") or []):
        add(f"roofline_select_saturated[{i}]", "select_rows_kernel (K2)", r.get("workload"), r)
    for i, r in enumerate(line.get("roofline_tds_resample") or []):
        add(f"roofline_tds_resample[{i}]", "tds_cdf + tds_gather (K4)", r.get("workload"), r)
    for mode, leg in (line.get("alt_precision") or {}).items():
        add(f"alt_precision.{mode}.roofline", "backbone_lp_t_kernel", f"C2 decode, {mode}", leg.get("roofline"))
        for key, name in (("conv_tower", "tower_lp_kernel"), ("gru", "gru_lp_kernel")):
            add(f"alt_precision.{mode}.roofline_value_net.{key}", name, f"C2 decode, {mode}", (leg.get("roofline_value_net") or {}).get(key))
    c4 = line.get("config4_enformer") or {}
    add("config4_enformer.roofline_trunk_gemm", "trunk_gemm256_kernel", "C4 shard, bf16x3", c4.get("roofline_trunk_gemm"))
    add("config4_enformer.f32.roofline_trunk_gemm", "trunk_gemm256_kernel", "C4 shard, f32", (c4.get("f32") or {}).get("roofline_trunk_gemm"))
    c3 = line.get("config3_pm") or {}
    add("config3_pm.roofline", "backbone_kernel", "C3 SVDD-PM decode, live candidates", c3.get("roofline"))
    for mode, leg in (c3.get("alt_precision") or {}).items():
        add(f"config3_pm.alt_precision.{mode}.roofline", "backbone_lp kernel", f"C3 SVDD-PM decode, {mode}", leg.get("roofline"))
    for name in ("tds_shard", "tds_population", "dps"):
        leg = line.get("config5_" + name) or {}
        add(f"config5_{name}.roofline", (leg.get("roofline") or {}).get("kernel", "").split(" ")[0], f"C5 {name}", leg.get("roofline"))
        for k, r in (leg.get("rooflines") or {}).items():
            add(f"config5_{name}.rooflines.{k}", r.get("kernel", k).split(" ")[0], f"C5 {name}", r)
    return also


def precision_evidence(model, emb, head, states, sched, modes, B, L, M, picks=(32, 96)):
    """Measured in THIS run, on states of this run's own fp32 decode: how far each precision mode's backbone logits and value scores
    are from the PyTorch modules evaluated in fp64 (the function itself, not one particular fp32 rounding of it), beside the same
    figure for the exact-fp32 kernels — so that "f16x3 is fp32-class" is a measurement in the driver's record, not a label.
    Two states (diffusion steps `picks`), B x L x 5 logits and B x M scores each. tools/precision_agreement.py is the long form."""
    import copy
    from svdd_amd import ops
    dev = states[0].device
    keep = model.precision
    out = {}
    try:
        with torch.no_grad(), torch.backends.cudnn.flags(enabled=False):
            bb64 = copy.deepcopy(model.backbone).double()
            bb64.clear_time_bias_cache()
            emb64, head64 = copy.deepcopy(emb).double(), copy.deepcopy(head).double()
            ref = []
            model.precision = "f32"
            for i in picks:
                x = states[i]
                lg64 = bb64(x.long(), torch.zeros(B, device=dev, dtype=torch.float64))
                lg32 = model._backbone_logits(x)
                cand, onehot, _ = ops.propose(lg32, x, sched[i, 2], sched[i, 1], M, ops.Rng(seed=0, row_offset=0, step=int(i)))
                sc64 = head64(emb64(onehot.double())).reshape(B, M)
                ref.append((x, lg64, cand, onehot, sc64))
            del bb64, emb64, head64
            for mode in ["f32"] + list(modes):
                model.precision = mode
                el, es, agree = 0.0, 0.0, []
                for x, lg64, cand, onehot, sc64 in ref:
                    el = max(el, float((model._backbone_logits(x).double() - lg64).abs().max()))
                    sc = model._value_scores(emb, head, onehot, B, M, cand, x)
                    es = max(es, float((sc.double() - sc64).abs().max()))
                    agree.append(float((sc.argmax(1) == sc64.argmax(1)).float().mean()))
                out[mode] = {"vs_fp64_logit_err": el, "vs_fp64_score_err": es, "selection_agreement_with_fp64": round(sum(agree) / len(agree), 5)}
        out["how"] = (f"max |error| against the PyTorch modules in fp64 on the states of diffusion steps {list(picks)} of this run's fp32 decode "
                      f"({B} x {L} x 5 logits, {B} x {M} scores per state; logits are O(1), scores O(0.01))")
    except Exception as e:                                     # noqa: BLE001
        out["error"] = f"{type(e).__name__}: {e}"
    finally:
        model.precision = keep
        torch.cuda.empty_cache()
    return out


def sampler_saturated(dev, L=200, M=10, B=16384, masked_frac=0.5, iters=100):
    """K1 (propose) at a size that leaves launch latency behind (B*M*L = 32.8 M candidate tokens, 626 MB per launch):
    the HBM fraction the north star quotes for the resample kernel is only measurable there (SURVEY.md section 7
    "launch-bound inner loop"). Same kernel, same arguments as in the decode; HIP events bound to each dispatch."""
    from svdd_amd import _lib, ops
    g = torch.Generator(device=dev).manual_seed(0)
    logits = torch.randn(B, 5, L, device=dev, generator=g).transpose(1, 2)          # the CNN backbone's memory image
    x = torch.where(torch.rand(B, L, device=dev, generator=g) < masked_frac, 4,
                    torch.randint(0, 4, (B, L), device=dev, generator=g)).to(torch.uint8)
    cand = torch.empty(B, M, L, dtype=torch.uint8, device=dev)
    onehot = torch.empty(B * M, L, 4, device=dev)
    rng = ops.Rng(seed=1, step=64)
    for _ in range(20):                                   # (the clocks take a few ms of load to settle)
        ops.propose(logits, x, 0.0078, 0.5, M, rng, cand=cand, onehot=onehot)
    torch.cuda.synchronize()
    _lib.profile_enable(True)
    for _ in range(iters):
        ops.propose(logits, x, 0.0078, 0.5, M, rng, cand=cand, onehot=onehot)
    torch.cuda.synchronize()
    _lib.profile_enable(False)
    tot, n = _lib.profile_collect(0)
    nbytes = B * L * (21 + 17 * M)
    gbs = nbytes / (tot / n * 1e-3) / 1e9
    del cand, onehot, logits
    torch.cuda.empty_cache()
    return {"bound": "hbm", "kernel": "propose_kernel (K1), saturated", "achieved": round(gbs, 1), "peak": HBM_PEAK_GBS,
            "unit": "GB/s", "frac": round(gbs / HBM_PEAK_GBS, 5), "bytes_per_launch": nbytes, "traffic": None,
            "traffic_source": None, "avg_launch_us": round(tot / n * 1e3, 2), "launches": n,
            "workload": f"B={B} L={L} M={M}, {masked_frac:.0%} of the positions masked, Philox"}


def select_saturated(dev, L=200, M=10, B=1 << 18, iters=50, near_uniform=False):
    """K2 (select + index-gather compaction: the north star's "multinomial resample with index-gather compaction") at a size
    where launch latency is gone: 2^18 rows. Algorithmic bytes per launch B*(4M + 2L + 4): the scores and the winning
    candidate row in, x_next and the index out. near_uniform: scores ~1e-7 apart, what random-init value nets produce —
    every row then needs the exact softmax (correctly rounded exp + ordered sum) instead of the argmax shortcut."""
    from svdd_amd import _lib, ops
    g = torch.Generator(device=dev).manual_seed(0)
    scores = torch.randn(B, M, device=dev, generator=g) * (1e-7 if near_uniform else 1e-2) + 0.01
    cand = torch.randint(0, 5, (B, M, L), device=dev, generator=g, dtype=torch.uint8)
    x_next = torch.empty(B, L, dtype=torch.uint8, device=dev)
    for _ in range(10):
        ops.select(scores, cand, want_soft=False, x_next=x_next)
    torch.cuda.synchronize()
    _lib.profile_collect(1)
    _lib.profile_enable(True)
    for _ in range(iters):
        ops.select(scores, cand, want_soft=False, x_next=x_next)
    torch.cuda.synchronize()
    _lib.profile_enable(False)
    tot, n = _lib.profile_collect(1)
    nbytes = B * (4 * M + 2 * L + 4)
    gbs = nbytes / (tot / n * 1e-3) / 1e9
    del cand, scores
    torch.cuda.empty_cache()
    # HBM bytes actually moved per launch, from the separate PMC passes of tools/resample_microbench.py (FETCH_SIZE x 2 + WRITE_SIZE,
    # rocprofv3 reports KB = 1024 B; MI355X_MICROARCH.md HBM section): the 200-byte rows gathered at arbitrary offsets over-fetch
    traffic, src = None, None
    if (B, L, M) == (1 << 18, 200, 10):
        traffic = (2 * 46138.3 + 52279.8) * 1024
        src = ("profiles/r05_pmc_k2_raw.txt (round 5's passes; the kernel is unchanged), row stride 200 (separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of "
               "tools/resample_microbench.py one 10 0, not measured in this run)")
    return {"bound": "hbm", "kernel": "select_rows_kernel (K2: softmax over M, argmax, index-gather compaction), saturated",
            "achieved": round(gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(gbs / HBM_PEAK_GBS, 5),
            "bytes_per_launch": nbytes, "traffic": None if traffic is None else round(traffic), "traffic_source": src,
            "avg_launch_us": round(tot / n * 1e3, 2),
            "launches": n, "workload": f"B={B} L={L} M={M}, scores {'~1e-7 apart (exact softmax in every row)' if near_uniform else 'N(0.01, 1e-2)'}"}


def tds_saturated(dev, L=200, B=65536, iters=10):
    """K4 (SMC/TDS resample) at B = 65536 particles and at BASELINE configs[4]'s 2048. Bytes B*(2L + 24). Its float64 cumsum
    is a serial chain by numpy's definition (np.random.choice), so the kernel is latency-bound, not HBM-bound: the figure
    is reported for completeness."""
    from svdd_amd import _lib, ops
    out = []
    for b in (2048, B):
        g = torch.Generator(device=dev).manual_seed(0)
        num, den = torch.randn(b, device=dev, generator=g) * 0.1, torch.randn(b, device=dev, generator=g) * 0.1
        sample = torch.randint(0, 5, (b, L), device=dev, generator=g, dtype=torch.uint8)
        u = torch.rand(b, device=dev, generator=g, dtype=torch.float64)
        for _ in range(3):
            ops.tds_resample(num, den, 0.5, sample, u)
        torch.cuda.synchronize()
        _lib.profile_collect(8)
        _lib.profile_enable(True)
        for _ in range(iters):
            ops.tds_resample(num, den, 0.5, sample, u)
        torch.cuda.synchronize()
        _lib.profile_enable(False)
        tot, n = _lib.profile_collect(8)
        nbytes = b * (2 * L + 24)
        gbs = nbytes / (tot / n * 1e-3) / 1e9
        out.append({"bound": "hbm", "kernel": "tds_cdf_kernel + tds_gather_kernel (K4)", "achieved": round(gbs, 2),
                    "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(gbs / HBM_PEAK_GBS, 6), "bytes_per_launch": nbytes,
                    "traffic": None, "traffic_source": None, "avg_launch_us": round(tot / n * 1e3, 2), "launches": n,
                    "workload": f"B={b} particles, L={L}",
                    "note": "serial float64 cumsum of B terms (numpy's order) bounds it: latency, not bandwidth"})
    return out


def trunk_gemm_roofline(model, emb, head, dev, n, L, precision="bf16x3"):
    """--value-net enformer: the dominant kernel of that workload is trunk_gemm256_kernel (csrc/svdd_trunk.hip), not the
    backbone. One trunk forward (bf16x3) on n candidates (~ the live candidates of a step) with a HIP event pair around every
    GEMM launch: multiply-adds of all GEMMs x 2 / summed launch time against the dense 16-bit MFMA peak — `frac` on the
    fp32-equivalent FLOPs, `issued_frac` with the three passes of the split product counted."""
    from svdd_amd.fused_trunk import FusedEnformerValueNet
    model.precision = precision
    fn = model.value_callable(emb, head)
    model.precision = "f32"
    if not isinstance(fn, FusedEnformerValueNet):
        return None
    f32 = precision == "f32"
    peak, passes = (FP32_PEAK_TFLOPS, 1) if f32 else (LP_PEAK_TFLOPS, 3)
    tok = torch.randint(0, 5, (n, L), device=dev, dtype=torch.uint8)
    streams, fn.tower_streams = fn.tower_streams, 1        # one chain of kernels: on two streams the GEMMs of the two half batches
    fn.forward_tokens(tok)                                 # overlap, and per-launch event pairs would count the shared time twice
    torch.cuda.synchronize()
    fn.timing = []
    fn.forward_tokens(tok)
    torch.cuda.synchronize()
    fn.tower_streams = streams
    issued = sum(2.0 * Mr * N * C * T for Mr, N, C, T, _, _ in fn.timing)          # incl. the zero rows between sequences
    ms = sum(e0.elapsed_time(e1) for _, _, _, _, e0, e1 in fn.timing)
    launches = len(fn.timing)
    fn.timing = None
    flops = float(emb.flops_per_sequence(L)) * n                                   # algorithmic (3.36 GFLOP / candidate)
    tf = flops / (ms * 1e-3) / 1e12
    return {"bound": "mfma", "kernel": "trunk_gemm256_kernel (every convolution / projection of the Enformer-shaped value trunk; " +
                                       ("fp32 operand plane, v_mfma_f32_16x16x4_f32)" if f32 else "bf16x3: 3 MFMA passes per product)"),
            "achieved": round(tf, 2), "peak": peak, "unit": "TFLOP/s", "frac": round(tf / peak, 5),
            "issued_frac": round(passes * issued / (ms * 1e-3) / 1e12 / peak, 5), "flops_per_forward": round(flops),
            "issued_flops_per_forward_incl_pad_rows": round(issued), "gemm_ms_per_forward": round(ms, 3),
            "launches": launches, "workload": f"one trunk forward on {n} candidates of length {L}", "traffic": None,
            "traffic_source": None}


def config4_leg(dev, steps, B=256, L=200, M=20, S=128, f32_steps=1):
    """BASELINE.json configs[3] at its per-GPU shard size (B = 256 of the 2048, M = 20, the Enformer-shaped 230 M-parameter
    value trunk) as an extra object of the default line: one warm-up decode + `steps` timed decodes in bf16x3 (split bf16
    operands: a 16-bit operand, 1e-5-class error — not fp32-class) and, beside it (`f32`), at the reference's own precision on the fp32-plane form of the same kernels (round 4).
    Reported beside the headline, never in it; a failure here is recorded, not raised."""
    try:
        from svdd_amd import synthetic
        from svdd_amd.fused_trunk import FusedEnformerValueNet
        model, emb, head, _ = synthetic.build("dna", dev, value="enformer")
        model.rng_mode, model.philox_seed, model.precision = "philox", 0, "bf16x3"
        assert isinstance(model.value_callable(emb, head), FusedEnformerValueNet)
        run = lambda: model.controlled_sample(emb, head, num_steps=S, eval_sp_size=B, sample_M=M)   # noqa: E731
        model.controlled_sample(emb, head, num_steps=8, eval_sp_size=B, sample_M=M)     # warm-up: 8 steps of the same shapes (a whole decode is 3 s)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            out = run()
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        assert out.shape == (B, L) and int(out.max()) <= 3
        res = {"workload": f"DNA enhancer SVDD-MC, batch={B}/GPU, L={L}, M={M}, {S} steps, Enformer-shaped value trunk "
                           "(230M params) — BASELINE.json configs[3] per-GPU shard", "value": round(B * steps / el, 3),
               "unit": "sequences/s", "n_gpus": 1, "steps": steps, "ms_per_step": round(el / steps * 1e3, 3), "dtype": "bf16x3",
               "arithmetic": "value trunk: fp32 operands split hi+lo in bf16 (16-bit operand: 1e-5-class error, not fp32-class), 3 MFMA passes, "
                             "fp32 accumulate; backbone: the same split (backbone_lp_t_kernel)", "data": "synthetic (random-init nets, all-MASK prior)"}
        try:                                                   # the dominant kernel of THIS workload, measured in this run
            res["roofline_trunk_gemm"] = trunk_gemm_roofline(model, emb, head, dev, int(0.75 * B * M), L)
        except Exception as e:                                 # noqa: BLE001
            res["roofline_trunk_gemm"] = {"error": f"{type(e).__name__}: {e}"}
        if f32_steps > 0:
            res["f32"] = config4_f32(model, emb, head, dev, f32_steps, B, L, M, S)
        del model, emb, head
        torch.cuda.empty_cache()
        return res
    except Exception as e:                                     # noqa: BLE001
        return {"error": f"{type(e).__name__}: {e}"}


def config4_f32(model, emb, head, dev, steps, B, L, M, S):
    """configs[3]'s shard at the REFERENCE's precision (fp32 value trunk): `steps` timed decodes after one warm-up. Which
    implementation ran is stated: the hand-written fp32 trunk kernels when Diffusion routes precision="f32" to them, else the
    PyTorch-ROCm modules (MIOpen / hipBLASLt)."""
    try:
        from svdd_amd.fused_trunk import FusedEnformerValueNet
        model.precision = "f32"
        fn = model.value_callable(emb, head)
        impl = ("hand-written fp32 trunk kernels (svdd_trunk.hip: one fp32 operand plane, v_mfma_f32_16x16x4_f32)" if isinstance(fn, FusedEnformerValueNet)
                else "PyTorch-ROCm modules (MIOpen / hipBLASLt), one [B*M] forward per step")
        run = lambda: model.controlled_sample(emb, head, num_steps=S, eval_sp_size=B, sample_M=M)   # noqa: E731
        model.controlled_sample(emb, head, num_steps=8, eval_sp_size=B, sample_M=M)     # warm-up: 8 steps of the same shapes (a whole decode is 10 s)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            out = run()
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        assert out.shape == (B, L) and int(out.max()) <= 3
        res = {"value": round(B * steps / el, 3), "unit": "sequences/s", "steps": steps, "ms_per_step": round(el / steps * 1e3, 3),
               "dtype": "f32", "value_trunk": impl, "warmup": "8 diffusion steps of the same shapes"}
        if isinstance(fn, FusedEnformerValueNet):
            res["roofline_trunk_gemm"] = trunk_gemm_roofline(model, emb, head, dev, int(0.75 * B * M), L, precision="f32")
        return res
    except Exception as e:                                     # noqa: BLE001
        return {"error": f"{type(e).__name__}: {e}"}


def _cpu_step(orc, model, emb, head, sched, x, i, M):
    """One SVDD-MC step of the CPU port (oracle/: backbone forward, propose, M value-net calls of batch B like
    diffusion_gosai.py:1207-1209, select) on state x at diffusion step i -> seconds."""
    B, L = x.shape
    t0 = time.perf_counter()
    with torch.no_grad():
        logits = model.backbone(torch.from_numpy(x.astype(np.int64)), torch.zeros(B)).contiguous().numpy()
    cand, onehot, _ = orc.propose(logits, x, sched[i, 2], sched[i, 1], M, seed=1, step=int(i), want_q=False)
    oh = onehot.reshape(B, M, L, 4)
    with torch.no_grad():
        sc = np.stack([head(emb(torch.from_numpy(np.ascontiguousarray(oh[:, m])))).reshape(-1).numpy() for m in range(M)], 1)
    orc.select(sc, cand)
    return time.perf_counter() - t0


SWEEP_THREADS = (8, 16, 32)
SWEEP_TIE = 0.05           # thread counts within 5 % of the fastest are a tie; ties go to the count nearest 16


def choose_threads(sweep, prefer=16, tie=SWEEP_TIE):
    """The thread count the CPU baseline runs on, by RULE (round 5 picked it on a 1.4 % race between 8 and 16 on a shared host):
    the fastest per-thread-count MINIMUM of the sweep; every count within `tie` of it is a tie, and ties go to the count nearest
    `prefer` (16: the fastest on every box seen in rounds 4-5 whenever the host was quiet)."""
    best = min(sweep.values())
    tied = [t for t, s in sweep.items() if s <= best * (1.0 + tie)]
    return min(tied, key=lambda t: (abs(t - prefer), t))


def cpu_thread_sweep(B, L, M, S, seed, candidates=SWEEP_THREADS, reps=3):
    """Seconds per WHOLE step of the CPU port (the same _cpu_step the baseline times) at full batch on a half-masked state, for each
    torch thread count that fits this host: one warm-up step per count, then `reps` rounds over all counts (interleaved, so that a
    burst of host load does not land on one count), per-count minimum. -> {threads: seconds}"""
    from oracle import svdd_oracle as orc
    from svdd_amd import synthetic
    model, emb, head, _ = synthetic.build("dna" if L == 200 else "rna", "cpu", seed=seed)
    sched = model._schedule(S, 1e-5)[0]
    rng = np.random.default_rng(0)
    x = np.where(rng.random((B, L)) < 0.5, orc.MASK, rng.integers(0, 4, (B, L))).astype(np.uint8)
    ncpu = os.cpu_count() or 1
    counts = sorted({min(c, ncpu) for c in candidates})
    sweep = {t: [] for t in counts}
    for rep in range(reps + 1):
        for t in counts:
            torch.set_num_threads(t)
            s = _cpu_step(orc, model, emb, head, sched, x, S // 2, M)
            if rep:                                            # rep 0 = warm-up at this count
                sweep[t].append(s)
    return {t: round(min(v), 4) for t, v in sweep.items()}


def cpu_thread_sweep_subprocess(B, L, M, S, seed):
    """cpu_thread_sweep in a fresh interpreter (`python bench.py --cpu-sweep-only B L M S seed`), so that this process's OpenMP pool
    never grows beyond the thread count the baseline runs on -> {threads: seconds} or None."""
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--cpu-sweep-only", str(B), str(L), str(M), str(S), str(seed)],
                           capture_output=True, text=True, timeout=300)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        return {int(k): float(v) for k, v in json.loads(line).items()}
    except Exception:                                          # noqa: BLE001
        return None


def cpu_baseline(B, L, M, S, sample_steps, seed=44, threads=None, states=None, passes=3):
    """Oracle (CPU port of the reference path: M value-net calls of batch B per step, like
    diffusion_gosai.py:1207-1209) on `sample_steps` diffusion steps of the same workload. `states`: the x_t of every
    step of a GPU decode of this very workload — the sampled steps then run on the real states of the trajectory
    (real masked fractions, real tokens) rather than on synthetic ones.
    threads = None: chosen by rule from a sweep in a child process (cpu_thread_sweep, choose_threads), recorded as `thread_sweep`;
    `sweep_predicted_s_per_step` (the sweep's minimum at the chosen count) stands beside the measured `s_per_step`, so that a
    loaded host shows in the record."""
    from oracle import svdd_oracle as orc
    from svdd_amd import synthetic
    model, emb, head, _ = synthetic.build("dna" if L == 200 else "rna", "cpu", seed=seed)
    sweep = None
    if threads is None:
        sweep = cpu_thread_sweep_subprocess(B, L, M, S, seed) or cpu_thread_sweep(B, L, M, S, seed)
        threads = choose_threads(sweep)
    threads = max(1, min(threads, os.cpu_count() or 1))
    torch.set_num_threads(threads)
    sched = model._schedule(S, 1e-5)[0]
    picks = np.linspace(0, S - 1, sample_steps).astype(int)
    rng = np.random.default_rng(0)
    per_pass, all_steps, work_s = [], [], 0.0
    _cpu_step(orc, model, emb, head, sched, np.full((B, L), orc.MASK, np.uint8), 0, M)       # warm-up at this thread count (untimed)
    for _ in range(max(1, passes)):
        x = np.full((B, L), orc.MASK, np.uint8)
        t_steps = []
        for i in picks:
            if states is not None:
                x = states[int(i)]
            else:                      # a state with the masked fraction step i would see (move chance ~ t_i)
                frac = 1.0 - i / S
                x = np.where(rng.random((B, L)) < frac, orc.MASK, rng.integers(0, 4, (B, L))).astype(np.uint8)
            t_steps.append(_cpu_step(orc, model, emb, head, sched, x, i, M))
        t0 = time.perf_counter()
        with torch.no_grad():
            logits = model.backbone(torch.from_numpy(x.astype(np.int64)), torch.zeros(B)).contiguous().numpy()
        orc.finalize(logits, x)
        t_final = time.perf_counter() - t0
        per_pass.append(float(np.mean(t_steps)) * S + t_final)
        all_steps += t_steps
        work_s += sum(t_steps) + t_final
    per_decode = float(np.median(per_pass))
    cpu_model, cpu_total = host_cpu()
    values = [B / t for t in per_pass]
    out = {
        "value": round(B / per_decode, 4), "unit": "sequences/s", "cores": threads,
        "cpu_model": cpu_model, "cores_total": cpu_total,
        "s_per_step": round(float(np.median(all_steps)), 4),
        "sweep_predicted_s_per_step": None if sweep is None else sweep.get(threads),
        "thread_sweep": None if sweep is None else {"s_per_step_of_the_nets_by_threads": sweep, "chosen": threads,
                                                    "rule": f"per-count minimum of 3 interleaved rounds of one whole CPU step (half-masked state) after a warm-up, in a child process; "
                                                            f"fastest wins, counts within {SWEEP_TIE:.0%} tie and ties go to the count nearest 16"},
        "kind": "port", "passes": len(per_pass), "seq_per_s_each_pass": [round(v, 4) for v in values],
        "spread": round((max(values) - min(values)) / max(values), 4),
        "sample_short": f"median of {len(per_pass)} passes x {sample_steps} of {S} steps (states of a GPU decode) at B={B} L={L} M={M}, scaled to a decode; {work_s:.0f} s CPU",
        "sample": f"median of {len(per_pass)} passes over {sample_steps} of {S} diffusion steps (evenly spaced, on the {'states of a GPU decode of this workload' if states is not None else 'synthetic states'}) "
                  f"at full batch (B={B}, L={L}, M={M}) + the noise-removal forward, scaled by {S}/{sample_steps} to one decode; "
                  f"{work_s:.1f} s of CPU work in all",
    }
    if sweep is not None and out["sweep_predicted_s_per_step"]:
        ratio = out["s_per_step"] / out["sweep_predicted_s_per_step"]
        out["measured_over_predicted"] = round(ratio, 3)
        if ratio > 1.2:
            out["host_load_note"] = "measured step > 1.2 x the sweep's minimum at the same thread count: the host (shared by the pod's GPU tenants) was loaded during the passes"
    return out


def value_net_roofline(model, emb, head, dev, B, L, M, S, tower_ms, tower_launches, gru_ms, gru_launches):
    """The #2 / #3 kernels of the headline decode (conv_tower2_kernel, gru_pc_kernel: the value net's conv tower and its
    bidirectional GRU, ~29 % of the decode) against the fp32-MFMA peak, two ways:
      decode  EXECUTED FLOPs of one decode / the kernels' summed HIP-event time in the profiled timed decode. The work-skipping
              decode runs the tower only on the candidates' row windows and the GRU only on the live candidates; both counts are
              summed on the device (Diffusion.skip_stats: tower_window_rows, live_candidates) in one extra, untimed decode of the
              same Philox stream (= the same work as the timed one).
      dense   the same kernels on B*M whole sequences (n = 2560 at config 2: every row tile live, 320 GRU units on 256 CUs) —
              the figures DESIGN.md section 4 quotes."""
    from svdd_amd import _lib, ops
    from svdd_amd.fused import FusedValueNet
    fn = model.value_callable(emb, head)
    if not (isinstance(fn, FusedValueNet) and fn.kernels_ok(L)):
        return None
    C = 64
    tower_row = 2.0 * (4 * C * 15 + 5 * C * C * 5)             # stem 4->64 x 15 taps + five 64->64 x 5-tap blocks, per sequence row
    gru_row = 2.0 * 2 * 3 * (C * C + C * C)                    # 2 directions x 3 gates x (W_ih + W_hh), per row
    # kernel times of THIS decode, with the late steps' two-part pipeline off: there the second part's GRU co-runs with the first
    # part's tower on two streams (FusedValueNet.split_gru_rounds), and per-dispatch durations of co-running kernels add up to more
    # than the wall time they take — the fractions below are kernel-exclusive
    split_was, fn.split_gru_rounds = fn.split_gru_rounds, False
    for k in (3, 5):
        _lib.profile_collect(k)
    model.skip_stats = {}
    _lib.profile_enable(True)
    model.controlled_sample(emb, head, num_steps=S, eval_sp_size=B, sample_M=M)
    torch.cuda.synchronize()
    _lib.profile_enable(False)
    fn.split_gru_rounds = split_was
    st, model.skip_stats = model.skip_stats, None
    (tower_ms, tower_launches), (gru_ms, gru_launches) = _lib.profile_collect(5), _lib.profile_collect(3)
    tail_ms, tail_launches = _lib.profile_collect(7)
    tail_row = 2.0 * C * 2 * C                                  # the 64 -> 128 map of the FFN on the matrix cores, per row
    for k in (0, 1, 6):
        _lib.profile_collect(k)
    out = {"timing": "per-dispatch HIP events of one extra decode of the same Philox stream with the value net as ONE part per step "
                     "(kernel-exclusive; the timed decodes run the late steps as two parts on two streams, DESIGN section 4b)"}
    # + the parents' pass on the all-MASK prior: ONE row when Diffusion.dedup_prior applies (B identical rows evaluated once), else B
    prior_rows = 1 if (model.dedup_prior and B > 1) else B
    rows_t = (st.get("tower_window_rows") or 0) + 2 * prior_rows * L   # forward_tokens(x) for the parents' scores + the first parent_out tower pass
    rows_g = (st["live_candidates"] + prior_rows) * L
    for key, kern, flops, ms, n in (("conv_tower", "conv_tower2_kernel (value net: stem + 5 residual conv blocks; candidates' row windows)",
                                     tower_row * rows_t, tower_ms, tower_launches),
                                    ("gru", "gru_pc_kernel (value net: bidirectional GRU 64 -> 64; live candidates only)",
                                     gru_row * rows_g, gru_ms, gru_launches),
                                    ("tail", "value_tail_kernel (value net after the GRU: direction sum + LayerNorm + FFN 64 -> 128 + ReLU + collapsed head + "
                                             "mean over length; live candidates only; fp32 MFMA and the vector ALU share one datapath, the non-MFMA third adds on top)",
                                     tail_row * rows_g, tail_ms, tail_launches)):
        tf = flops / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
        out[key] = {"bound": "mfma", "kernel": kern, "decode": {
            "achieved": round(tf, 2), "peak": FP32_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": round(tf / FP32_PEAK_TFLOPS, 5),
            "executed_flops_per_decode": round(flops), "kernel_ms_per_decode": round(ms, 3), "launches": n}}
    out["executed"] = {"tower_rows": int(rows_t), "gru_rows": int(rows_g), "nominal_rows": B * M * L * S,
                       "live_candidates": st["live_candidates"], "candidates": st["candidates"],
                       "flops_per_tower_row": tower_row, "flops_per_gru_row": gru_row, "flops_per_tail_row": tail_row}
    # dense: whole sequences
    n = B * M
    tok = torch.randint(0, 5, (n, L), device=dev, dtype=torch.uint8)
    for _ in range(3):
        fn.forward_tokens(tok)
    torch.cuda.synchronize()
    for k in (3, 5, 7):
        _lib.profile_collect(k)
    _lib.profile_enable(True)
    for _ in range(10):
        fn.forward_tokens(tok)
    torch.cuda.synchronize()
    _lib.profile_enable(False)
    for key, slot, per_row in (("conv_tower", 5, tower_row), ("gru", 3, gru_row), ("tail", 7, tail_row)):
        tot, k = _lib.profile_collect(slot)
        ms = tot / max(k, 1)
        tf = per_row * n * L / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
        out[key]["dense"] = {"achieved": round(tf, 2), "peak": FP32_PEAK_TFLOPS, "unit": "TFLOP/s",
                             "frac": round(tf / FP32_PEAK_TFLOPS, 5), "flops_per_launch": round(per_row * n * L),
                             "avg_launch_us": round(ms * 1e3, 2), "launches": k, "workload": f"{n} whole sequences of length {L}"}
    # the GRU at one (tile of 16 sequences, direction) unit per CU: 2048 sequences = 256 units (n = 2560 makes 320 units on 256 CUs:
    # 64 CUs run two); most steps of the work-skipping decode have <= 2048 live candidates
    n2 = 2048
    for _ in range(3):
        fn.forward_tokens(tok[:n2].contiguous())
    torch.cuda.synchronize()
    _lib.profile_collect(3)
    _lib.profile_enable(True)
    for _ in range(10):
        fn.forward_tokens(tok[:n2].contiguous())
    torch.cuda.synchronize()
    _lib.profile_enable(False)
    tot, k = _lib.profile_collect(3)
    ms = tot / max(k, 1)
    tf = gru_row * n2 * L / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
    out["gru"]["dense_2048"] = {"achieved": round(tf, 2), "peak": FP32_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": round(tf / FP32_PEAK_TFLOPS, 5),
                                "flops_per_launch": round(gru_row * n2 * L), "avg_launch_us": round(ms * 1e3, 2), "launches": k,
                                "workload": f"{n2} whole sequences of length {L} (one unit per CU)"}
    _lib.profile_collect(5)
    _lib.profile_collect(7)
    return out


def replay_leg(model, emb, head, B, L, M, S, decodes=2):
    """The parity mode at speed: the SAME workload with rng_mode = "replay" — the categorical uniforms are torch's global CPU
    mt19937 stream (what the reference's rand_like consumes, diffusion_gosai.py:33), continued on the device by
    svdd_mt19937_uniform_f32 for the span of a decode. Token-exact against the reference's own runs (tests/test_e2e_gpu.py);
    here only its throughput, next to the host replay of rounds 1-3 (torch.rand + a 10 MB upload per step)."""
    out = {}
    keep = (model.rng_mode, model.replay_rng)
    try:
        for how in ("device", "host"):
            model.rng_mode, model.replay_rng = "replay", how
            torch.manual_seed(0)
            model.controlled_sample(emb, head, num_steps=S, eval_sp_size=B, sample_M=M)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(decodes):
                model.controlled_sample(emb, head, num_steps=S, eval_sp_size=B, sample_M=M)
            torch.cuda.synchronize()
            el = (time.perf_counter() - t0) / decodes
            out[how] = {"value": round(B / el, 3), "unit": "sequences/s", "ms_per_step": round(el * 1e3, 3), "steps": decodes}
    finally:
        model.rng_mode, model.replay_rng = keep
    out["note"] = ("device: torch's CPU generator state uploaded once per decode, stream generated by one workgroup a step ahead on a "
                   "side stream, state written back at the end; host: torch.rand(M, B, 5, L) + upload every step")
    return out


def small_batch_leg(model, emb, head, L, S, decodes=3):
    """BASELINE.json configs[0]'s shape on the GPU (B = 4, M = 2: the reference's own CPU-runnable case): a batch this small
    runs the backbone on 4 workgroups per sequence (svdd_backbone_cnn_f32's small-batch form, same bits); the one-workgroup
    form is timed beside it (svdd_set_option(SVDD_OPT_BACKBONE_SPLIT, 1))."""
    from svdd_amd import _lib
    B, M = 4, 2
    out = {"workload": f"DNA enhancer SVDD-MC, batch={B}, L={L}, M={M}, {S} steps (BASELINE.json configs[0]) on one MI355X"}
    was = _lib.current_option(7)
    try:
        for name, opt in (("backbone_on_4_workgroups_per_sequence", 0), ("backbone_on_1_workgroup_per_sequence", 1)):
            _lib.set_option(7, opt)
            model.controlled_sample(emb, head, num_steps=S, eval_sp_size=B, sample_M=M)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(decodes):
                model.controlled_sample(emb, head, num_steps=S, eval_sp_size=B, sample_M=M)
            torch.cuda.synchronize()
            el = (time.perf_counter() - t0) / decodes
            out[name] = {"value": round(B / el, 3), "unit": "sequences/s", "ms_per_step": round(el * 1e3, 3), "steps": decodes}
    finally:
        _lib.set_option(7, was)
    return out


def cpu_baseline_c1(passes=3, threads=8):
    """BASELINE.md section 2's stated CPU baseline: the WHOLE decode of BASELINE.json configs[0] (B = 4, L = 200, M = 2, 128
    steps + noise removal) by the oracle port (CPU restatement of the reference path, PyTorch CPU modules for the nets), median
    of `passes`; cores stated. (The C2 sample in `cpu_baseline` is the same code at the headline batch.)"""
    from oracle import svdd_oracle as orc
    from svdd_amd import synthetic
    B, L, M, S = 4, 200, 2, 128
    threads = max(1, min(threads, os.cpu_count() or 1))
    torch.set_num_threads(threads)
    model, emb, head, _ = synthetic.build("dna", "cpu")
    sched = model._schedule(S, 1e-5)[0]
    bb = lambda x: model.backbone(x, torch.zeros(x.shape[0]))                               # noqa: E731
    val = lambda oh: head(emb(oh)).reshape(-1)                                              # noqa: E731
    times = []
    for p in range(passes):
        x = np.full((B, L), orc.MASK, np.uint8)
        t0 = time.perf_counter()
        with torch.no_grad():
            for i in range(S):
                logits = bb(torch.from_numpy(x.astype(np.int64))).contiguous().numpy()
                cand, onehot, _ = orc.propose(logits, x, sched[i, 2], sched[i, 1], M, seed=p, step=i, want_q=False)
                oh = onehot.reshape(B, M, L, 4)
                sc = np.stack([val(torch.from_numpy(np.ascontiguousarray(oh[:, m]))).numpy() for m in range(M)], 1)
                x = orc.select(sc, cand)[0]
            logits = bb(torch.from_numpy(x.astype(np.int64))).contiguous().numpy()
            x0 = orc.finalize(logits, x)
        times.append(time.perf_counter() - t0)
        assert x0.shape == (B, L) and int(x0.max()) <= 3
    cpu_model, cpu_total = host_cpu()
    med = float(np.median(times))
    return {"value": round(B / med, 4), "unit": "sequences/s", "cores": threads, "cpu_model": cpu_model, "cores_total": cpu_total,
            "kind": "port", "passes": passes, "s_per_decode_each_pass": [round(t, 3) for t in times],
            "sample": f"whole decodes of BASELINE.json configs[0] (B={B}, L={L}, M={M}, {S} steps + noise removal), median of {passes}"}


COMPACT_LIMIT = 6144       # bytes: the driver's record keeps the LAST ~8 KB of stdout; round 5's 24.9 KB line was cut mid-object


def _r(v, nd=4):
    return round(float(v), nd) if isinstance(v, (int, float)) and not isinstance(v, bool) else v


def _short_where(w):
    """`where` of a roofline.also entry as a short code: c2 / c3 / c4 / c5 = BASELINE.json configs[1..4]; sat = saturated size."""
    w = str(w or "")
    for a, b in (("C2 decode, executed rows", "c2"), ("C2 decode (launch-bound size)", "c2"), ("C2 decode, ", "c2 "),
                 ("2560 whole sequences", "dense2560"), ("saturated, B=16384", "sat B=16384"),
                 ("C3 SVDD-PM decode, live candidates", "c3"), ("C3 SVDD-PM decode, ", "c3 "), ("C4 shard, ", "c4 "),
                 ("C5 tds_shard", "c5 tds256"), ("C5 tds_population", "c5 tds2048"), ("C5 dps", "c5 dps"),
                 (", scores ~1e-7 apart (exact softmax in every row)", " tied"), (", scores N(0.01, 1e-2)", ""),
                 ("B=262144 L=200 ", "sat 2^18 "), (" particles, L=200", "")):
        w = w.replace(a, b)
    return w[:28]


def _short_also(also):
    out = []
    for e in also or []:
        s = {"k": str(e.get("kernel", "")).split(" ")[0].replace("_kernel", "")[:22], "w": _short_where(e.get("where")), "frac": _r(e.get("frac"))}
        if e.get("issued_frac") is not None and e["issued_frac"] != e.get("frac"):
            s["issued"] = _r(e["issued_frac"])
        if e.get("avg_launch_us") is not None:
            s["us"] = _r(e["avg_launch_us"], 1)
        else:
            ms = e.get("ms_per_decode", e.get("ms_per_forward"))
            if ms is not None:
                s["ms"] = _r(ms, 1)
        out.append(s)
    return out


def _leg(d, frac_from="roofline", **more):
    """{value, ms_per_step, frac} of one config object of the full record (None when the leg was skipped; its error when it failed)."""
    if not isinstance(d, dict):
        return None
    if "error" in d and "value" not in d:
        return {"error": str(d["error"])[:80]}
    r = d.get(frac_from) or {}
    out = {"value": _r(d.get("value"), 2), "ms_per_step": _r(d.get("ms_per_step"), 1)}
    if isinstance(r, dict) and r.get("frac") is not None:
        out["frac"] = _r(r["frac"])
    out.update({k: v for k, v in more.items() if v is not None})
    return out


def compact_line(full, full_path=None, limit=COMPACT_LIMIT):
    """The ONE line the driver parses: bench.py's LAST stdout line, <= `limit` bytes. Everything the contract names (metric, value,
    unit, n_gpus, steps, warmup, ms_per_step, higher_is_better, scaling, vs_baseline, dtype, data, config, roofline, cpu_baseline) in
    full; every other kernel fraction of the run as short `roofline.also` entries {k, w, frac[, issued], us | ms}; the other BASELINE
    configs as `configs{...: {value, ms_per_step, frac}}`; the opt-in split-precision decodes as `alt`. The long form (`full`) goes to
    --full-json and stderr. If the record ever outgrows the limit the tail of `also`, then `configs` / `alt` detail, are dropped —
    never the contract keys."""
    g = full.get
    roof = dict(g("roofline") or {})
    also = _short_also(roof.pop("also", None))
    vs64 = roof.pop("vs_fp64", None) or {}
    roof_c = {k: roof.get(k) for k in ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "flops_per_launch", "avg_launch_us", "launches")}
    roof_c["kernel"] = str(roof_c["kernel"] or "").split(" (")[0]
    if roof.get("traffic_source"):
        roof_c["traffic_src"] = str(roof["traffic_source"]).split(":")[0].split(" (")[0] + " (separate --pmc passes)"
    if vs64:
        roof_c["logit_err_vs_fp64"] = float("%.3g" % vs64.get("vs_fp64_logit_err", 0.0))
    roof_c["also"] = also
    line = {k: g(k) for k in ("metric", "value", "unit", "n_gpus", "ranks_seen", "backend", "steps", "warmup", "ms_per_step",
                              "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "x0_sha1", "config")}
    line["roofline"] = roof_c
    if g("e2e_fp32_frac") is not None:
        line["e2e_fp32_frac"] = g("e2e_fp32_frac")
    if g("own_kernels_ms_per_decode"):
        line["kernels_ms"] = {k: _r(v, 1) for k, v in g("own_kernels_ms_per_decode").items() if v}
    c1, c3, c4 = g("config1_b4") or {}, g("config3_pm"), g("config4_enformer")
    dps = g("config5_dps")
    configs = {
        "c1_b4": _leg(c1.get("backbone_on_4_workgroups_per_sequence")),
        "c3_pm": _leg(c3, f16x3=_r((((c3 or {}).get("alt_precision") or {}).get("f16x3") or {}).get("value"), 1)),
        "c4_f32": _leg((c4 or {}).get("f32") if isinstance(c4, dict) and "error" not in c4 else c4, "roofline_trunk_gemm"),
        "c4_bf16x3": _leg(c4, "roofline_trunk_gemm"),
        "c5_tds_shard": _leg(g("config5_tds_shard")), "c5_tds_pop": _leg(g("config5_tds_population")),
        "c5_dps": _leg(dps, attributed=_r((dps or {}).get("attributed_frac"), 3) if isinstance(dps, dict) else None),
        "replay_rng": _leg((g("replay_rng") or {}).get("device")),
    }
    if g("config5_error"):
        configs["c5_error"] = str(g("config5_error"))[:80]
    line["configs"] = {k: v for k, v in configs.items() if v is not None}
    alt = {}
    for mode, leg in (g("alt_precision") or {}).items():
        alt[mode] = {"value": _r(leg.get("value"), 1), "ms_per_step": _r(leg.get("ms_per_step"), 1), "rows_vs_f32": leg.get("x0_rows_identical_vs_f32"),
                     "x0_sha1": leg.get("x0_sha1")}
        if leg.get("vs_fp64_logit_err") is not None:
            alt[mode]["logit_err_vs_fp64"] = float("%.3g" % leg["vs_fp64_logit_err"])
            alt[mode]["sel_agree_fp64"] = leg.get("selection_agreement_with_fp64")
    if alt:
        line["alt"] = alt
    if g("per_rank"):
        line["per_rank"] = {k: v for k, v in g("per_rank").items() if k != "note"}
    cb = g("cpu_baseline")
    if isinstance(cb, dict):
        line["cpu_baseline"] = {k: cb.get(k) for k in ("value", "unit", "cores", "cpu_model", "cores_total", "kind", "passes",
                                                       "s_per_step", "sweep_predicted_s_per_step") if cb.get(k) is not None}
        sw = (cb.get("thread_sweep") or {}).get("s_per_step_of_the_nets_by_threads")
        if sw:
            line["cpu_baseline"]["sweep_s"] = sw
        line["cpu_baseline"]["sample"] = str(cb.get("sample_short") or cb.get("sample") or "")[:160]
    else:
        line["cpu_baseline"] = None
    c1b = g("cpu_baseline_c1")
    if isinstance(c1b, dict):
        line["cpu_baseline_c1"] = {k: c1b.get(k) for k in ("value", "cores", "passes")}
    if g("leg_seconds"):
        line["wall_s"] = round(sum(g("leg_seconds").values()), 1)
    if full_path:
        line["full_json"] = full_path
    # never over the limit: shed detail from the least important end
    enc = lambda: json.dumps(line, separators=(",", ":"))                                  # noqa: E731
    while len(enc()) > limit and line["roofline"]["also"]:
        line["roofline"]["also"].pop()
        line["roofline"]["also_truncated"] = True
    for key in ("kernels_ms", "per_rank", "alt", "configs"):
        if len(enc()) > limit:
            line.pop(key, None)
    assert len(enc()) <= limit, len(enc())
    return enc()


def emit(full, full_path):
    """Long form -> `full_path` (+ stderr), compact line -> stdout, LAST."""
    written = None
    if full_path:
        try:
            with open(full_path, "w") as f:
                json.dump(full, f, indent=1)
            written = os.path.relpath(full_path, ROOT) if os.path.abspath(full_path).startswith(ROOT) else full_path
        except OSError as e:
            print(f"bench.py: could not write {full_path}: {e}", file=sys.stderr)
    sys.stderr.write("BENCH_FULL " + json.dumps(full) + "\n")
    sys.stderr.flush()
    sys.stdout.flush()
    print(compact_line(full, written), flush=True)


def _gpu_count_without_hip():
    """GPUs this process may use, counted WITHOUT a HIP / HSA call (torch.cuda.device_count() can fall through to
    hipGetDeviceCount, which initialises the runtime in this — the launching — process): the visibility variables if set,
    else the KFD topology in sysfs (a node with simd_count > 0 is a GPU)."""
    for var in ("HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        v = os.environ.get(var)
        if v is not None:
            return len([x for x in v.split(",") if x.strip() != ""])
    n, root = 0, "/sys/class/kfd/kfd/topology/nodes"
    try:
        for node in os.listdir(root):
            with open(os.path.join(root, node, "properties")) as f:
                props = dict(ln.split()[:2] for ln in f if len(ln.split()) >= 2)
            n += int(props.get("simd_count", "0")) > 0
    except OSError:
        return 0
    return n


def self_launch(n):
    """`python bench.py --gpus N` from a bare shell: start the N ranks as a child `torch.distributed.run` (one process per
    GPU, rendezvous on 127.0.0.1) and return its exit code. This process never touches the GPU (devices are counted from sysfs / the visibility variables, not through HIP), and
    nothing is exec'd: the launcher runs as a child whose exit code is returned."""
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "8")
    if "--dry-run" not in sys.argv and _gpu_count_without_hip() < n:
        # fewer GPUs than ranks: the ranks share devices, which RCCL refuses — host-side collectives, labelled in the line
        env.setdefault("SVDD_DIST_BACKEND", "gloo")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    # the child's stdout is filtered: rank 0's JSON line goes to stdout, anything else (gloo's connection banner, ...) to stderr
    proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, text=True, bufsize=1)
    for ln in proc.stdout:
        (sys.stdout if ln.lstrip().startswith("{") else sys.stderr).write(ln)
    sys.stdout.flush()
    return proc.wait()


def dry_run(args):
    """The N-rank skeleton of the bench without the GPU: rendezvous (gloo), barrier-bracketed timing with the MAX over
    ranks, weak-scaling row ownership (rank r owns global rows r*B .. r*B + B - 1) and the one all-gather of the decoded
    tokens, with a stand-in "decode" that is a pure function of the global row (what Philox keying gives the real one).
    Verifies the gathered batch on every rank. No throughput is reported."""
    import torch.distributed as dist
    from svdd_amd import distributed
    rank, world, _ = distributed.init_from_env("gloo")
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    B, L = args.batch, args.length
    rows = lambda lo, n: ((torch.arange(lo, lo + n)[:, None] * 7 + torch.arange(L)[None, :]) % 4).to(torch.uint8)   # noqa: E731
    rank_times = []

    def one():
        t_a = time.perf_counter()
        x0 = rows(rank * B, B)
        t_b = time.perf_counter()
        out = distributed.gather_tokens(x0, B * world)
        rank_times.append((t_b - t_a, time.perf_counter() - t_b))
        return out
    for _ in range(args.warmup):
        one()
    if world > 1:
        dist.barrier()
    rank_times.clear()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = one()
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    assert torch.equal(out, rows(0, B * world)), f"rank {rank}: gathered batch differs"
    per_rank = None
    if world > 1:
        tmax = torch.tensor([elapsed], dtype=torch.float64)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        elapsed = float(tmax.item())
        mine = torch.tensor([sum(t[0] for t in rank_times) / len(rank_times), sum(t[1] for t in rank_times) / len(rank_times)],
                            dtype=torch.float64)
        allr = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(allr, mine)
        per_rank = {"decode_ms": [round(float(t[0]) * 1e3, 3) for t in allr],
                    "allgather_ms": [round(float(t[1]) * 1e3, 3) for t in allr]}
    if rank == 0:
        print(json.dumps({"metric": "decoded sequences/sec (whole node), L=200 M=10 128-step SVDD-MC", "value": None,
                          "unit": "sequences/s", "dry_run": True, "n_gpus": world,
                          "ranks_seen": dist.get_world_size() if world > 1 else 1,
                          "backend": dist.get_backend() if world > 1 else None, "steps": args.steps, "warmup": args.warmup,
                          "ms_per_step": round(elapsed / args.steps * 1e3, 3), "scaling": "weak",
                          "config": {"workload": "stand-in decode on the host (launch / rendezvous / all-gather check only)",
                                     "global_batch": B * world, "sharding": f"rows x{world}, 1 all-gather"},
                          "gathered_rows_verified": B * world, "per_rank": per_rank}))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def headline(args, world, elapsed, out):
    """The keys every line carries, plain or --full: `elapsed` = wall seconds of the args.steps timed decodes (max over ranks),
    `out` = the gathered tokens of the last one."""
    import torch.distributed as dist
    B, L, M, S = args.batch, args.length, args.sample_M, args.diffusion_steps
    workload = (f"DNA enhancer SVDD-MC, batch={B}/GPU, L={L}, M={M}, {S} steps "
                f"(BASELINE.json configs[1]); dilated-CNN backbone 3.3M params + ConvGRU value net")
    if args.value_net != "convgru":
        workload += " [value net: Enformer-shaped trunk, 230M params — BASELINE configs[3] shape]"
    return {
        "metric": "decoded sequences/sec (whole node), L=200 M=10 128-step SVDD-MC",
        "value": round(B * world * args.steps / elapsed, 3), "unit": "sequences/s", "n_gpus": world,
        "ranks_seen": dist.get_world_size() if world > 1 else 1,
        "backend": ({"nccl": "nccl (RCCL)"}.get(dist.get_backend(), dist.get_backend()) if world > 1 else None),
        "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 3),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32",
        "data": "synthetic (random-init nets, all-MASK prior)",
        "x0_sha1": _digest(out),       # of the gathered batch of the last timed decode: equal for any number of ranks (Philox is keyed by the global row)
        "config": {"workload": workload, "global_batch": B * world, "rng": args.rng, "sharding": f"rows x{world}, 1 all-gather"},
    }


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--cpu-sweep-only":          # child of cpu_baseline: never touches the GPU
        B, L, M, S, seed = (int(v) for v in sys.argv[2:7])
        print(json.dumps(cpu_thread_sweep(B, L, M, S, seed)))
        return
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=256, help="rows per GPU")
    ap.add_argument("--length", type=int, default=200)
    ap.add_argument("--sample-M", type=int, default=10)
    ap.add_argument("--diffusion-steps", type=int, default=128)
    ap.add_argument("--cpu-steps", type=int, default=6, help="diffusion steps timed for cpu_baseline (0 = skip)")
    ap.add_argument("--rng", default="philox", choices=["philox", "replay"])
    ap.add_argument("--alt-precision", default="f16x3,bf16x3,bf16",
                    help="comma list of split-precision modes measured AFTER the fp32 headline ('' = none)")
    ap.add_argument("--alt-steps", type=int, default=2, help="timed decodes per alt-precision mode")
    ap.add_argument("--value-net", default="convgru", choices=["convgru", "enformer"],
                    help="enformer: the 230M-parameter Enformer-shaped value trunk of BASELINE config 4 (not the headline config)")
    ap.add_argument("--c4-steps", type=int, default=1, help="decodes timed for the config4_enformer object of the default line (0 = skip)")
    ap.add_argument("--c3-steps", type=int, default=1, help="decodes timed for the config3_pm object (BASELINE configs[2], SVDD-PM; 0 = skip)")
    ap.add_argument("--c5-steps", type=int, default=1, help="decodes timed for the config5 objects (BASELINE configs[4], TDS / DPS; 0 = skip)")
    ap.add_argument("--extra-legs", type=int, default=1,
                    help="0: skip the legs that launch the headline's kernels under other conditions (replay_rng: the backbone with the "
                         "mt19937 workgroup beside it; config1_b4: 4-sequence launches) — used for the rocprofv3 --stats pass, whose "
                         "per-kernel averages should be the headline workload's")
    ap.add_argument("--c4-f32-steps", type=int, default=1, help="decodes of the config-4 shard timed at fp32 (the reference's precision) inside config4_enformer (0 = skip)")
    ap.add_argument("--cpu-passes", type=int, default=3, help="cpu_baseline passes; the median is reported (BASELINE.md section 2)")
    ap.add_argument("--full-json", default=os.path.join(ROOT, "bench_full.json"),
                    help="where the LONG record goes (every object of the run with its prose); stdout's last line is the compact record (<= 6 KB) the driver parses; '' = stderr only")
    ap.add_argument("--dry-run", action="store_true",
                    help="launch / rendezvous / all-gather skeleton with a stand-in decode on the host (no GPU, gloo)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, every other leg (rooflines, alt precisions, other configs, CPU baselines) and the compact "
                         "record; without it the line carries the headline only and no per-dispatch events are taken")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the decoded tokens of the last timed decode to DIR/x0.npy (float32)")
    args = ap.parse_args()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args.gpus))
    if args.steps < 1 or args.warmup < 0:        # checked in the ranks: a failing rank must fail the launcher's command
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.dry_run:
        return dry_run(args)

    from svdd_amd import _lib, distributed, synthetic
    from svdd_amd.backbone import CNNModel
    from svdd_amd.value_nets import ConvGRUTrunk
    import torch.distributed as dist

    legs = _Legs()
    rank, world, local = distributed.init_from_env()
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    local = local % max(torch.cuda.device_count(), 1)        # (dry runs with more ranks than GPUs share devices)
    torch.cuda.set_device(local)
    dev = f"cuda:{local}"
    nccl = world > 1 and dist.get_backend() == "nccl"
    barrier = (lambda: dist.barrier(device_ids=[local])) if nccl else (lambda: dist.barrier())
    to_dist = (lambda t: t) if (world == 1 or nccl) else (lambda t: t.cpu())      # gloo dry run: collectives on host tensors
    B, L, M, S = args.batch, args.length, args.sample_M, args.diffusion_steps

    model, emb, head, _ = synthetic.build("dna" if L == 200 else "rna", dev, value=args.value_net)
    model.rng_mode, model.philox_seed, model.row_offset = args.rng, 0, rank * B
    # (An opaque value net could also skip the copies of the parent — Diffusion.skip_generic — but every new live-batch
    #  size makes MIOpen pick / build kernels for that size; with the 1536-channel Enformer-shaped trunk that cost more than
    #  the skipped work in a 25-minute trial. Left off.)

    if world > 1:                  # communicator set-up (seconds with RCCL) never lands in the timed region, even with --warmup 0
        dist.all_reduce(to_dist(torch.zeros(1, device=dev)))
        barrier()

    rank_times = []                # (decode s, all-gather s) of every timed decode of this rank

    if args.rng == "replay" and world > 1:
        # parity mode over ranks: every rank replays the WHOLE batch's mt19937 stream and K1 reads its rows
        model._shard = (rank * B, (rank + 1) * B, B * world, world)

    def one_decode():
        if args.rng == "replay":
            torch.manual_seed(0)               # every rank (and every decode) from the same generator state, like the reference's process
        t_a = time.perf_counter()
        x0 = model.controlled_sample(emb, head, num_steps=S, eval_sp_size=B, sample_M=M)
        if world > 1:
            torch.cuda.synchronize()
        t_b = time.perf_counter()
        out = distributed.gather_tokens(x0, B * world)
        if world > 1:
            torch.cuda.synchronize()
            rank_times.append((t_b - t_a, time.perf_counter() - t_b))
        return out

    def fence():
        if world > 1:
            barrier()
        torch.cuda.synchronize()

    legs.mark("setup")
    for _ in range(args.warmup):
        one_decode()
    fence()
    rank_times.clear()
    legs.mark("warmup")
    t0 = time.perf_counter()
    for k in range(args.steps):
        if args.full and k == args.steps - 1:
            _lib.profile_enable(True)      # per-dispatch HIP events on the LAST timed decode (a few us of host time per launch)
        out = one_decode()
    fence()
    elapsed = time.perf_counter() - t0
    legs.mark("headline")
    _lib.profile_enable(False)
    assert out.shape == (B * world, L) and int(out.max()) <= 3
    per_rank = None
    if world > 1:
        tmax = to_dist(torch.tensor([elapsed], device=dev, dtype=torch.float64))
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        elapsed = float(tmax.item())
        mine = to_dist(torch.tensor([sum(t[0] for t in rank_times) / len(rank_times), sum(t[1] for t in rank_times) / len(rank_times)],
                                    device=dev, dtype=torch.float64))
        allr = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(allr, mine)
        per_rank = {"decode_ms": [round(float(t[0]) * 1e3, 2) for t in allr],
                    "allgather_ms": [round(float(t[1]) * 1e3, 3) for t in allr],
                    "note": "mean over the timed decodes; the all-gather time of a rank includes its wait for the slowest rank"}
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, out)
    if not args.full:
        if rank == 0:
            line = headline(args, world, elapsed, out)
            if per_rank:
                line["per_rank"] = per_rank
            print(json.dumps(line, separators=(",", ":")), flush=True)
        if world > 1:
            barrier()
            dist.destroy_process_group()
        return
    k1_total_ms, k1_launches = _lib.profile_collect(0)
    k2_total_ms, k2_launches = _lib.profile_collect(1)
    conv_total_ms, conv_launches = _lib.profile_collect(2)
    gru_total_ms, gru_launches = _lib.profile_collect(3)
    epi_total_ms, epi_launches = _lib.profile_collect(4)
    tower_total_ms, tower_launches = _lib.profile_collect(5)
    bb_total_ms, bb_launches = _lib.profile_collect(6)
    tail_total_ms, tail_launches = _lib.profile_collect(7)

    # ---- the same workload with the nets on the 16-bit matrix cores (never the headline)
    H = 128
    conv_flops_fwd = sum(2.0 * B * H * H * sum(max(0, L - abs(t - 4) * d) for t in range(9))
                         for d in (1, 1, 4, 16, 64) for _ in range(4))
    bb_flops = conv_flops_fwd + 2.0 * B * L * (5 * H * 9 + H * H + H * 5)
    alt = {}
    pmc_lp, pmc_lp_src = {}, None                # HBM bytes per backbone_lp_kernel launch, from separate --pmc passes
    for name in ("r06_pmc.json", "r05_pmc.json", "r04_pmc.json", "r03_pmc.json"):
        pth = os.path.join(ROOT, "profiles", name)
        if pmc_lp:
            break
        if os.path.exists(pth) and (B, L, M) == (256, 200, 10):
            pmc_lp = json.load(open(pth)).get("backbone_lp_traffic_bytes_per_launch", {})
            pmc_lp_src = f"profiles/{name} (separate rocprofv3 --pmc passes, not measured in this run)"
    modes = [m for m in args.alt_precision.split(",") if m]
    # (value net = the Enformer-shaped trunk: every split-precision mode runs it on the hand-written kernels of
    #  csrc/svdd_trunk.hip — the x3 modes as bf16x3, the one-pass modes as bf16; the fp32 line above is the PyTorch module)
    for mode in modes:
        model.precision = mode
        one_decode()
        fence()
        t1 = time.perf_counter()
        for k in range(args.alt_steps):
            if k == args.alt_steps - 1:
                _lib.profile_enable(True)
            out_alt = one_decode()
        fence()
        el = time.perf_counter() - t1
        _lib.profile_enable(False)
        prof = {k: _lib.profile_collect(k) for k in (0, 1, 3, 5, 6, 7)}
        if world > 1:
            tm = to_dist(torch.tensor([el], device=dev, dtype=torch.float64))
            dist.all_reduce(tm, op=dist.ReduceOp.MAX)
            el = float(tm.item())
        bb_ms_lp = prof[6][0] / max(prof[6][1], 1)
        passes = 3 if mode.endswith("x3") else 1
        tf = bb_flops / (bb_ms_lp * 1e-3) / 1e12 if prof[6][1] else 0.0
        alt[mode] = {
            "value": round(B * world * args.alt_steps / el, 3), "unit": "sequences/s", "ms_per_step": round(el / args.alt_steps * 1e3, 3),
            "steps": args.alt_steps, "dtype": mode, "x0_sha1": _digest(out_alt),
            "x0_rows_identical_vs_f32": round(float((out_alt == out).all(dim=1).float().mean()), 5),
            "arithmetic": ("fp32 operands split hi+lo in %s, a*b = ahi*bhi + ahi*blo + alo*bhi on the 16-bit MFMA, fp32 accumulate; %s"
                           % (mode[:-2], "22-bit operand: fp32-class" if mode == "f16x3" else "16-bit operand: 1e-5-class, NOT fp32-class"))
                          if passes == 3 else "operands rounded to %s, one MFMA pass, fp32 accumulate" % mode,
            "roofline": {"bound": "mfma", "kernel": "backbone_lp_kernel (svdd_backbone_cnn_lp, one launch per forward)",
                         "achieved": round(tf, 2), "peak": LP_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": round(tf / LP_PEAK_TFLOPS, 5),
                         "flops_per_launch": round(bb_flops), "mfma_passes": passes,
                         "issued_frac": round(tf * passes / LP_PEAK_TFLOPS, 5), "avg_launch_us": round(bb_ms_lp * 1e3, 3),
                         "launches": prof[6][1], "traffic": pmc_lp.get(mode), "traffic_source": pmc_lp_src if pmc_lp.get(mode) else None},
            "own_kernels_ms_per_decode": {"backbone_cnn": round(prof[6][0], 2), "conv_tower": round(prof[5][0], 2),
                                          "gru": round(prof[3][0], 2), "value_tail": round(prof[7][0], 2),
                                          "propose": round(prof[0][0], 3), "select": round(prof[1][0], 3)},
        }
    model.precision = "f32"
    legs.mark("alt_precision")

    if rank == 0:
        k1_ms = k1_total_ms / max(k1_launches, 1)
        k1_bytes = B * L * (21 + 17 * M)
        traffic = None
        achieved = k1_bytes / (k1_ms * 1e-3) / 1e9
        seqs = B * world * args.steps
        flops_seq = (CNNModel.flops_per_position() * L * (S + 1) + ConvGRUTrunk.flops_per_position() * L * S * M)
        # useful FLOPs of the 20 dilated 128->128 x 9-tap convs of one backbone forward (dnaconv.py:151-156)
        conv_ms = conv_total_ms / max(conv_launches, 1)
        conv_tf = (conv_flops_fwd / 20.0) / (conv_ms * 1e-3) / 1e12 if conv_launches else 0.0
        pmc, pmc_src = {}, None
        for name in ("r06_pmc.json", "r05_pmc.json", "r04_pmc.json", "r03_pmc.json", "r02_pmc.json", "r01_pmc.json"):   # separate --pmc passes of this workload, see the file
            pmc_path = os.path.join(ROOT, "profiles", name)
            if os.path.exists(pmc_path) and (B, L, M) == (256, 200, 10):
                pmc = json.load(open(pmc_path))
                pmc_src = (f"profiles/{name}: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this workload collected "
                           "separately (tools/collect_round_profile.sh), not measured in this run")
                break
        if bb_launches:
            # the job's dominant kernel: the whole backbone forward in one launch. Algorithmic FLOPs per launch = the
            # multiply-adds of one forward that touch real data (taps that fall into the zero padding excluded):
            # 20 dilated convs + the 9-tap first conv on the one-hot + the two 1x1 convs.
            bb_ms = bb_total_ms / bb_launches
            bb_tf = bb_flops / (bb_ms * 1e-3) / 1e12
            roofline = {"bound": "mfma", "kernel": "backbone_kernel (svdd_backbone_cnn_f32: first conv + 20 x [LayerNorm, "
                                                   "dilated 9-tap conv 128->128, ReLU, residual] + 2 x 1x1 conv, one launch)",
                        "achieved": round(bb_tf, 2), "peak": FP32_PEAK_TFLOPS, "unit": "TFLOP/s",
                        "frac": round(bb_tf / FP32_PEAK_TFLOPS, 5), "traffic": pmc.get("backbone_traffic_bytes_per_launch"),
                        "traffic_source": pmc_src if pmc.get("backbone_traffic_bytes_per_launch") else None,
                        "flops_per_launch": round(bb_flops), "avg_launch_us": round(bb_ms * 1e3, 3), "launches": bb_launches}
        else:
            roofline = {"bound": "mfma", "kernel": "conv1d_cl_static_kernel<128,128,9,dil,200> (backbone dilated conv, "
                                                   "dil 1,1,4,16,64 x4 per forward)",
                        "achieved": round(conv_tf, 2), "peak": FP32_PEAK_TFLOPS, "unit": "TFLOP/s",
                        "frac": round(conv_tf / FP32_PEAK_TFLOPS, 5), "traffic": pmc.get("conv_traffic_bytes_per_launch"),
                        "traffic_source": pmc_src if pmc.get("conv_traffic_bytes_per_launch") else None,
                        "flops_per_launch": round(conv_flops_fwd / 20.0), "avg_launch_us": round(conv_ms * 1e3, 3),
                        "launches": conv_launches}
        line = headline(args, world, elapsed, out)
        line.update({
            "roofline": roofline,
            "roofline_sampler": {"bound": "hbm", "kernel": "propose_kernel (K1)", "achieved": round(achieved, 2),
                                 "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 5),
                                 "traffic": pmc.get("k1_traffic_bytes_per_launch", traffic),
                                 "traffic_source": pmc_src if pmc.get("k1_traffic_bytes_per_launch") else None,
                                 "bytes_per_launch": k1_bytes,
                                 "avg_launch_us": round(k1_ms * 1e3, 3), "launches": k1_launches,
                                 "select_kernel_avg_launch_us": round(k2_total_ms / max(k2_launches, 1) * 1e3, 3)},
            "own_kernels_ms_per_decode": {"backbone_cnn": round(bb_total_ms, 2), "conv_tower": round(tower_total_ms, 2),
                                          "value_tail": round(tail_total_ms, 2),
                                          "conv1d": round(conv_total_ms, 2), "gru": round(gru_total_ms, 2),
                                          "epilogue_ln": round(epi_total_ms, 2),
                                          "propose": round(k1_total_ms, 3), "select": round(k2_total_ms, 3)},
            "own_kernels_note": "summed per-dispatch durations of the last timed decode; in its late steps the second part's GRU / tail co-run with the "
                                "first part's tower on a side stream, so the sum can exceed the wall time those kernels take (roofline_value_net is kernel-exclusive)",
            # reference-equivalent FLOPs (every candidate through every net) per second over the fp32 peak:
            # a throughput normalisation, not a utilisation — exact work-skipping executes fewer FLOPs than that
            "e2e_fp32_frac": round(flops_seq * seqs / elapsed / 1e12 / (FP32_PEAK_TFLOPS * world), 5),
            "alt_precision": alt or None,
        })
        if per_rank:
            line["per_rank"] = per_rank
        if world == 1 and args.value_net == "convgru":
            line["roofline_sampler_saturated"] = sampler_saturated(dev, L=L, M=M)
            if pmc.get("k1_saturated_traffic_bytes_per_launch"):      # HBM bytes of THAT launch size, from the separate PMC passes
                line["roofline_sampler_saturated"]["traffic"] = pmc["k1_saturated_traffic_bytes_per_launch"]
                line["roofline_sampler_saturated"]["traffic_source"] = pmc_src
            # (the near-tied leg first: scores ~1e-7 apart are what the random-init value nets of this workload actually produce)
            line["roofline_select_saturated"] = [select_saturated(dev, L=L, M=M, near_uniform=True), select_saturated(dev, L=L, M=M),
                                                 select_saturated(dev, L=L, M=20)]
            legs.mark("saturated")
            if args.extra_legs in (1, 2):
                line["replay_rng"] = replay_leg(model, emb, head, B, L, M, S)
            if args.extra_legs in (1, 3):
                line["config1_b4"] = small_batch_leg(model, emb, head, L, S)
            legs.mark("replay_c1" if args.extra_legs else "saturated")
            line["roofline_tds_resample"] = tds_saturated(dev, L=L)
            line["roofline_value_net"] = value_net_roofline(model, emb, head, dev, B, L, M, S, tower_total_ms, tower_launches,
                                                            gru_total_ms, gru_launches)
            # the same two kernels of the split-precision decodes (tower_lp_kernel, gru_lp_kernel) against the 16-bit MFMA peak, on the
            # rows the fp32 decode of the same Philox stream executed (a split-precision decode selects differently on a handful
            # of steps; its counts differ by well under 1 %): issued = useful x MFMA passes
            ex = (line["roofline_value_net"] or {}).get("executed")
            for mode, leg in (alt or {}).items():
                if not ex or "own_kernels_ms_per_decode" not in leg:
                    continue
                passes = 3 if mode.endswith("x3") else 1
                rv = {}
                for key, kern, flops, ms in (("conv_tower", "tower_lp_kernel", ex["flops_per_tower_row"] * ex["tower_rows"], leg["own_kernels_ms_per_decode"]["conv_tower"]),
                                             ("gru", "gru_lp_kernel", ex["flops_per_gru_row"] * ex["gru_rows"], leg["own_kernels_ms_per_decode"]["gru"])):
                    tf = flops / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
                    rv[key] = {"bound": "mfma", "kernel": kern, "achieved": round(tf, 2), "peak": LP_PEAK_TFLOPS, "unit": "TFLOP/s",
                               "frac": round(tf / LP_PEAK_TFLOPS, 5), "issued_frac": round(tf * passes / LP_PEAK_TFLOPS, 5),
                               "executed_flops_per_decode": round(flops), "kernel_ms_per_decode": ms}
                leg["roofline_value_net"] = rv
        legs.mark("value_net_roofline")
        if args.value_net != "convgru":
            line["e2e_fp32_frac"] = None
            # (the headline line of this workload is fp32: the trunk runs on the fp32-plane kernels; the split modes are in alt_precision)
            line["roofline_trunk_gemm"] = trunk_gemm_roofline(model, emb, head, dev, int(0.75 * B * M), L, precision="f32")
            line["roofline_trunk_gemm_bf16x3"] = trunk_gemm_roofline(model, emb, head, dev, int(0.75 * B * M), L)
        if args.c4_steps > 0 and world == 1 and args.value_net == "convgru" and (B, L, M) == (256, 200, 10):
            line["config4_enformer"] = config4_leg(dev, args.c4_steps, f32_steps=args.c4_f32_steps)
            legs.mark("config4")
        if world == 1 and args.value_net == "convgru" and (B, L, M) == (256, 200, 10):
            if args.c3_steps > 0:
                line["config3_pm"] = config3_leg(dev, args.c3_steps, S=S)
                legs.mark("config3")
            if args.c5_steps > 0:
                c5 = config5_leg(dev, args.c5_steps, S=S)
                for k, v in c5.items():
                    line["config5_" + k] = v
                legs.mark("config5")
        line["roofline"]["also"] = roofline_also(line)
        if args.cpu_steps > 0 and world == 1 and args.value_net == "convgru":
            model.state_trace = []                                  # one extra (untimed) decode: the trajectory's states
            model.controlled_sample(emb, head, num_steps=S, eval_sp_size=B, sample_M=M)
            torch.cuda.synchronize()
            states = [x.cpu().numpy() for x in model.state_trace]
            if (B, L, M) == (256, 200, 10) and S == 128:
                ev = precision_evidence(model, emb, head, model.state_trace, model._schedule(S, 1e-5)[0], list((alt or {}).keys()), B, L, M)
                line["roofline"]["vs_fp64"] = ev.get("f32")           # the headline's own arithmetic against fp64, beside its roofline
                for mode in (alt or {}):
                    if mode in ev:
                        alt[mode].update(ev[mode])
                line["precision_evidence"] = ev
            model.state_trace = None
            legs.mark("precision_evidence")
            line["cpu_baseline"] = cpu_baseline(B, L, M, S, args.cpu_steps, states=states, passes=args.cpu_passes)
            legs.mark("cpu_baseline")
            line["cpu_baseline_c1"] = cpu_baseline_c1(passes=args.cpu_passes)
            legs.mark("cpu_baseline_c1")
        else:
            line["cpu_baseline"] = None
        line["leg_seconds"] = legs.secs
        emit(line, args.full_json)
    if world > 1:
        barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
