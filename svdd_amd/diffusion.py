"""`Diffusion` — host-side mirror of the reference sampler `diffusion_gosai.Diffusion` for the
decode hot path (reference diffusion_gosai.py:74-175, 286-377, 751-753, 820-1496).

Same method names, keyword arguments, return types and error behaviour as the reference for the
methods on the SVDD decode path, so `BaseModel`/`decode.py`-style callers work unchanged:

    forward, _process_sigma, _sample_prior, _sample, decode_sample, controlled_sample,
    controlled_sample_tweedie, controlled_sample_TDS, controlled_sample_DPS, controlled_sample_classfier,
    _ddpm_update_finetune[_controlled[_twedie|_TDS|_DPS]], _ddpm_update_finetune_classfier, compute_gradient,
    transform_samples, and the ELBO scoring of clean sequences: _sample_t, q_xt, _forward_pass_diffusion, _loss
    (plus sequence_nll / nll_metrics, the per-sequence API built on them)
and, without a reference method of their own (a loop of the reference's q_xt and per-step updates from a given state):
    decode_sample_from, controlled_sample_from (template-constrained design), renoise, refine (re-mask refinement)
and the data path that trains the value function (reference Enformer.py:163-267): _sample(cdq=True) and value_targets

What differs is where the work runs: everything between "backbone logits" and "next x_t" is one
or two launches of the hand-written HIP kernels (svdd_amd/csrc, C ABI include/svdd_hip.h) instead
of ~16*M+20 tiny tensor ops and B host syncs per step; the nets stay PyTorch-ROCm modules.
There is no CPU fallback: the sampler methods need a gfx950 GPU and raise otherwise.

Whatever the engine derives from a module's weights — the fused formulations of the nets, the GRU packs of the gradient paths, the
validity of the backbone's conv packs — is held in ONE WeightCache (`Diffusion._fused`): validated against the weights once per
outermost sampler call (`_decode_scope`), at every call outside one, and dropped by `clear_fused()`.

Engine knobs (attributes; defaults reproduce the reference's observable behaviour):
  rng_mode         "replay": the categorical uniforms are drawn from torch's global CPU mt19937
                   generator in exactly the order the reference's CPU path consumes them
                   (M x rand_like(q_xs), in q_xs' memory order) — token-exact parity. replay_rng = "device" (default):
                   the generator's 624-word state is uploaded once per sampler call, the stream is produced on the GPU by
                   svdd_mt19937_uniform_f32 a step ahead on a side stream, and the advanced state is written back into
                   torch's generator when the call returns; "host": torch.rand on the host + a 10 MB upload per step.
                   "philox": generated in-kernel from (seed, step, global row, m, l) — no host
                   traffic, identical results for any sharding of the batch over GPUs.
  value_batching   "batched": one value-net forward over all B*M candidates (default);
                   "reference": M forwards of batch B like diffusion_gosai.py:1207-1209.
  select_mode      "argmax" (reference, :1225) or "multinomial" (the commented-out :1223; philox only).
  fuse_nets        True: nets of known architecture (CNNModel backbone; ConvGRUTrunk+ConvHead value /
                   reward nets) are run through their MI355X formulations in svdd_amd/fused.py (same
                   weights, exact fp32: one-launch backbone kernel, conv-tower / GRU / value-tail kernels; in
                   SVDD-MC the conv tower is evaluated once per parent x_t and per candidate only around the
                   positions it changed — bit-identical, `FusedValueNet.share_parent_tower`).
                   False: call the modules as given.
  precision        "f32" (default): the fused nets compute in exact fp32 — the parity path and what bench.py's
                   headline measures. "f16x3" / "bf16x3": matrix products on the 16-bit matrix cores with operands
                   split hi + lo (3 MFMAs per product, fp32 accumulate) at ~2.5x the speed. ONLY f16x3 is fp32-class (a 22-bit
                   operand: logits 3e-6 from an fp64 forward, the fp32 kernels 4.5e-6); bf16x3 carries a 16-bit operand —
                   logits 4.5e-5 from fp64, ten times fp32's error, 1e-5-class. "f16" / "bf16": one 16-bit pass.
                   Tokens can differ from the fp32 decode at near-ties; tools/precision_agreement.py reports it.
  skip_unchanged   True (default): exact work-skipping. A candidate that unmasked nothing is a copy of
                   its parent x_t (:1203) and, time_conditioning being off (:334-335), every net output for it is the
                   parent's: SVDD-MC evaluates the value net only on the live candidates and takes a copy's score from
                   the parent (= the score of the candidate selected one step earlier); SVDD-PM runs the candidate
                   backbone forward, x0-hat and reward on the live candidates only and never re-runs the parent forward
                   (the selected candidate's logits ARE the next parent's). With logits_cache the backbone also skips
                   rows whose x_t did not change. Compaction is done on the device; no host round trip in the loop.
                   Decodes are bit-identical to skip_unchanged = False (tests/test_skip_gpu.py). Needs the fused nets.
  logits_cache     "auto" (default): SVDD-MC keeps a per-row logits cache when several sequences share a backbone tile
                   (L <= 104; at L = 200 one workgroup owns one sequence and skipping rows frees CUs but saves no
                   time); "on" / "off". (SVDD-PM always carries the selected candidate's logits forward.)
  incremental_backbone  "auto" (default): the SVDD-MC skipping loop at 104 < L <= 208 (one sequence per backbone tile, fp32, CNN backbone
                   with a leading run of dilation-1 layers, more than 128 rows) carries the residual stream behind those layers
                   across the steps and recomputes, per step, only the 16-row tiles a changed token can reach
                   (svdd_backbone_incr2_f32; the remaining layers run from the last carried plane). Same logits bit for bit
                   (tests/test_backbone_incremental_gpu.py). "on": wherever the kernels apply, whatever the batch; "off". Off under
                   graph capture. The first forward of such a decode fills the planes of all B rows: with dedup_prior it is one
                   broadcast of the all-MASK row's cached planes and logits (svdd_backbone_incr_seed_f32), else the whole forward.
  incremental_depth  how many conv layers the incremental backbone carries: an int from the leading run of dilation-1 layers (8)
                   up to the end of the dilation-4 run behind them (12; svdd_backbone_incr3_f32 — a change has reached +- 52 .. 100
                   rows there), or "auto" (default) = fused.INCR_DEPTH_AUTO, the depth the measurement of
                   profiles/deep_planes_depth.txt picked. The environment variable SVDD_INCR_DEPTH sets the value every new model
                   starts with (A/B runs). Same bits at every depth (tests/test_backbone_incr3_gpu.py).
  incremental_items  "tight" (default): the dilation-1 layers of the incremental backbone recompute 16-row tiles that start at the first
                   row a changed token reaches, with a 4-row halo, and the step's work list is built in one launch
                   (svdd_backbone_incr4_f32); "aligned": tiles at multiples of 16 (svdd_backbone_incr3_f32). The environment variable
                   SVDD_INCR_ITEMS sets the value every new model starts with (A/B runs). Same bits (tests/test_backbone_incr4_gpu.py).
  dedup_prior      True (default): every row of the prior x_T is the same all-MASK row (_sample_prior, :751-753), and with the hand-written
                   kernels a row's net output does not depend on the batch around it — so the FIRST backbone forward of a decode, the
                   parents' first value / reward score and their first tower pass run on one row and are broadcast. Bit-identical to
                   forwarding all B rows (tests/test_skip_gpu.py); one backbone launch of 129 and a value-net pass less per decode.
                   In the SVDD-MC skipping loop that one row's results are constants of the weights and are computed once, not once
                   per decode: the fused nets keep them (fused.PriorSeeds, dropped with the nets when the weights change) and a
                   decode broadcasts them (tests/test_prior_seed_gpu.py). False switches all of it off.
  dps_one_launch   True (default): the differentiable backbone pass of a DPS step (forward2 on one_hot(x_t) + its input gradient) is ONE
                   launch each way (fp32, CNN backbone, 104 < L <= 208): the forward is the inference kernel bit for bit, so its logits
                   also give q_xs and the reference's second, identical forward (:1306 vs :1324) is not run. False: the layer-wise
                   autograd path of round 3 (20 + 20 convolution launches and a pass per layer each way).
  dps_single_forward  (only where the one-launch pair does not apply) False (default): a DPS step runs the no-grad forward for q_xs AND the differentiable pass for the gradient,
                   like the reference (:1306 and :1324 evaluate one function twice). True (opt-in): the differentiable pass
                   (forward2) also supplies the log-probs of q_xs — equal to round-off (~1e-6), so zero guidance is no longer
                   bit-for-bit the un-guided decode at near-ties.
  cdq_draws        10 (the reference's hard-coded count, :846): next states _sample(cdq=True) draws per step.
  skip_stats       None, or a dict the samplers fill with device-side hit counters (live candidates, changed rows).
  skip_generic     False (default). True: SVDD-MC also skips the copies of the parent for an OPAQUE value function (any
                   nn.Module, e.g. the Enformer-shaped trunk): the live candidates are gathered into a smaller batch whose
                   size is read back once per step (one host sync, negligible next to a net that takes milliseconds).
                   Mathematically identical; bit-identical only if the module's kernels do not depend on the batch size
                   (vendor libraries pick — and sometimes build — kernels per size; with a large MIOpen-backed trunk the
                   first decode pays for every new live-batch size, rounded to 256 rows here), hence opt-in. The one-pass modes "bf16" / "f16" run an
                   opaque value / reward net under torch.autocast; the x3 modes leave it in fp32.
"""
import contextlib
import functools
import math
import os
import warnings
import weakref
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from . import noise_schedule, ops
from .backbone import CNNModel


@dataclass
class Loss:
    """The reference's loss record (diffusion_gosai.py:43-47), returned by Diffusion._loss."""
    loss: torch.Tensor
    nlls: torch.Tensor
    token_mask: torch.Tensor


@dataclass
class ValueTargets:
    """The training set of one value-function iteration (Diffusion.value_targets), rows step-major (row k B + b = state k of
    sequence b): states u8 [S, B, L], their one-hot f32 [S B, L, 4] (MASK rows zero) or None, the regression targets y f32 [S B],
    and the rollout's x_0 int64 [B, L] (= states[S - 1])."""
    states: torch.Tensor
    onehot: Optional[torch.Tensor]
    y: torch.Tensor
    x0: torch.Tensor


@dataclass
class LedidiResult:
    """What Diffusion.ledidi returns, per design b of B with S samples: the S hard samples of the iteration with the lowest total
    loss (x_best u8 [B, S, L]; the S copies of the start while best_iter == -1) and their scores (score_best f32 [B, S]), that
    iteration's total / output / input loss (f32 [B]) and index (best_iter i32 [B]), n_iter = the iterations the longest-running
    design executed, trace f32 [n_iter, B, 3] (total, output, input loss per iteration; NaN after a design stopped) or None; x0 u8
    [B, L] and score0 f32 [B]: the start sequences and their scores."""
    x_best: torch.Tensor
    score_best: torch.Tensor
    best_total: torch.Tensor
    best_output: torch.Tensor
    best_input: torch.Tensor
    best_iter: torch.Tensor
    n_iter: int
    trace: Optional[torch.Tensor]
    x0: torch.Tensor
    score0: torch.Tensor


def design_pick(result, target=None):
    """One sequence per design from a LedidiResult: the best of the design's S best-iteration samples by the design's own objective
    (the highest score, or with target — a float or [B] — the score closest to it), the lowest s among ties; a design whose
    objectives are all NaN gives s = 0. -> (tokens u8 [B, L], score f32 [B], edits int64 [B] = positions that differ from x0)."""
    sc = result.score_best
    B, S = sc.shape
    if target is None:
        key = sc
    else:
        t = torch.as_tensor(target, dtype=torch.float32, device=sc.device).reshape(-1)
        if t.numel() not in (1, B):
            raise ValueError(f"target must be a float or hold {B} values, got {t.numel()}")
        key = -(sc - t.expand(B)[:, None]) ** 2
    key = torch.where(key != key, torch.full_like(key, float("-inf")), key)
    best = key.max(dim=1, keepdim=True).values
    s_idx = torch.arange(S, device=sc.device).expand(B, S)
    s = torch.where(key == best, s_idx, torch.full_like(s_idx, S)).min(dim=1).values.clamp(max=S - 1)
    rows = torch.arange(B, device=sc.device)
    tokens = result.x_best[rows, s]
    return tokens, sc[rows, s], (tokens != result.x0).sum(dim=1)


def _capturing():
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


def weight_fingerprint(*modules, content=True):
    """Identity of the weights of `modules`: (storage address, in-place version counter, shape) of every parameter and
    buffer — changes when a tensor is replaced (load_state_dict with assign, .to()) or modified in place through autograd-
    visible ops (optimizer step, load_state_dict copy_) — plus, with `content`, a CONTENT checksum (1- and 2-norm of every
    floating tensor, two multi-tensor launches and one read-back): writes through `.data` do not bump `_version`
    (`p.data.copy_(...)` is how the reference swaps EMA weights around sampling, models/ema.py:62,87 with
    diffusion_gosai.py:1564-1574), and a cached re-packing of the weights must not survive them. -> (meta, content)."""
    meta, tensors = [], []
    for m in modules:
        for t in list(m.parameters()) + list(m.buffers()):
            meta.append((t.data_ptr(), t._version, tuple(t.shape)))
            if t.is_floating_point() and t.numel():
                tensors.append(t.detach())
    chk = None
    if content and tensors and not _capturing():
        by_dev = {}
        for t in tensors:
            by_dev.setdefault((t.device, t.dtype), []).append(t)
        parts = []
        for ts in by_dev.values():
            parts.append(torch.stack(torch._foreach_norm(ts, 1) + torch._foreach_norm(ts, 2)).double().cpu())
        chk = tuple(torch.cat(parts).tolist())
    return tuple(meta), chk


def _same_weights(a, b):
    """Fingerprints equal; a side without a content checksum (taken during graph capture) compares by meta only."""
    return a[0] == b[0] and (a[1] is None or b[1] is None or a[1] == b[1])


class WeightCache:
    """Whatever is derived from the weights of modules (a fused formulation, re-packed GRU weights, the validity of the backbone's
    conv packs) holds COPIES of them, so it is valid only for the very module objects it was built from (weak references: an id()
    can be recycled after garbage collection) with the very weights (weight_fingerprint, content checksum included). Inside one
    decode scope an entry is validated once; without a scope, at every call."""

    def __init__(self):
        self._entries = {}               # (kind, id(module), ...) -> (weak references, fingerprint, value, scope stamp)

    def __len__(self):
        return len(self._entries)

    def clear(self):
        self._entries.clear()

    def get(self, kind, modules, build, scope):
        """build()'s result for these very `modules` with these very weights. `scope`: the id of the running decode scope (an entry
        already stamped with it is returned without fingerprinting: this keeps the check off the per-step path) or None. A None
        from build() is cached like any other result."""
        key = (kind,) + tuple(id(m) for m in modules)
        ent = self._entries.get(key)
        alive = ent is not None and all(r() is m for r, m in zip(ent[0], modules))
        if alive and scope is not None and ent[3] == scope:
            return ent[2]
        fp = weight_fingerprint(*modules)
        if alive and _same_weights(ent[1], fp):
            value = ent[2]
        else:
            for k in [k for k, v in self._entries.items() if any(r() is None for r in v[0])]:
                del self._entries[k]                                # entries of collected modules
            value = build()
        self._entries[key] = (tuple(weakref.ref(m) for m in modules), fp, value, scope)
        return value


def _refuse_motif_reward(what, *nets):
    """The gradient-guided samplers and the attributions differentiate their net; a motifs.GuidedReward only has values."""
    from .motifs import GuidedReward
    if any(isinstance(n, GuidedReward) for n in nets):
        raise TypeError(f"{what}: a GuidedReward is not differentiable (its motif term has reward values, no gradient): decode with "
                        "controlled_sample_tweedie (SVDD-PM) or controlled_sample_TDS")


def _decode_scope(fn):
    """Marks one call of a public sampler method: the fused-net caches are validated against the modules' weights once
    per outermost call (a decode), not at every diffusion step."""
    @functools.wraps(fn)
    def wrapped(self, *a, **k):
        if self._scope_depth == 0:
            self._scope_id += 1
        self._scope_depth += 1
        ok = False
        try:
            out = fn(self, *a, **k)
            ok = True
        finally:
            self._scope_depth -= 1
            if self._scope_depth == 0 and self._replay_stream is not None:
                st, self._replay_stream = self._replay_stream, None
                st.close()                 # the advanced mt19937 state goes back into torch's global CPU generator
        if ok and self._scope_depth == 0 and not _capturing():
            from .fused import check_backbone_split
            check_backbone_split()         # a small-batch backbone launch whose workgroups could not all be resident: raise, never return its tokens
        return out
    return wrapped


class Diffusion(nn.Module):
    replays_global_stream = True     # distributed.sharded_sample: replay mode shards by replaying the whole batch's stream per rank

    def __init__(self, config, backbone=None):
        super().__init__()
        self.config = config
        self.vocab_size = 4                                   # diffusion_gosai.py:85
        self.sampler = config.sampling.predictor
        self.mask_index = self.vocab_size                     # :94
        self.vocab_size += 1                                  # :95
        self.parameterization = config.parameterization
        if backbone is not None:
            self.backbone = backbone
        elif config.backbone == "cnn":
            self.backbone = CNNModel(config.model, alphabet_size=self.vocab_size, num_cls=3)   # :100-101
        elif config.backbone == "dit":
            # dead in the reference snapshot (models/__init__.py:1, needs CUDA-only flash_attn); here via ROCm SDPA
            from .dit import DIT
            self.backbone = DIT(config.model, vocab_size=self.vocab_size)                      # :102-104
        else:
            raise ValueError(f"Unknown backbone: {config.backbone}")
        if self.parameterization != "subs":
            raise ValueError("only the `subs` parameterization is on the reference's decode path "
                             "(configs_gosai/config_gosai.yaml:13)")
        self.T = config.T
        self.subs_masking = config.subs_masking
        self.noise = noise_schedule.get_noise(config)
        self.time_conditioning = config.time_conditioning
        self.neg_infinity = -1000000.0
        self.sampling_eps = config.training.sampling_eps
        # engine knobs
        self.rng_mode = "replay"
        self.value_batching = "batched"
        self.select_mode = "argmax"
        self.philox_seed = 0
        self.row_offset = 0
        self._shard = None               # (lo, hi, total, world) while distributed.sharded_sample runs this model
        self.fuse_nets = True
        self.precision = "f32"
        self.skip_unchanged = True
        self.late_steps_from = os.environ.get("SVDD_LATE_STEPS_FROM") or "auto"   # (the environment variable: A/B runs)
                                         # when FusedValueNet may run the live candidates as two parts (split_gru_rounds): "auto" = on every
                                         # step, as one fixed launch sequence whose parts the DEVICE sizes from the step's live counts
                                         # (svdd_value_late_step_f32; nothing is read back); a number = the host-decided side-stream form
                                         # from that fraction of the steps on (rounds 4-5: 0.8, tuned to the random-init benchmark; A/B)
        self.dedup_prior = True          # the prior's rows are identical (all MASK): its net evaluations run on ONE row (exact; see _prior_logits)
        self.seed_prior = os.environ.get("SVDD_SEED_PRIOR", "1") != "0"   # SVDD-MC skipping loop with dedup_prior: the all-MASK row's results (carried
                                         # planes, logits, tower output, score) come from the fused nets' per-weights cache and a decode
                                         # broadcasts them; False (A/B; the environment variable sets what a new model starts with):
                                         # the row is evaluated once per decode and the first stem forward runs on all B rows
        self.dps_fused = True            # DPS: the whole step on hand-written kernels, no autograd (_dps_fused_nets); False: round 5's autograd path between the same big kernels
        self.dps_one_launch = True       # DPS: the differentiable backbone pass as one launch each way (svdd_backbone_cnn_save_f32 / _grad_f32) where it applies
        self._dps_hard_onehot, self._dps_raw_logits, self._dps_logp = False, None, None
        self.dps_single_forward = False  # DPS opt-in: q_xs from the differentiable pass's log-probs, not from a second backbone forward per step
        self.logits_cache = "auto"
        self.incremental_backbone = "auto"
        self.incremental_depth = os.environ.get("SVDD_INCR_DEPTH") or "auto"   # carried layers of the incremental backbone (see the module docstring)
        self.incremental_items = os.environ.get("SVDD_INCR_ITEMS") or "tight"  # "tight" / "aligned" tiles in its dilation-1 layers
        self.skip_stats = None
        self.skip_generic = False
        self.trace = None          # set to a list to record (logits, scores) of every step (tests / smoke)
        self.state_trace = None    # set to a list to record x_t (uint8 clone) at the start of every step + the final x
        self._sched_cache = {}
        self._fused = WeightCache()      # everything derived from weights: fused nets, GRU packs, conv-pack validity (clear_fused drops it)
        self._scope_depth, self._scope_id = 0, 0
        self.fuse_trunk_f32 = True       # precision "f32" + Enformer-shaped value trunk: the hand-written fp32 trunk kernels (False: the PyTorch modules)
        self.replay_rng = "device"       # rng_mode "replay": "device" = torch's CPU mt19937 stream continued by K8 on the GPU for
        self._replay_stream = None       # the span of a sampler call; "host" = torch.rand on the host + upload (round 1-3)
        self._replay_checked = None      # scope id of the sharded replay decode whose generator state was compared across ranks
        self._classifier_fused_last = None   # classifier guidance: whether the last step's gradient ran on the fused kernels (no autograd)
        self.elbo_trace = None           # set to a list to record (t, sigma, dsigma, move_chance, w, xt) of every _forward_pass_diffusion
        self._from_state = False         # set by _decode_start: the running decode starts from a caller's state, not from the all-MASK prior
        self.cdq_draws = 10              # _sample(cdq=True): next states drawn per step (the reference's `for j in range(10)`, :846)
        self._step_base = 0              # added to the step index in every Philox key: refine() gives each round its own range of keys

    # ------------------------------------------------------------------ plumbing ----
    @property
    def device(self):
        return next(self.parameters()).device

    def _require_gpu(self):
        if self.device.type != "cuda":
            raise ops.SvddError("the SVDD sampler runs on the GPU only (move the model with .cuda()); "
                                "there is no CPU fallback for the hot path")

    def _schedule(self, num_steps, eps, t_start=1.0):
        key = (num_steps, eps, float(t_start))
        if key not in self._sched_cache:
            tab, timesteps, dt = noise_schedule.move_chance_table(self.noise, num_steps, eps, float(t_start))
            self._sched_cache[key] = (tab.numpy().copy(), timesteps, dt)
        return self._sched_cache[key]

    def _tokens_u8(self, x):
        return x if x.dtype == torch.uint8 else x.to(torch.uint8)

    def clear_fused(self):
        """Drop everything cached from weights (the fused formulations, the GRU packs of the gradient paths, the validity of the
        backbone's conv packs) and the backbone's cached zero-sigma time biases. Every cache entry carries a fingerprint of the
        weights it was built from (tensor identity, in-place version AND a content checksum, so `.data` / EMA swaps are caught
        too) and is rebuilt at the next decode when that no longer matches; call this to force it, or after changing weights
        in the middle of a per-step loop inside one sampler call."""
        self._fused.clear()
        if isinstance(self.backbone, CNNModel):
            self.backbone.clear_time_bias_cache()
            self.backbone._cpk_key = None

    @property
    def _scope(self):
        """Id of the running decode scope (_decode_scope) for WeightCache.get, None outside one."""
        return self._scope_id if self._scope_depth > 0 else None

    def _validate_conv_packs(self):
        """The packed dilated-conv weights of CNNModel._trunk_cl (DPS gradient path) are keyed by tensor identity + version
        inside the backbone; a `.data` / EMA swap changes neither. Validated like the fused nets: a changed fingerprint (or a
        cleared cache) makes the backbone re-pack."""
        bb = self.backbone
        self._fused.get("conv_packs", (bb.convs,), lambda: setattr(bb, "_cpk_key", None), self._scope)

    def _fused_backbone(self):
        def build():
            from .fused import FusedBackbone
            self.backbone.clear_time_bias_cache()
            return FusedBackbone(self.backbone).to(self.device).eval()
        fb = self._fused.get("backbone", (self.backbone,), build, self._scope)
        fb.precision = self.precision
        return fb

    def value_callable(self, embedding, head):
        """The callable the engine uses for `head(embedding(onehot))`: onehot fp32 [n,L,4] -> [n,1,1]."""
        from .enformer_value import EnformerTrunk
        from .value_nets import ConvGRUTrunk, ConvHead
        if (self.fuse_nets and isinstance(embedding, ConvGRUTrunk) and isinstance(head, ConvHead)
                and embedding.gru_tower.gru.hidden_size == 64 and embedding.gru_tower.gru.input_size == 64
                and embedding.gru_tower.gru.num_layers == 1 and next(embedding.parameters()).is_cuda):
            def build():
                from .fused import FusedValueNet
                return FusedValueNet(embedding, head).to(self.device).eval()
            fused = self._fused.get("value", (embedding, head), build, self._scope)
            fused.precision = self.precision
            return fused
        if (self.fuse_nets and (self.precision != "f32" or self.fuse_trunk_f32) and isinstance(embedding, EnformerTrunk)
                and isinstance(head, ConvHead) and next(embedding.parameters()).is_cuda):
            # BASELINE configs[3]'s Enformer-shaped trunk on the hand-written kernels (svdd_trunk.hip): "f32" = one fp32 operand
            # plane, fp32 MFMAs (the reference's precision; round 4); the x3 modes map to bf16x3 (bf16 keeps fp32's exponent
            # range: no operand scaling needed), the one-pass modes to bf16
            tp = "f32" if self.precision == "f32" else "bf16x3" if self.precision.endswith("x3") else "bf16"

            def build():
                from .fused_trunk import FusedEnformerValueNet
                # a trunk whose GEMM shapes the kernels do not take (output channels must come in 128s, input channels in
                # 32s: a 384-channel toy trunk has a 192-channel stem) stays on the PyTorch modules — said once per build, and
                # ONLY for that documented reason: an assertion while packing a supported trunk is a bug and propagates
                ok, why = FusedEnformerValueNet.supports(embedding, head)
                if ok:
                    return FusedEnformerValueNet(embedding, head, tp)
                warnings.warn(f"Enformer-shaped value trunk stays on the PyTorch modules: {why}", stacklevel=4)   # value_callable's caller
                return None
            fused = self._fused.get(("trunk", tp), (embedding, head), build, self._scope)
            if fused is not None:
                return fused
        if self.precision in ("bf16", "f16"):                       # opaque nets: PyTorch-ROCm's own 16-bit kernels
            dt = torch.bfloat16 if self.precision == "bf16" else torch.float16

            def autocast_value(onehot):
                with torch.autocast("cuda", dtype=dt):
                    return head(embedding(onehot)).float()
            return autocast_value
        return lambda onehot: head(embedding(onehot))

    def reward_callable(self, reward_model):
        """The callable the engine uses for `reward_model(onehot_t [n,4,L])` -> [n,n_tasks,1]."""
        from .motifs import GuidedReward
        from .value_nets import RewardModel
        if isinstance(reward_model, GuidedReward):                  # a reward net plus a motif term: the same wrapper
            base = reward_model.reward_model                        # around the net's own callable (the fused net, from the cache)
            return GuidedReward(None if base is None else self.reward_callable(base), reward_model.motif_reward)
        if self.fuse_nets and isinstance(reward_model, RewardModel):
            fused = self.value_callable(reward_model.embedding, reward_model.head)
            if isinstance(fused, nn.Module):
                return fused
        return reward_model

    def _backbone_logits(self, x_u8):
        """Raw backbone output for tokens x (sigma is zeroed when time_conditioning is False, :334-335)."""
        if isinstance(self.backbone, CNNModel) and not self.time_conditioning:
            if self.fuse_nets and x_u8.is_cuda and self.backbone.args.hidden_dim in (64, 128, 256):
                return self._fused_backbone()(x_u8)
            return self.backbone(x_u8, None, zero_sigma=True)
        sigma = torch.zeros(x_u8.shape[0], device=x_u8.device)
        return self.backbone(x_u8.long(), sigma).float()

    def _prior_dedup_ok(self, x_u8):
        """True when the net evaluations of the prior state x_u8 (every row all-MASK by construction) may run on one row: more than
        one row, and the one-launch backbone kernel (a row's logits are then the same bits wherever and with whomever it is evaluated)."""
        return (self.dedup_prior and not self._from_state and x_u8.shape[0] > 1 and x_u8.is_cuda and not _capturing() and
                self._fused_backbone_or_none(x_u8.shape[1]) is not None)

    def _prior_logits(self, x_u8):
        """Backbone logits of the PRIOR state (the first forward of every sampler loop): one row forwarded, broadcast to all B."""
        if self._prior_dedup_ok(x_u8):
            B, L = x_u8.shape
            return self._backbone_logits(x_u8[:1].contiguous()).expand(B, L, self.vocab_size).contiguous()
        return self._backbone_logits(x_u8)

    def _step_scalars(self, t, dt):
        """(mct, mcs, mct - mcs) for an explicit (t, dt) as the per-step API receives them
        (:1176-1187), evaluated on the host with the reference's fp32 ops."""
        t0 = t.reshape(-1)[:1].detach().float().cpu().view(1, 1)
        sigma_t, _ = self.noise(t0)
        sigma_s, _ = self.noise(t0 - dt)
        mct = 1 - torch.exp(-sigma_t.squeeze(-1))
        mcs = 1 - torch.exp(-sigma_s.squeeze(-1))
        return float(mct), float(mcs), float(mct - mcs)

    def _step_index(self, t, dt):
        """Index i of the diffusion step a per-step call belongs to: the reference loops call the per-step methods with
        t_i = 1 - i * dt (diffusion_gosai.py:1036-1043). It keys the Philox counter, so that a caller who drives the
        per-step API draws fresh uniforms at every step (with a constant key a position that stays MASK would see the
        same Gumbel noise again and again)."""
        t0 = float(t.reshape(-1)[0])
        return max(0, int(round((1.0 - t0) / float(dt))))

    def _replay_layout(self, logits):
        """Memory order in which the REFERENCE consumes its uniforms: rand_like(q_xs) fills in the
        memory order of the reference backbone's output — [b][v][l] for its CNN, whose output is a
        permuted view (models/dnaconv.py:201) — whatever layout this engine's backbone emits."""
        if self.config.backbone == "cnn":
            return ops.LAYOUT_BVL
        return ops.layout_of(logits)[1]

    def _rng(self, step, M, B, L, logits):
        if self.rng_mode == "replay":
            ul = self._replay_layout(logits)
            # a rank of a batch-sharded decode replays the WHOLE batch's stream and reads its rows (svdd_rng.uniforms_rows)
            shard = self._shard if (self._shard is not None and self._shard[3] > 1) else None
            rows = shard[2] if shard else B
            shape = (M, rows, L, 5) if ul == ops.LAYOUT_BLV else (M, rows, 5, L)
            extra = dict(row_offset=shard[0], uniforms_rows=rows) if shard else {}
            if shard and not (self._scope_depth > 0 and self._replay_checked == self._scope_id):
                # every rank replays the whole batch's stream and slices its rows: only the reference's run if all ranks start from
                # the same generator state (a rank seeded per rank, or one that drew anything extra, would silently decode other tokens)
                import hashlib
                from . import distributed
                digest = hashlib.sha1(torch.get_rng_state().numpy().tobytes()).digest()
                distributed.assert_same_on_all_ranks(int.from_bytes(digest[:8], "little", signed=True),
                                                     "sharded replay decode: torch's CPU generator state (seed every rank identically)")
                self._replay_checked = self._scope_id
            if self.replay_rng == "device" and self._scope_depth > 0 and logits.is_cuda and not _capturing():
                # the same stream, generated on the device (svdd_mt19937_uniform_f32): the generator's state is uploaded at the
                # first draw of a sampler call and written back into torch's global generator when the call returns
                if self._replay_stream is None:
                    self._replay_stream = ops.DeviceReplayStream(logits.device)
                u = self._replay_stream.uniforms(M * rows * L * 5).view(shape)
            else:
                u = torch.rand(shape).to(logits.device, non_blocking=True)   # torch's global CPU generator
            return ops.Rng(uniforms=u, uniforms_layout=ul, **extra)
        if self.rng_mode == "philox":
            return ops.Rng(seed=self.philox_seed, row_offset=self.row_offset, step=self._step_base + step)
        raise ValueError(f"rng_mode {self.rng_mode!r}")

    def _select_args(self, step):
        """(ABI constant of select_mode, the Rng a multinomial select draws from at diffusion step `step` | None)."""
        mode = {"argmax": ops.SELECT_ARGMAX, "multinomial": ops.SELECT_MULTINOMIAL}[self.select_mode]
        if mode != ops.SELECT_MULTINOMIAL:
            return mode, None
        if self.rng_mode != "philox":
            raise ValueError("select_mode='multinomial' needs rng_mode='philox'")
        return mode, ops.Rng(seed=self.philox_seed, row_offset=self.row_offset, step=self._step_base + step)

    def _select(self, scores, cand, step):
        mode, rng = self._select_args(step)
        x_next, _, _ = ops.select(scores, cand, mode=mode, rng=rng, want_soft=False)
        return x_next

    def _value_scores(self, embedding, head, onehot, B, M, cand=None, x_u8=None):
        """scores[b, m] = head(embedding(onehot of candidate m of sample b)) (:1207-1209,1219)."""
        fn = self.value_callable(embedding, head)
        if self.value_batching == "batched":
            if cand is not None and hasattr(fn, "candidates_ok") and fn.candidates_ok(onehot.shape[1], M):
                return fn.forward_candidates(onehot, cand, x_u8).reshape(B, M).float()
            return fn(onehot).reshape(B, M).float()
        oh = onehot.view(B, M, onehot.shape[1], 4)
        return torch.stack([fn(oh[:, m].contiguous()).reshape(B) for m in range(M)], dim=1).float()

    def _batch_size(self, eval_sp_size):
        return self.config.loader.eval_batch_size if eval_sp_size is None else eval_sp_size

    def _num_steps(self, num_steps):
        return self.config.sampling.steps if num_steps is None else num_steps

    def _decode_start(self, num_steps, eps, eval_sp_size, x_init=None, t_start=1.0, check_tokens=True):
        """What every sampler loop opens with -> (B, L, S, schedule table [S, 3], the all-MASK prior x_T as u8 [B, L], :751-753).
        x_init [B, L] (tokens 0..3, 4 = MASK, on the model's device): the decode starts from this state at t = t_start instead — the
        schedule is linspace(t_start, eps, S + 1), S = max(1, ceil(t_start * config.sampling.steps)) unless given (the full decode's
        dt), and the shortcuts that rely on B identical all-MASK rows are off for the decode (self._from_state; _prior_dedup_ok).
        check_tokens False: the caller vouches for the tokens (a state svdd_refine_remask wrote) and no value is read back."""
        self._require_gpu()
        self._from_state = x_init is not None
        if x_init is None:
            if float(t_start) != 1.0:
                raise ValueError("t_start needs a start state (x_init): the all-MASK prior belongs to t = 1")
            B, L, S = self._batch_size(eval_sp_size), self.config.model.length, self._num_steps(num_steps)
            sched, _, _ = self._schedule(S, eps)
            return B, L, S, sched, torch.full((B, L), self.mask_index, dtype=torch.uint8, device=self.device)
        if self.time_conditioning:
            raise NotImplementedError("decoding from a given state: time-conditioned backbones are not supported (the work-skipping "
                                      "loops and the fused backbone run at sigma = 0)")
        if not isinstance(x_init, torch.Tensor) or not x_init.is_cuda or x_init.device != self.device:
            raise ops.SvddError("x_init must be a tensor on the model's GPU (the SVDD hot path has no CPU fallback)")
        L = self.config.model.length
        if x_init.dim() != 2 or x_init.shape[0] == 0 or x_init.shape[1] != L:
            raise ValueError(f"x_init must be [B, {L}] (config.model.length) with B > 0, got {tuple(x_init.shape)}")
        if x_init.dtype.is_floating_point or x_init.dtype == torch.bool:
            raise ValueError(f"x_init must hold integer tokens, got {x_init.dtype}")
        self._check_t(t_start, eps, "t_start")
        if check_tokens:
            lo, hi = torch.aminmax(x_init)
            if int(lo) < 0 or int(hi) > self.mask_index:
                raise ops.SvddError(f"x_init holds a token outside 0..{self.mask_index} (0..3 = A, C, G, T; {self.mask_index} = MASK)")
        S = max(1, math.ceil(float(t_start) * self.config.sampling.steps)) if num_steps is None else int(num_steps)
        if S <= 0:
            raise ValueError(f"num_steps must be positive, got {num_steps}")
        sched, _, _ = self._schedule(S, eps, t_start)
        return x_init.shape[0], L, S, sched, self._tokens_u8(x_init).contiguous().clone()

    @staticmethod
    def _check_t(t, eps, name):
        if not (float(eps) < float(t) <= 1.0):
            raise ValueError(f"{name} must lie in (eps, 1] = ({eps}, 1], got {t}")

    def _step_result(self, x_next, x, q):
        """What the reference's per-step methods return: (x_next int64, x, q_xs, copy_flag)."""
        return x_next.long(), x, q, (x != self.mask_index).to(x.dtype)

    def _noise_removal(self, x_u8, logits=None):
        """:1049-1060 — x = forward(x, sigma(t_last))[:, :, :-1].argmax(-1) ; returns int64. `logits`: the backbone
        output for x_u8 when the caller already holds it (work-skipping SVDD-PM)."""
        if self.config.sampling.noise_removal:
            if self.sampler == "analytic":
                raise NotImplementedError("analytic sampler is not on the reference's decode path")
            if logits is None:
                logits = self._backbone_logits(x_u8)
            self._record(logits, None, x_u8)
            return ops.finalize(logits, x_u8)
        return x_u8.long()

    def _record(self, logits, scores, x=None):
        if self.trace is not None:
            self.trace.append((logits.detach().clone(), None if scores is None else scores.detach().clone()))
        if self.state_trace is not None and x is not None:
            self.state_trace.append(x.detach().clone())

    # ---------------------------------------------------------- reference API: basics ----
    def _process_sigma(self, sigma):
        if sigma.ndim > 1:
            sigma = sigma.squeeze(-1)
        if not self.time_conditioning:
            sigma = torch.zeros_like(sigma)
        assert sigma.ndim == 1, sigma.shape
        return sigma

    @_decode_scope
    def forward(self, x, sigma):
        """Returns log score: backbone logits under the SUBS parameterization (:339-357)."""
        self._require_gpu()
        sigma = self._process_sigma(sigma)
        x_u8 = self._tokens_u8(x)
        return ops.subs_logp(self._backbone_logits(x_u8), x_u8)

    def forward2(self, x_onehot, x, sigma):
        """Differentiable log score on a one-hot input (:359-377), used by the DPS baseline. Autograd
        must see every op, so the SUBS step is expressed in torch here."""
        sigma = self._process_sigma(sigma)
        fb = self._dps_one_launch(x_onehot) if self._dps_hard_onehot else None
        if fb is not None:
            # DPS: x_onehot IS one_hot(x) (:1308) — the whole backbone as ONE launch each way (forward = the inference kernel's
            # bits + saved statistics, backward = svdd_backbone_cnn_grad_f32): no layer-wise launches, no saved activations rows
            logits = fb.forward_with_grad(x_onehot, self._tokens_u8(x))
            self._dps_raw_logits = logits.detach()
        elif isinstance(self.backbone, CNNModel):
            # dilated convs on the hand-written kernel, both directions — for this call only (the flag does not outlive it:
            # a later backbone.forward2 by the user gets plain autograd unless asked otherwise)
            was = self.backbone.hip_convs
            self.backbone.hip_convs = bool(self.fuse_nets)
            if self.backbone.hip_convs:
                self._validate_conv_packs()
            try:
                logits = self.backbone.forward2(x_onehot, sigma)
            finally:
                self.backbone.hip_convs = was
        else:
            logits = self.backbone.forward2(x_onehot, sigma)
        neg = torch.zeros(self.vocab_size, device=logits.device)
        neg[self.mask_index] = self.neg_infinity
        logits = logits + neg
        logits = logits - torch.logsumexp(logits, dim=-1, keepdim=True)
        unmasked = (x != self.mask_index)
        fixed = torch.full_like(logits, self.neg_infinity).scatter(-1, x.clamp(max=self.vocab_size - 1)[..., None], 0.0)
        return torch.where(unmasked[..., None], fixed, logits)

    def _dps_one_launch(self, x_onehot):
        """The fused backbone when the differentiable pass of a DPS step can run as one launch each way, else None."""
        if not (self.fuse_nets and self.dps_one_launch and x_onehot.is_cuda and not self.time_conditioning
                and isinstance(self.backbone, CNNModel) and not self.backbone.training):
            return None
        fb = self._fused_backbone_or_none(x_onehot.shape[1])
        return fb if fb is not None and fb.grad_ok(x_onehot.shape[1]) else None

    def _sample_prior(self, *batch_dims):
        return self.mask_index * torch.ones(*batch_dims, dtype=torch.int64)          # :751-753

    def transform_samples(self, samples, num_classes=4):
        """tokens -> one-hot(4), MASK rows zero; int64 like the reference's F.one_hot (:1462-1470)."""
        if samples.is_cuda and num_classes == 4:
            return ops.transform_samples(self._tokens_u8(samples)).long()
        mask = samples != 4
        return F.one_hot((samples * mask).long(), num_classes=num_classes) * mask.unsqueeze(-1)

    # --------------------------------------------------------------- per-step updates ----
    @_decode_scope
    @torch.no_grad()
    def _ddpm_update_finetune(self, x, t, dt):
        """Un-guided ancestral step (:1147-1172) -> (x_next, x, q_xs, copy_flag)."""
        self._require_gpu()
        _, mcs, dm = self._step_scalars(t, dt)
        x_u8 = self._tokens_u8(x)
        logits = self._backbone_logits(x_u8)
        B, L = x_u8.shape
        cand, _, q = ops.propose(logits, x_u8, dm, mcs, 1, self._rng(self._step_index(t, dt), 1, B, L, logits), want_q=True)
        return self._step_result(cand[:, 0], x, q)

    @_decode_scope
    @torch.no_grad()
    def _ddpm_update_finetune_controlled(self, x, t, dt, pre_scorer_embedding, pre_scorer_head, repeats=10):
        """One SVDD-MC step (:1174-1228) -> (final_samples, x, q_xs, copy_flag)."""
        self._require_gpu()
        _, mcs, dm = self._step_scalars(t, dt)
        x_u8 = self._tokens_u8(x)
        logits = self._backbone_logits(x_u8)
        B, L = x_u8.shape
        step = self._step_index(t, dt)
        cand, onehot, q = ops.propose(logits, x_u8, dm, mcs, repeats, self._rng(step, repeats, B, L, logits), want_q=True)
        scores = self._value_scores(pre_scorer_embedding, pre_scorer_head, onehot, B, repeats, cand, x_u8)
        x_next = self._select(scores, cand, step)
        return self._step_result(x_next, x, q)

    @_decode_scope
    @torch.no_grad()
    def _ddpm_update_finetune_controlled_twedie(self, x, t, dt, reward_model, repeats=10, options="True", task="dna"):
        """One SVDD-PM step (:1373-1460) -> (final_samples, x, q_xs, copy_flag)."""
        self._require_gpu()
        _, mcs, dm = self._step_scalars(t, dt)
        x_u8 = self._tokens_u8(x)
        logits = self._backbone_logits(x_u8)
        B, L = x_u8.shape
        step = self._step_index(t, dt)
        cand, _, q = ops.propose(logits, x_u8, dm, mcs, repeats, self._rng(step, repeats, B, L, logits), want_q=True)
        scores = self._tweedie_scores(cand, reward_model, options, task)
        x_next = self._select(scores, cand, step)
        return self._step_result(x_next, x, q)

    def _tweedie_scores(self, cand, reward_model, options, task):
        """scores[b,m] = reward_model(x0hat(candidate))[:, 0] (:1413-1436)."""
        if task == "rna_saluki":
            raise NotImplementedError("rna_saluki needs a data file the reference hard-codes by absolute path "
                                      "(diffusion_gosai.py:1478); unsupported offline")
        B, M, L = cand.shape
        flat = cand.reshape(B * M, L)
        if options == "True":
            oh, _ = ops.x0hat(self._backbone_logits(flat), flat)          # :1415-1419
        else:
            oh = ops.transform_samples(flat, transposed=True)             # heuristic branch :1420-1424
        return self.reward_callable(reward_model)(oh)[:, 0].reshape(B, M).float()   # :1430,1436

    @_decode_scope
    @torch.no_grad()
    def _ddpm_update_finetune_controlled_TDS(self, x, t, dt, reward_model, alpha=1.0):
        """One SMC/TDS step (:1230-1284) -> x_next. Consumes B doubles of numpy's global RandomState,
        like the reference's np.random.choice."""
        self._require_gpu()
        _, mcs, dm = self._step_scalars(t, dt)
        x_u8 = self._tokens_u8(x)
        return self._tds_step(x_u8, dm, mcs, reward_model, alpha, self._step_index(t, dt)).long()

    def _tds_step(self, x_u8, dm, mcs, reward_model, alpha, step, carry=None):
        """One SMC/TDS step. `carry`: None, or a dict the decode loop threads through the steps for EXACT reuse: the
        resampled particles x_next = sample[idx] are copies of proposals whose backbone logits and x0-hat reward this step
        already computed, so the next step's forward(x_next) and its denominator reward are row gathers of this step's
        forward(sample) and numerator reward (2 of the 3 net evaluations of a step; bit-identical because the hand-written
        kernels' output for a row does not depend on where the row sits in the batch)."""
        B, L = x_u8.shape
        have = carry is not None and "logits" in carry
        prior = carry is not None and carry.pop("prior", False)           # first step of a decode: x is the all-MASK prior
        logits = carry["logits"] if have else (self._prior_logits(x_u8) if prior else self._backbone_logits(x_u8))
        cand, _, _ = ops.propose(logits, x_u8, dm, mcs, 1, self._rng(step, 1, B, L, logits))
        sample = cand[:, 0].contiguous()
        logits_s = self._backbone_logits(sample)
        oh_num, _ = ops.x0hat(logits_s, sample)                           # :1263-1268
        reward_fn = self.reward_callable(reward_model)
        reward_num = reward_fn(oh_num)[:, 0][:, 0].float()                # :1269
        if have and "den" in carry:
            reward_den = carry["den"]
        else:
            # forward(x, sigma_s) == forward(x, sigma_t): sigma is zeroed (:334-335), so `logits` is reused (:1273)
            oh_den, _ = ops.x0hat(logits, x_u8)
            reward_den = reward_fn(oh_den)[:, 0][:, 0].float()            # :1277
        keep_logits = carry is not None and carry.get("keep_logits")
        keep_den = carry is not None and carry.get("keep_den")
        shard = self._shard
        if shard is not None and shard[3] > 1:
            # batch sharded over GPUs: the resample draws ancestors from the WHOLE batch — one all-gather, then every rank
            # resamples the whole batch identically and keeps its rows (distributed.tds_exchange)
            from . import distributed
            u_all = torch.from_numpy(np.random.random_sample(shard[2]))
            extra = logits_s.reshape(B, -1) if keep_logits else None
            sample_all, num_all, den_all, u, extra_all = distributed.tds_exchange(shard, sample, reward_num, reward_den,
                                                                                  u_all, extra)
            x_all, idx = ops.tds_resample(num_all, den_all, alpha, sample_all, u)
            mine = idx[shard[0]:shard[1]].long()
            x_next, src_logits, src_num = x_all[shard[0]:shard[1]].contiguous(), extra_all, num_all
        else:
            u = torch.from_numpy(np.random.random_sample(B)).to(x_u8.device)   # what np.random.choice draws (:1282)
            x_next, idx = ops.tds_resample(reward_num, reward_den, alpha, sample, u)
            mine, src_logits, src_num = idx.long(), logits_s.reshape(B, -1), reward_num
        if carry is not None:
            carry.pop("logits", None), carry.pop("den", None)
            if keep_logits:
                carry["logits"] = src_logits.index_select(0, mine).view(B, *logits_s.shape[1:])
            if keep_den:
                carry["den"] = src_num.index_select(0, mine)
        return x_next

    def _tds_carry(self, reward_model, L):
        """What a TDS decode may reuse from step to step (see _tds_step): only results of kernels whose output for a row
        is independent of the batch around it — the one-launch backbone, the hand-written value-net kernels."""
        if not (self.skip_unchanged and self.fuse_nets):
            return None
        from .fused import FusedValueNet
        fn = self.reward_callable(reward_model)
        return {"keep_logits": self._fused_backbone_or_none(L) is not None,
                "keep_den": isinstance(fn, FusedValueNet) and fn.kernels_ok(L)}

    # ------------------------------------------------------------------ DPS baseline ----
    def compute_gradient_DPS(self, x_onehot, x, reward_model, sigma_s, copy_flag):
        """d mean(reward(softmax(E[x0|x_t]))) / d onehot(x_t)  (reference :1321-1330). Pure autograd: the
        differentiable backbone entry `forward2` and the reward net are run as plain torch modules."""
        x_onehot.requires_grad_(True)
        keep = copy_flag[:, :, None]
        logp = self.forward2(x_onehot, x, sigma_s)
        self._dps_logp = logp.detach()                            # log p(x0 | x_t): _dps_guided_q takes its q_xs from it
        expected_x0 = keep * x_onehot + (1 - keep) * logp
        probs = torch.softmax(expected_x0, dim=2)
        fn = self.reward_callable(reward_model) if (self.fuse_nets and self.dps_one_launch and x_onehot.is_cuda) else None
        from .fused import FusedValueNet
        if isinstance(fn, FusedValueNet) and fn.grad_ok(x_onehot.shape[1]):
            # the reward net without MIOpen (round 5): convolutions on svdd_conv1d_cl_f32 both ways, GRU on the BPTT kernels
            scores = fn.forward_grad(probs[:, :, 0:4].contiguous())[:, 0]
            scores.mean().backward()
            return x_onehot.grad.clone()
        with self._gru_backward_ready([reward_model], x_onehot.is_cuda):
            reward_model(probs.transpose(1, 2)[:, 0:4, :])[:, 0].mean().backward()
        return x_onehot.grad.clone()

    @contextlib.contextmanager
    def _gru_backward_ready(self, modules, on_gpu):
        """The recurrent modules of `modules` made ready for a backward pass on the GPU, for the span of the context (the loss is
        built AND back-propagated inside it). MIOpen's fused RNN backward insists on train(). A GRU without inter-layer dropout
        computes the same function in both modes, so only those modules are switched (BatchNorm / Dropout stay in eval): 113 -> 54 ms
        per gradient at B = 256 against the per-timestep native cells (400 cell launches forward + backward). Any other recurrent
        module falls back to the native cells. Where the GRU is the reward net's 64-unit bidirectional one, neither is used: the
        recurrence runs on the hand-written forward + BPTT kernels (csrc/svdd_gru_train.hip; 35.9 -> ~1 ms of the gradient at
        B = 256). On the CPU nothing is touched: a dropout-free GRU is the same function in both modes there too."""
        hip = [b for m in modules for b in self._hip_gru_blocks(m)] if (self.fuse_nets and on_gpu) else []
        taken = {id(b.gru) for b in hip}
        rnns = [r for m in modules for r in m.modules() if isinstance(r, nn.RNNBase) and id(r) not in taken]
        flip = [r for r in rnns if isinstance(r, nn.GRU) and r.dropout == 0 and not r.training] if on_gpu else []
        native = on_gpu and len(flip) != len([r for r in rnns if not r.training])
        for r in flip:
            r.train()
        try:
            with torch.backends.cudnn.flags(enabled=not native) if on_gpu else contextlib.nullcontext():
                yield
        finally:
            for r in flip:
                r.eval()
            for b in hip:
                b._hip_gru = None

    def _hip_gru_blocks(self, reward_model):
        """GRUBlocks of `reward_model` whose nn.GRU the kernels of csrc/svdd_gru_train.hip take (64 -> 64, one layer,
        bidirectional, eval mode or no dropout), switched to them; their re-packed weights are cached like the fused nets."""
        from .fused import GruBidirFunction, pack_gru, pack_gru_bwd
        from .value_nets import GRUBlock
        blocks = []
        for b in reward_model.modules():
            g = getattr(b, "gru", None)
            if not (isinstance(b, GRUBlock) and isinstance(g, nn.GRU) and g.hidden_size == 64 and g.input_size == 64 and
                    g.num_layers == 1 and g.bidirectional and g.bias and g.batch_first and not g.training):
                continue

            def build(g=g):
                wpack, bpack = pack_gru(g)
                dev = next(g.parameters()).device
                return wpack.to(dev), bpack.to(dev), pack_gru_bwd(g).to(dev)
            packs = self._fused.get("gru_packs", (g,), build, self._scope)
            b._hip_gru = lambda xx, p=packs: GruBidirFunction.apply(xx, *p)
            blocks.append(b)
        return blocks

    def _dps_guided_q(self, x_u8, mcs, dm, reward_model, guidance_scale):
        """The guided transition weights q_xs of one DPS step (:1306-1314) -> fp32 [B, L, 5]."""
        B, L = x_u8.shape
        fused = self._dps_fused_nets(x_u8, reward_model)
        if fused is not None:
            # round 6: the whole step without autograd — the one-launch backbone pair, the per-position pieces (K9: svdd_dps_probs /
            # _probs_bwd / _guided_q) and the reward net's gradient pass on hand-written kernels (FusedValueNet.mean_score_input_grad):
            # 22 launches where rounds 4-5 issued ~200 (torch element-wise ops and their autograd twins between the kernels)
            from .fused import backbone_cnn_grad, backbone_cnn_save
            fb, fn = fused
            with torch.no_grad():
                pk = fb.ol_pack()
                logits, saved = backbone_cnn_save(x_u8.contiguous(), pk)              # the inference kernel's bits + saved statistics
                dprobs = fn.mean_score_input_grad(ops.dps_probs(logits, x_u8))        # :1325-1329
                dlogits, direct = ops.dps_probs_bwd(logits, x_u8, dprobs)
                dx_bb = backbone_cnn_grad(dlogits, pk, fb.grad_pack(), saved)
                return ops.dps_guided_q(logits, x_u8, dx_bb, direct, dm, mcs, guidance_scale)     # :1306-1314
        x = x_u8.long()
        copy_flag = (x != self.mask_index).to(x.dtype)
        x_onehot = F.one_hot(x, num_classes=self.vocab_size).float()                          # :1308
        # The reference evaluates the backbone twice per step on the same x_t (forward() for q_xs, :1306 ; forward2() inside the
        # gradient, :1324). With the one-launch pair the differentiable forward IS the inference kernel, bit for bit (same kernel
        # template, plus stores): its raw logits serve both, through the same SUBS kernel — zero guidance stays bit-for-bit the
        # un-guided decode (tests/test_configs_gpu.py), and the second, identical forward is not run.
        # (a split-precision mode keeps its own sampling forward for q_xs — the mode's bits — and takes only the gradient from the
        #  fp32 pair: the differentiable pass has always been fp32)
        pair = self._dps_one_launch(x_onehot) is not None            # the gradient comes from the one-launch fp32 pair ...
        reuse = pair and self.precision == "f32"                     # ... whose forward logits also give q_xs
        legacy_single = self.dps_single_forward and not pair         # round 4's opt-in, layer-wise path only
        if not reuse and not legacy_single:
            with torch.no_grad():
                q_xs = torch.exp(ops.subs_logp(self._backbone_logits(x_u8), x_u8)) * float(dm)   # :1306-1307
        sigma = torch.zeros(B, device=x.device)
        self._dps_hard_onehot = True
        try:
            with torch.enable_grad():
                x_grad = self.compute_gradient_DPS(x_onehot, x, reward_model, sigma, copy_flag)   # :1310
        finally:
            self._dps_hard_onehot = False
        with torch.no_grad():
            if reuse:
                q_xs = torch.exp(ops.subs_logp(self._dps_raw_logits, x_u8)) * float(dm)       # :1306-1307 on the very same logits
            elif legacy_single:
                # The reference evaluates the backbone twice per step on the same x_t with the same (zeroed) sigma: forward() for
                # q_xs (:1306) and forward2() inside the gradient (:1324). They are one function; the differentiable pass's log-probs
                # are taken for both (round-off apart: ~1e-6, far inside the 1e-3 .. 1e-2 that the gradient's own ReLU decisions
                # move it by). dps_single_forward = False (the default) runs the second forward like the reference.
                q_xs = torch.exp(self._dps_logp) * float(dm)
            self._dps_raw_logits = self._dps_logp = None
            guidance = guidance_scale * (x_grad - x_grad[:, :, self.mask_index][:, :, None])   # :1311
            q_xs[:, :, self.mask_index] = float(mcs)                                          # :1312
            return q_xs * guidance.exp()                                                      # :1314

    def _dps_fused_nets(self, x_u8, reward_model):
        """(fused backbone, fused reward net) when a DPS step can run without autograd, else None: the one-launch fp32 backbone pair at
        this length, the reference-shaped ConvGRU reward net on the hand-written kernels, exact-fp32 mode (a split-precision mode keeps
        its own sampling forward for q_xs: the autograd path), dps_fused on."""
        if not (self.dps_fused and self.dps_one_launch and self.fuse_nets and self.precision == "f32" and x_u8.is_cuda
                and not self.time_conditioning and isinstance(self.backbone, CNNModel) and not self.backbone.training):
            return None
        L = x_u8.shape[1]
        fb = self._fused_backbone_or_none(L)
        if fb is None or not fb.grad_ok(L):
            return None
        from .fused import FusedValueNet
        fn = self.reward_callable(reward_model)
        if not (isinstance(fn, FusedValueNet) and fn.grad_ok(L)):
            return None
        return fb, fn

    def _dps_step(self, x_u8, mcs, dm, reward_model, guidance_scale, step):
        B, L = x_u8.shape
        q_xs = self._dps_guided_q(x_u8, mcs, dm, reward_model, guidance_scale)
        with torch.no_grad():
            cand, _ = ops.sample_categorical(q_xs, x_u8, 1, self._rng(step, 1, B, L, q_xs))   # :1316-1319
        return cand.view(B, L)

    @_decode_scope
    def _ddpm_update_finetune_controlled_DPS(self, x, t, dt, reward_model, guidance_scale):
        """One DPS (gradient-guidance) step (:1286-1319) -> x_next."""
        self._require_gpu()
        _, mcs, dm = self._step_scalars(t, dt)
        return self._dps_step(self._tokens_u8(x), mcs, dm, reward_model, guidance_scale, self._step_index(t, dt)).long()

    @_decode_scope
    def controlled_sample_DPS(self, reward_model, guidance_scale, num_steps=None, eps=1e-5, eval_sp_size=None,
                              sample_M=10):
        """DPS baseline decode (:980-1019). Not under no_grad in the reference either: it back-propagates."""
        _refuse_motif_reward("controlled_sample_DPS", reward_model)
        B, L, S, sched, x = self._decode_start(num_steps, eps, eval_sp_size)
        for i in range(S):
            x = self._dps_step(x, sched[i, 1], sched[i, 2], reward_model, guidance_scale, i)
        with torch.no_grad():
            return self._noise_removal(x)

    # ------------------------------------------------------------ classifier guidance ----
    def compute_gradient(self, x, pre_scorer_embedding, pre_scorer_head):
        """d mean(head(embedding(x))) / d x for the masked one-hot x [B, L, 4] (reference :1362-1371): the mean runs over the batch AND
        the tasks, so a row's gradient carries a 1 / B factor. Pure autograd, on whatever device x lives (CPU included); on the GPU the
        value net's GRUs are prepared for the backward pass by _gru_backward_ready, as in compute_gradient_DPS. The value net's modes
        are otherwise left as the caller set them."""
        x.requires_grad_(True)
        mods = [m for m in (pre_scorer_embedding, pre_scorer_head) if isinstance(m, nn.Module)]
        with torch.enable_grad(), self._gru_backward_ready(mods, x.is_cuda):
            pre_scorer_head(pre_scorer_embedding(x)).mean().backward()
        return x.grad.clone()

    def _classifier_fused_value(self, embedding, head, L):
        """The value net as FusedValueNet when its input gradient can run without autograd (mean_score_input_grad: the reference-shaped
        ConvGRU net with one task, at a length the gradient kernels take), else None."""
        from .value_nets import ConvGRUTrunk
        if not (self.fuse_nets and isinstance(embedding, ConvGRUTrunk)):
            return None
        from .fused import FusedValueNet
        fn = self.value_callable(embedding, head)
        if isinstance(fn, FusedValueNet) and fn.grad_ok(L) and fn.w_eff.shape[1] == 1:
            return fn
        return None

    def _classifier_grad(self, onehot, embedding, head):
        """x_grad [B, L, 4] of one classifier-guidance step (:1354) from the masked one-hot of x_t -> (grad, fused?)."""
        fn = self._classifier_fused_value(embedding, head, onehot.shape[1]) if onehot.is_cuda else None
        if fn is not None:
            with torch.no_grad():
                return fn.mean_score_input_grad(onehot), True
        return self.compute_gradient(onehot.detach().clone(), embedding, head), False

    def _classifier_step(self, x_u8, onehot, logits, dm, mcs, embedding, head, guidance_scale, step, want_q=False):
        """x_grad (fused or autograd), then ONE svdd_classifier_propose launch: the guided draw, the copy_flag merge, the next step's
        value-net input -> (x_next u8, onehot_next f32 [B, L, 4], un-guided q_xs | None)."""
        B, L = x_u8.shape
        grad, fused = self._classifier_grad(onehot, embedding, head)
        self._classifier_fused_last = fused
        with torch.no_grad():
            return ops.classifier_propose(logits, x_u8, grad, dm, mcs, guidance_scale, self._rng(step, 1, B, L, logits), want_q=want_q)

    def _classifier_checks(self, guidance_scale):
        if guidance_scale is None:
            raise ValueError("controlled_sample_classfier needs a guidance_scale (the reference's default None fails at "
                             "`None * x_grad`, diffusion_gosai.py:1357)")
        if self._shard is not None and self._shard[3] > 1:
            raise NotImplementedError("classifier guidance is not batch-sharded: the gradient's batch mean would use the local batch")
        self._require_gpu()

    @_decode_scope
    def _ddpm_update_finetune_classfier(self, x, t, dt, pre_scorer_embedding, pre_scorer_head, guidance_scale):
        """One classifier-guidance step (:1332-1360) -> (x_next, x, q_xs, copy_flag); q_xs is the UN-guided one, as in the reference."""
        self._classifier_checks(guidance_scale)
        _, mcs, dm = self._step_scalars(t, dt)
        x_u8 = self._tokens_u8(x)
        with torch.no_grad():
            logits = self._backbone_logits(x_u8)
            onehot = ops.transform_samples(x_u8)
        x_next, _, q = self._classifier_step(x_u8, onehot, logits, dm, mcs, pre_scorer_embedding, pre_scorer_head, guidance_scale,
                                             self._step_index(t, dt), want_q=True)
        return self._step_result(x_next, x, q)

    @_decode_scope
    def controlled_sample_classfier(self, pre_scorer_embedding, pre_scorer_head, num_steps=None, eps=1e-5, eval_sp_size=None,
                                    guidance_scale=None):
        """Classifier-guidance decode (reference :1064-1104): per step the backbone forward, the value net's input gradient
        x_grad = d mean(head(embedding(onehot(x_t)))) / d onehot and one draw from the SIGNED weights q_xs + guidance_scale * x_grad,
        then noise removal. With the reference-shaped ConvGRU value net (one task, fp32 gradient, L in the gradient kernels' set) a step
        is the backbone launch, the gradient pass's launches (FusedValueNet.mean_score_input_grad) and one svdd_classifier_propose: no
        autograd, no torch element-wise op. Any other value net takes its gradient through torch autograd (compute_gradient) before the
        same propose kernel. `precision` applies to the backbone forward that gives q_xs; the gradient is always fp32.
        Deviation from the reference: the value net is evaluated in the mode the caller left it in (the harness and the CLI put it in
        eval mode for every task; the reference's decode_classfier.py leaves it in train mode for task "rna", i.e. dropout on and
        batch-statistics BatchNorm, which makes that run irreproducible). guidance_scale=None raises ValueError (the reference fails
        with a TypeError). A batch-sharded decode is refused."""
        _refuse_motif_reward("controlled_sample_classfier", pre_scorer_embedding, pre_scorer_head)
        self._classifier_checks(guidance_scale)
        B, L, S, sched, x = self._decode_start(num_steps, eps, eval_sp_size)
        onehot = torch.zeros((B, L, 4), dtype=torch.float32, device=self.device)            # transform_samples of the prior
        for i in range(S):
            with torch.no_grad():
                logits = self._prior_logits(x) if i == 0 else self._backbone_logits(x)
            self._record(logits, None, x)
            x, onehot, _ = self._classifier_step(x, onehot, logits, sched[i, 2], sched[i, 1], pre_scorer_embedding, pre_scorer_head,
                                                 guidance_scale, i)
        with torch.no_grad():
            return self._noise_removal(x)

    controlled_sample_classifier = controlled_sample_classfier

    # ------------------------------------------------------------------ outer loops ----
    @_decode_scope
    @torch.no_grad()
    def decode_sample(self, num_steps=None, eps=1e-5, eval_sp_size=None, cdq=False):
        """Un-guided decode (:888-936) -> LongTensor[B,L]."""
        return self._unguided_sample(num_steps, eps, eval_sp_size, keep_mid=False)[0]

    @_decode_scope
    @torch.no_grad()
    def _sample(self, num_steps=None, eps=1e-5, eval_sp_size=None, cdq=False):
        """Un-guided decode that also returns the S-1 intermediate states (:820-886). cdq=True: the reference's CD-Q rollout
        (:839-853) -> (x_0 int64 [B, L], mid_x: S - 1 x int64 [B, L], all_time_mid_x: S x cdq_draws x int64 [B, L]): every step draws
        cdq_draws next states from the same q_xs (ONE backbone forward and one propose with M = cdq_draws here; the reference forwards
        10 times on identical input) and continues from the last one; mid_x[i] is all_time_mid_x[i][-1]. Replay mode consumes
        torch's generator as the reference's loop does (cdq_draws consecutive rand_like(q_xs) blocks per step). For drop-in
        parity: value_targets() builds the training set without these lists. The draw count is the engine knob `cdq_draws` (the
        reference hard-codes 10, :846; the parameter list is the reference's and stays)."""
        self._require_gpu()
        if not cdq:
            return self._unguided_sample(num_steps, eps, eval_sp_size, keep_mid=True)
        M = self._check_draws(self.cdq_draws)
        B, L, S, sched, x = self._decode_start(num_steps, eps, eval_sp_size)
        mid_x, all_time_mid_x = [], []
        for i in range(S):
            logits = self._prior_logits(x) if i == 0 else self._backbone_logits(x)
            cand, _, _ = ops.propose(logits, x, sched[i, 2], sched[i, 1], M, self._rng(i, M, B, L, logits))
            all_time_mid_x.append([cand[:, j].long() for j in range(M)])
            x, _, _ = ops.value_target(None, cand)                            # x = x0 after the draws' loop, :851
            if i != S - 1:
                mid_x.append(all_time_mid_x[i][-1])
        return self._noise_removal(x), mid_x, all_time_mid_x

    @staticmethod
    def _check_draws(draws):
        if int(draws) != draws or not 1 <= int(draws) <= ops._lib.MAX_M:
            raise ValueError(f"draws must be an integer in 1..{ops._lib.MAX_M}, got {draws}")
        return int(draws)

    # ------------------------------------------------- value-function training data: MC and CD-Q rollouts (ABI 17) ----
    @_decode_scope
    @torch.no_grad()
    def value_targets(self, pre_scorer_embedding, pre_scorer_head, reward_model, mode="mc", draws=10, reduce="mean", alpha=1.0,
                      num_steps=None, eps=1e-5, eval_sp_size=None, want_onehot=True):
        """The training set of one value-function iteration (reference Enformer.py:192-259), built on the device in one pass:
        -> ValueTargets(states u8 [S, B, L], onehot f32 [S B, L, 4] | None, y f32 [S B], x0 int64 [B, L]), rows step-major in the
        reference's torch.cat order: states[k] = mid_x[k] for k < S - 1, states[S - 1] = x_0.
          mode "mc"   (:192-225) the un-guided rollout; y[k B + b] = r(x_0)[b] for every k, the reward evaluated once.
          mode "cdq"  (:226-259) per step i >= 1 the value net on the B * draws candidates drawn from states[i - 1], reduced by
                      svdd_value_target into y[(i - 1) B + b] (which also writes states[i] = the last draw and its one-hot); step 0
                      runs no value net; the last block is r(x_0). reduce "mean" is the reference's sequential fp32 mean, bit for bit
                      given the same scores; "logmeanexp" the soft backup alpha log mean exp(v / alpha) (alpha > 0; an extension).
        One backbone launch per step, no materialised draws, no host round trip. One task only (NotImplementedError otherwise).
        DEPARTURE FROM THE REFERENCE: the targets are evaluated with EVAL-MODE nets (BatchNorm running statistics, dropout off). The
        reference evaluates head(embedding(.)) in whatever mode the module is in - while training that is batch statistics and live
        dropout inside the regression target, which the inference kernels cannot reproduce and nobody wants. embedding / head are put
        into eval() for the call and every submodule's mode is restored afterwards. Their weights may change between calls (they
        are being trained): the weight-validated cache rebuilds the fused net when they do."""
        self._require_gpu()
        if mode not in ("mc", "cdq"):
            raise ValueError(f"mode = {mode!r}: expected 'mc' or 'cdq'")
        if reduce not in ops.TARGET_REDUCE:
            raise ValueError(f"reduce = {reduce!r}: expected 'mean' or 'logmeanexp'")
        if not (float(alpha) > 0.0 and math.isfinite(float(alpha))):
            raise ValueError(f"alpha must be finite and > 0, got {alpha}")
        M = self._check_draws(draws) if mode == "cdq" else 1
        for m in (pre_scorer_embedding, pre_scorer_head, reward_model):
            p = next(m.parameters(), None)
            if p is not None and (not p.is_cuda or p.device != self.device):
                raise ops.SvddError("value_targets: the value and reward nets must be on the model's GPU (the SVDD hot path has no "
                                    "CPU fallback)")
        from .value_nets import ConvHead
        for head in (pre_scorer_head, getattr(reward_model, "head", None)):
            if isinstance(head, ConvHead) and head.channel_transform.conv.layer.out_channels != 1:
                raise NotImplementedError("value_targets: one task only (multi-task heads are out of scope)")
        was = [(sm, sm.training) for m in (pre_scorer_embedding, pre_scorer_head) for sm in m.modules()]
        try:
            pre_scorer_embedding.eval()
            pre_scorer_head.eval()
            return self._value_targets(pre_scorer_embedding, pre_scorer_head, reward_model, M if mode == "cdq" else 0, reduce,
                                       float(alpha), want_onehot, *self._decode_start(num_steps, eps, eval_sp_size))
        finally:
            for sm, training in was:
                sm.training = training

    def _value_targets(self, embedding, head, reward_model, M, reduce, alpha, want_onehot, B, L, S, sched, x):
        """The rollout behind value_targets: M = 0 the un-guided loop (MC), M >= 1 the CD-Q loop with M draws per step."""
        dev = self.device
        states = torch.empty((S, B, L), dtype=torch.uint8, device=dev)
        y = torch.empty((S, B), dtype=torch.float32, device=dev)
        slab = torch.empty((S, B, L, 4), dtype=torch.float32, device=dev) if want_onehot else None
        if M:
            cand = torch.empty((B, M, L), dtype=torch.uint8, device=dev)
            onehot = torch.empty((B * M, L, 4), dtype=torch.float32, device=dev)
        else:
            scratch = torch.empty((B, L, 4), dtype=torch.float32, device=dev)        # propose always writes a one-hot
        x_last = torch.empty((B, L), dtype=torch.uint8, device=dev)                  # the state before the noise removal
        for i in range(S):
            logits = self._prior_logits(x) if i == 0 else self._backbone_logits(x)
            nxt = states[i] if i != S - 1 else x_last
            oh = slab[i] if (want_onehot and i != S - 1) else None
            if M:
                ops.propose(logits, x, sched[i, 2], sched[i, 1], M, self._rng(i, M, B, L, logits), cand=cand, onehot=onehot)
                scores = None
                if i > 0:                                                            # the reference skips time == 0, Enformer.py:233-234
                    scores = self._value_scores(embedding, head, onehot, B, M, cand, x)
                    if scores.numel() != B * M:
                        raise NotImplementedError("value_targets: one task only (the value net returned more than one)")
                self._record(logits, scores, x)
                ops.value_target(scores, cand, reduce, alpha, x_next=nxt, onehot_next=oh, target=y[i - 1] if i > 0 else None)
            else:
                ops.propose(logits, x, sched[i, 2], sched[i, 1], 1, self._rng(i, 1, B, L, logits), cand=nxt.view(B, 1, L),
                            onehot=oh if oh is not None else scratch)
            x = nxt
        x0 = self._noise_removal(x)
        states[S - 1] = x0
        if want_onehot:
            slab[S - 1].copy_(ops.transform_samples(states[S - 1]))
        r = self.reward_callable(reward_model)(ops.transform_samples(states[S - 1], transposed=True))
        if r.dim() < 2 or r.shape[1] != 1 or r.numel() != B:
            raise NotImplementedError(f"value_targets: one task only (the reward model returned {tuple(r.shape)})")
        r = r.reshape(B).float()
        if M:
            y[S - 1] = r
        else:
            y.copy_(r.expand(S, B))
        return ValueTargets(states, slab.view(S * B, L, 4) if want_onehot else None, y.view(S * B), x0)

    def _unguided_sample(self, num_steps, eps, eval_sp_size, keep_mid, x_init=None, t_start=1.0):
        """The un-guided loop -> (x_0 int64, [x_t int64 after every step but the last] if keep_mid else [])."""
        B, L, S, sched, x = self._decode_start(num_steps, eps, eval_sp_size, x_init, t_start)
        mid_x = []
        for i in range(S):
            logits = self._prior_logits(x) if i == 0 else self._backbone_logits(x)
            cand, _, _ = ops.propose(logits, x, sched[i, 2], sched[i, 1], 1, self._rng(i, 1, B, L, logits))
            x = cand.view(B, L)
            if keep_mid and i != S - 1:
                mid_x.append(x.long())
        return self._noise_removal(x), mid_x

    @_decode_scope
    @torch.no_grad()
    def controlled_sample(self, pre_scorer_embedding, pre_scorer_head, num_steps=None, eps=1e-5,
                          eval_sp_size=None, sample_M=10):
        """SVDD-MC decode (:1021-1061): S x [backbone -> propose -> value net -> select], then noise removal."""
        return self._controlled_sample(pre_scorer_embedding, pre_scorer_head, sample_M,
                                       *self._decode_start(num_steps, eps, eval_sp_size))

    def _controlled_sample(self, pre_scorer_embedding, pre_scorer_head, M, B, L, S, sched, x):
        """The SVDD-MC loops from the start state x (the prior, or a caller's state: _decode_start)."""
        cand = torch.empty((B, M, L), dtype=torch.uint8, device=self.device)
        onehot = torch.empty((B * M, L, 4), dtype=torch.float32, device=self.device)
        fn = self.value_callable(pre_scorer_embedding, pre_scorer_head)
        if self._can_skip(fn, L, M):
            return self._controlled_sample_skipping(fn, x, cand, onehot, sched, B, L, S, M)
        if (self.skip_unchanged and self.skip_generic and M > 1 and self.value_batching == "batched" and
                self.select_mode in ("argmax", "multinomial")):
            return self._controlled_sample_generic_skipping(fn, x, cand, onehot, sched, B, L, S, M)
        for i in range(S):
            logits = self._prior_logits(x) if i == 0 else self._backbone_logits(x)
            ops.propose(logits, x, sched[i, 2], sched[i, 1], M, self._rng(i, M, B, L, logits), cand=cand, onehot=onehot)
            scores = self._value_scores(pre_scorer_embedding, pre_scorer_head, onehot, B, M, cand, x)
            self._record(logits, scores, x)
            x = self._select(scores, cand, i)
        return self._noise_removal(x)

    # ------------------------------------------- decoding from a given state: templates and re-mask refinement (ABI 16) ----
    # The per-step updates take any (x, t, dt) and carry every non-MASK token forward (copy_flag, :1199, :1203), and SUBS keeps an
    # unmasked position at the final argmax: a decode may therefore start from ANY state — a template whose open positions are
    # MASK (t_start = 1), or a finished design re-noised to t0 < 1 by q_xt (:738-749) — over linspace(t_start, eps, S + 1). The
    # loops are the samplers' own; only the shortcuts that rely on B identical all-MASK rows are off (_decode_start, _from_state).
    #   replay: a reference-side loop of q_xt + per-step updates draws torch.rand(B, L) for the mask, then the decode's own
    #           uniforms; the generator ends where that loop leaves it. Refused under a batch-sharded run (the mask block is the
    #           batch's own, svdd_refine_remask takes no row slice of a larger block).
    #   philox: the mask is keyed by (philox_seed, row_offset + b, round, position) on stream word 1; the decode of round r uses the
    #           step keys steps_full + r S .. steps_full + (r + 1) S - 1 (steps_full = config.sampling.steps, S = steps per round):
    #           svdd_propose packs the step into the top 16 bits of counter word 2, so every key must stay below 65536, and no
    #           (round, step) of a row shares a key with another — nor with a default-length decode from the prior, whose design
    #           the rounds usually refine.
    def _from_state_checks(self):
        self._require_gpu()
        if self.rng_mode == "replay" and self._shard is not None and self._shard[3] > 1:
            raise ops.SvddError("decoding from a given state in replay mode is not batch-sharded (use rng_mode = 'philox': its "
                                "counters are keyed by the global row)")

    def _move_chance(self, t):
        """1 - exp(-sigma(t)) of ONE t, with the reference's fp32 torch ops on the host (:1725-1729), as _elbo_scalars."""
        sigma, _ = self.noise(torch.tensor([float(t)], dtype=torch.float32))
        return float((1 - torch.exp(-sigma))[0])

    def _mask_rng(self, B, L, round):
        """The Rng of one svdd_refine_remask launch: replay = the next torch.rand(B, L) of the reference's stream (generated on the
        device inside a sampler call, like the decode's own uniforms); philox = (philox_seed, row_offset, round)."""
        if self.rng_mode == "replay":
            if self.replay_rng == "device" and self._scope_depth > 0 and not _capturing():
                if self._replay_stream is None:
                    self._replay_stream = ops.DeviceReplayStream(self.device)
                return ops.Rng(uniforms=self._replay_stream.uniforms(B * L, prefetch=False).view(B, L))
            return ops.Rng(uniforms=torch.rand(B, L).to(self.device, non_blocking=True))
        if self.rng_mode == "philox":
            if not 0 <= int(round) <= 65535:
                raise ops.SvddError(f"round {round}: the Philox counter of svdd_refine_remask holds 16 bits of it")
            return ops.Rng(seed=self.philox_seed, row_offset=self.row_offset, step=int(round))
        raise ValueError(f"rng_mode {self.rng_mode!r}")

    @_decode_scope
    @torch.no_grad()
    def decode_sample_from(self, x_init, t_start=1.0, num_steps=None, eps=1e-5):
        """Un-guided decode from the state x_init [B, L] (tokens 0..3 are kept, 4 = MASK is filled in) at t = t_start -> LongTensor[B, L]."""
        self._from_state_checks()
        return self._unguided_sample(num_steps, eps, None, keep_mid=False, x_init=x_init, t_start=t_start)[0]

    @_decode_scope
    @torch.no_grad()
    def controlled_sample_from(self, x_init, pre_scorer_embedding, pre_scorer_head, t_start=1.0, num_steps=None, eps=1e-5,
                               sample_M=10):
        """SVDD-MC decode from the state x_init [B, L] at t = t_start -> LongTensor[B, L]: the loops of controlled_sample over
        linspace(t_start, eps, S + 1). Every non-MASK token of x_init is in the result (a template: MASK marks the open positions,
        t_start = 1; a re-noised design: renoise(x0, t0), t_start = t0). num_steps None: max(1, ceil(t_start * config.sampling.steps))."""
        self._from_state_checks()
        return self._controlled_sample(pre_scorer_embedding, pre_scorer_head, sample_M,
                                       *self._decode_start(num_steps, eps, None, x_init, t_start))

    @_decode_scope
    @torch.no_grad()
    def renoise(self, x0, t, frozen=None, round=0):
        """q_xt (:738-749) under a frozen mask: x_t = MASK where u < move_chance(t) and frozen == 0, else x0 — one
        svdd_refine_remask launch with the accept step off. x0 [B, L] on the GPU (a MASK token stays MASK), frozen [B, L] (non-zero =
        keep) or None; round keys the Philox draw. -> x_t with x0's dtype."""
        self._from_state_checks()
        if self.time_conditioning:
            raise NotImplementedError("renoise: time-conditioned backbones are not supported")
        self._check_t(t, 0.0, "t")
        x_u8, fz = self._refine_inputs(x0, frozen)
        B, L = x_u8.shape
        xt, _, _ = ops.refine_remask(x_u8, self._move_chance(t), self._mask_rng(B, L, round), frozen=fz)
        return xt if x0.dtype == torch.uint8 else xt.to(x0.dtype)

    def _refine_inputs(self, x0, frozen):
        """(x0 as u8 [B, L], frozen as u8 [B, L] | None), both contiguous on the model's device; CPU tensors and tokens > 4 are
        refused here (one read-back, before the first launch)."""
        for name, t in (("x0", x0), ("frozen", frozen)):
            if t is not None and (not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != self.device):
                raise ops.SvddError(f"{name} must be a tensor on the model's GPU (the SVDD hot path has no CPU fallback)")
        if x0.dim() != 2 or x0.shape[0] == 0 or x0.shape[1] == 0:
            raise ValueError(f"x0 must be [B, L] with B, L > 0, got {tuple(x0.shape)}")
        if x0.dtype.is_floating_point or x0.dtype == torch.bool:
            raise ValueError(f"x0 must hold integer tokens, got {x0.dtype}")
        lo, hi = torch.aminmax(x0)                        # once, at entry: a bad token is refused before any launch (whatever the dtype)
        if int(lo) < 0 or int(hi) > self.mask_index:
            raise ops.SvddError(f"x0 holds a token outside 0..{self.mask_index} (0..3 = A, C, G, T; {self.mask_index} = MASK)")
        if frozen is not None and tuple(frozen.shape) != tuple(x0.shape):
            raise ValueError(f"frozen must have x0's shape {tuple(x0.shape)}, got {tuple(frozen.shape)}")
        fz = None if frozen is None else (frozen != 0).to(torch.uint8).contiguous()
        return self._tokens_u8(x0).contiguous(), fz

    @staticmethod
    def _require_rows(x):
        """The first check of the design entries (ISM, patterns, attributions, Ledidi); no device. -> x's shape (B, L)."""
        if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.shape[0] == 0 or x.shape[1] == 0:
            raise ValueError(f"x must be a [B, L] tensor with B, L > 0, got {tuple(x.shape) if isinstance(x, torch.Tensor) else type(x)}")
        return x.shape

    def _design_scorer(self, pre_scorer_embedding, pre_scorer_head, reward_model):
        """tokens u8 [B, L] -> fp32 [B]: the score refine() judges a finished row by — the value function on the clean tokens, or
        (reward_model given) the reward; task 0 of a multi-task net. One kernel path for every call, so scores compare exactly."""
        if reward_model is None:
            fn = self.value_callable(pre_scorer_embedding, pre_scorer_head)
            opaque = lambda x: fn(ops.transform_samples(x))                                     # noqa: E731
        else:
            fn = self.reward_callable(reward_model)
            opaque = lambda x: fn(ops.transform_samples(x, transposed=True))                    # noqa: E731
        run = fn.forward_tokens if hasattr(fn, "forward_tokens") else opaque
        return lambda x: run(x).reshape(x.shape[0], -1)[:, 0].float().contiguous()

    @_decode_scope
    @torch.no_grad()
    def refine(self, x0, pre_scorer_embedding, pre_scorer_head, rounds, t_renoise, num_steps=None, eps=1e-5, sample_M=10,
               frozen=None, accept="improve", reward_model=None):
        """Test-time refinement of finished designs x0 [B, L]: `rounds` times, re-mask every row at noise level t_renoise (frozen
        positions excepted), decode it again from there with SVDD-MC (controlled_sample_from) and score the result; with accept =
        "improve" a row keeps its new version only if it scores higher than the version it had ("always": the new version is kept).
        The score is the value function on the clean tokens (pre_scorer_head(pre_scorer_embedding(.)), or reward_model's if given.
        Per round: one svdd_refine_remask launch (accept the last round's rows + re-mask), one decode, one scoring pass of B rows;
        no host round trip inside or between rounds. -> (x int64 [B, L], score fp32 [B], stats) with stats = {"accepted": rows
        that took their new version per round, "masked": MASK tokens of the re-masked batch per round}, read once at the end.
        rounds = 0 returns x0 and its score."""
        self._from_state_checks()
        if self.time_conditioning:
            raise NotImplementedError("refine: time-conditioned backbones are not supported")
        if accept not in ("improve", "always"):
            raise ValueError(f"accept = {accept!r}: expected 'improve' or 'always'")
        rounds = int(rounds)
        if rounds < 0:
            raise ValueError(f"rounds must be >= 0, got {rounds}")
        self._check_t(t_renoise, eps, "t_renoise")
        x_keep, fz = self._refine_inputs(x0, frozen)
        x_keep = x_keep.clone()
        B, L = x_keep.shape
        if L != self.config.model.length:
            raise ValueError(f"x0 must be [B, {self.config.model.length}] (config.model.length), got {tuple(x0.shape)}")
        steps_full = int(self.config.sampling.steps)
        S = max(1, math.ceil(float(t_renoise) * steps_full)) if num_steps is None else int(num_steps)
        if S <= 0:
            raise ValueError(f"num_steps must be positive, got {num_steps}")
        if self.rng_mode == "philox" and (rounds > 65536 or steps_full + rounds * S > 65536):
            raise ops.SvddError(f"refine: {rounds} rounds of {S} steps after {steps_full} need Philox step keys beyond 65535 (the "
                                "counter of svdd_propose holds 16 bits of the step)")
        score_fn = self._design_scorer(pre_scorer_embedding, pre_scorer_head, reward_model)
        dev = self.device
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        accepted = torch.zeros((max(rounds, 1), B), dtype=torch.int32, device=dev)
        nmasked = torch.zeros((max(rounds, 1), B), dtype=torch.int32, device=dev)
        score_keep = score_fn(x_keep)                              # the input's score: what round 0's result has to beat
        mc = self._move_chance(t_renoise)
        x_new = score_new = None
        x_t = torch.empty((B, L), dtype=torch.uint8, device=dev)
        base = self._step_base
        try:
            for r in range(rounds):
                rng = self._mask_rng(B, L, r)
                if r == 0:
                    ops.refine_remask(x_keep, mc, rng, frozen=fz, x_t=x_t, nmasked=nmasked[0], err=err)
                else:                                              # accept round r - 1's rows, re-mask what is kept
                    self._refine_boundary(x_new, score_new, x_keep, score_keep, accept, accepted[r - 1], err,
                                          mc=mc, rng=rng, frozen=fz, x_t=x_t, nmasked=nmasked[r])
                self._step_base = base + steps_full + r * S
                out = self._controlled_sample(pre_scorer_embedding, pre_scorer_head, sample_M,
                                              *self._decode_start(S, eps, None, x_t, t_renoise, check_tokens=False))
                x_new = self._tokens_u8(out).contiguous()
                score_new = score_fn(x_new)
        finally:
            self._step_base = base
        if rounds:
            self._refine_boundary(x_new, score_new, x_keep, score_keep, accept, accepted[rounds - 1], err)
        ops.check_refine_err(err)                                   # the one read-back (with the counters below)
        stats = {"rounds": rounds, "steps_per_round": S, "move_chance": mc,
                 "accepted": accepted[:rounds].sum(1).tolist(), "masked": nmasked[:rounds].sum(1).tolist()}
        return x_keep.long(), score_keep, stats

    def _refine_boundary(self, x_new, score_new, x_keep, score_keep, accept, accepted, err, mc=0.0, rng=None, **remask):
        """One svdd_refine_remask launch at a round boundary: x_keep / score_keep (updated in place) take the new row where it is
        accepted; with `remask` arguments the kept rows are re-masked into x_t as well."""
        if accept == "improve":
            ops.refine_remask(x_new, mc, rng, x_old=x_keep, score_new=score_new, score_old=score_keep, x_keep=x_keep,
                              score_keep=score_keep, accepted=accepted, err=err, remask=bool(remask), **remask)
        else:
            ops.refine_remask(x_new, mc, rng, score_new=score_new, x_keep=x_keep, score_keep=score_keep, accepted=accepted,
                              err=err, remask=bool(remask), **remask)

    # ------------------------------------------------------------- in-silico mutagenesis, ISM-driven evolution ----
    ISM_WAVES_PER_CHUNK = 32              # default mutant rows per value-net pass = 32 x the CU count (8192 on MI355X): the [rows, L, 64]
                                          # tower buffer and the GRU's two output planes are 1.26 GB at L = 200
    ISM_COMPARE = (None, "subtract", "divide", "log2FC")

    @dataclass
    class _MutantKind:
        """One kind of mutant scan, built per call (_ism_kind, _pattern_kind): the positions and their chunking, and everything in
        which in-silico mutagenesis and pattern scanning differ. The scan itself (_ScanWorkspace, _scan_pass, _scan_scores,
        _scan_evolve) is written once behind it."""
        pos_dev: torch.Tensor             # i32 [P], ascending
        P: int
        Pc: int                           # positions per chunk: B * per_pos * Pc <= chunk_rows (never less than one position)
        per_pos: int                      # mutants per position: 3 | K
        width: int                        # table entries per position: 4 | K
        copies: bool                      # can a live row's mutant equal the row? (a pattern that is already there; ISM: never)
        trace_key: str                    # the trace's second key: the pick's "allele" | "pattern"
        mutants: object                   # (x, p0, pc, live, cand=, onehot=, err=): ops.ism_mutants | ops.pattern_mutants
        fold: object                      # (scores, parent_score, x, p0, pc, slot=, live=, table=, best=): ops.ism_fold | pattern_fold
        apply: object                     # (best, x, score_cur, ..., stop=, live=, trace=): ops.evolve_apply | pattern_apply
        check_err: object                 # ops.check_ism_err | ops.check_pattern_err
        pat_dev: Optional[torch.Tensor] = None       # patterns only: u8 [K, 32], i32 [K]
        widths_dev: Optional[torch.Tensor] = None

    def _scan_inputs(self, x, positions, chunk_rows, n_pos, per_pos, range_text, mask_text):
        """The checks the two kinds share after the shape's, in an order that needs no device until the last one: the positions
        (None = all n_pos), chunk_rows, a MASK token, then _refine_inputs' (a CPU tensor, a token outside 0..4).
        -> (x u8 [B, L], pos_dev i32 [P], P, Pc)."""
        if positions is None:
            pos = list(range(n_pos))
        else:
            pos = [int(p) for p in (positions.tolist() if isinstance(positions, torch.Tensor) else positions)]
            if not pos:
                raise ValueError("positions must not be empty")
            if any(p < 0 or p >= n_pos for p in pos):
                raise ValueError(f"{range_text}, got {pos}")
            if any(b <= a for a, b in zip(pos, pos[1:])):
                raise ValueError(f"positions must be strictly ascending (no duplicates), got {pos}")
        if chunk_rows is not None and int(chunk_rows) <= 0:
            raise ValueError(f"chunk_rows must be positive, got {chunk_rows}")
        if not x.dtype.is_floating_point and x.dtype != torch.bool and bool((x == self.mask_index).any()):
            raise ops.SvddError(f"x holds a MASK token: {mask_text} (tokens 0..3)")
        x_u8, _ = self._refine_inputs(x, None)
        self._require_gpu()
        if chunk_rows is None:
            chunk_rows = self.ISM_WAVES_PER_CHUNK * torch.cuda.get_device_properties(self.device).multi_processor_count
        Pc = max(1, min(len(pos), int(chunk_rows) // (per_pos * x_u8.shape[0])))
        return x_u8, torch.tensor(pos, dtype=torch.int32, device=self.device), len(pos), Pc

    def _ism_kind(self, x, positions, chunk_rows):
        """ism_scores' / evolve's input checks -> (x u8 [B, L], the kind of the single-base mutants at `positions`)."""
        L = self._require_rows(x)[1]
        x_u8, pos_dev, P, Pc = self._scan_inputs(x, positions, chunk_rows, L, 3, f"positions must lie in 0..{L - 1}",
                                                 "in-silico mutagenesis scores finished sequences")
        return x_u8, self._MutantKind(
            pos_dev, P, Pc, per_pos=3, width=4, copies=False, trace_key="allele",
            mutants=lambda x, p0, pc, live, **out: ops.ism_mutants(x, pos_dev[p0:p0 + pc], live, want_onehot=False, **out),
            fold=lambda sc, parent, x, p0, pc, table=None, **kw: ops.ism_fold(sc, parent, x, pos_dev, p0, pc, ism=table, **kw),
            apply=ops.evolve_apply, check_err=ops.check_ism_err)

    class _ScanWorkspace:
        """The buffers of one scan, sized for a full chunk. The one-hot rows exist only where a kernel reads them (the fp32 windowed
        tower); flags / iota only where copies are told apart (the windowed route; patterns on the whole-mutant route)."""
        def __init__(self, kind, B, L, dev, fused):
            n = B * kind.per_pos * kind.Pc
            self.cand = torch.empty(n * L, dtype=torch.uint8, device=dev)
            self.onehot = self.flags = self.live_idx = self.slot = self.count = self.iota = None
            if fused is not None:
                if not fused.lp_ok(L):
                    self.onehot = torch.empty(n * L * 4, dtype=torch.float32, device=dev)
                self.flags, self.live_idx, self.slot = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
                self.count = torch.zeros(1, dtype=torch.int32, device=dev)
            elif kind.copies:
                self.flags = torch.empty(n, dtype=torch.int32, device=dev)
                self.iota = torch.arange(n, dtype=torch.int32, device=dev)
            self.err = torch.zeros(1, dtype=torch.int32, device=dev)

    def _ism_route(self, pre_scorer_embedding, pre_scorer_head, reward_model, L):
        """(score_fn: tokens u8 [n, L] -> fp32 [n], fused net or None). The fused net is given when the windowed tower applies
        (FusedValueNet, 104 < L <= 208, candidates_ok): the mutants' towers are then computed on their row windows only. Otherwise
        score_fn runs on the mutants' tokens: forward_tokens of a fused net, or the opaque fn(transform_samples(.)) call."""
        from .fused import FusedValueNet
        score_fn = self._design_scorer(pre_scorer_embedding, pre_scorer_head, reward_model)
        fn = (self.value_callable(pre_scorer_embedding, pre_scorer_head) if reward_model is None
              else self.reward_callable(reward_model))
        windowed = isinstance(fn, FusedValueNet) and fn.kernels_ok(L) and fn.candidates_ok(L, 3)
        return score_fn, (fn if windowed else None)

    def _scan_pass(self, kind, x, score_fn, fused, ws, parent_score, live=None, table=None, best=None):
        """The mutants of x at every position, chunk by chunk in ascending position order: kind.mutants, the value net, and kind.fold
        into table [B, P, width] and / or the running best. Copies (a stopped row's mutants; a pattern that is already there) are
        compacted away on the windowed route, and on the whole-mutant route pass through score_fn with the rest, where the fold
        takes the parent's score in a pattern's place; ISM without `live` has none and does neither. Nothing returns to the host."""
        from .fused import candidate_windows
        B, L = x.shape
        if fused is not None:                                       # the parents' tower output, once per pass
            parent_out = fused.parent_tower(x)
        for p0 in range(0, kind.P, kind.Pc):
            pc = min(kind.Pc, kind.P - p0)
            n = B * kind.per_pos * pc
            cand = ws.cand[:n * L].view(B, kind.per_pos * pc, L)
            onehot = None if ws.onehot is None else ws.onehot[:n * L * 4].view(n, L, 4)
            kind.mutants(x, p0, pc, live, cand=cand, onehot=onehot, err=ws.err)
            slot = None
            if fused is None:                                       # whole mutants through score_fn
                if kind.copies:                                     # flags > 0: the mutant differs from its parent
                    candidate_windows(cand, x, flags=ws.flags[:n])
                    slot = torch.where(ws.flags[:n] > 0, ws.iota[:n], ws.iota[:n] - n)
                sc = score_fn(cand.view(n, L))
            else:
                if kind.copies or live is not None:
                    flags, live_idx, slot = ws.flags[:n], ws.live_idx[:n], ws.slot[:n]
                    win = fused.tower_ranges_of(cand, x, key=flags)
                    ops.compact_flags(flags, live_idx, slot, ws.count)
                    sc = fused.forward_candidates_from(onehot, cand, win, parent_out, live_idx=live_idx, count=ws.count)
                else:
                    sc = fused.forward_candidates_from(onehot, cand, fused.tower_ranges_of(cand, x), parent_out)
                sc = sc.reshape(n, -1)
                sc = sc.reshape(n) if sc.shape[1] == 1 else sc[:, 0].contiguous()      # task 0 of a multi-task net
            kind.fold(sc, parent_score, x, p0, pc, slot=slot, live=live, table=table, best=best)

    @staticmethod
    def _compare_to(table, parent_score, compare):
        if compare is None:
            return table
        ref = parent_score[:, None, None]
        return table - ref if compare == "subtract" else table / ref if compare == "divide" else torch.log2(table / ref)

    def _scan_scores(self, x_u8, kind, nets, compare):
        """The table of one scan, fp32 [B, P, kind.width]; nets = (pre_scorer_embedding, pre_scorer_head, reward_model)."""
        B, L = x_u8.shape
        score_fn, fused = self._ism_route(*nets, L)
        ws = self._ScanWorkspace(kind, B, L, self.device, fused)
        parent_score = score_fn(x_u8)
        table = torch.empty((B, kind.P, kind.width), dtype=torch.float32, device=self.device)
        self._scan_pass(kind, x_u8, score_fn, fused, ws, parent_score, table=table)
        kind.check_err(ws.err)
        return self._compare_to(table, parent_score, compare)

    def _scan_evolve(self, x_u8, kind, nets, max_iter, stop):
        """Greedy evolution on one kind's table (evolve's and evolve_patterns' contract): per iteration one pass folded into a
        per-row best and one kind.apply launch; the host reads the one `stopped` word per iteration."""
        x_u8 = x_u8.clone()
        B, L = x_u8.shape
        dev = self.device
        score_fn, fused = self._ism_route(*nets, L)
        ws = self._ScanWorkspace(kind, B, L, dev, fused)
        score_cur = score_fn(x_u8).clone()
        x_best, score_best = x_u8.clone(), score_cur.clone()
        neg = torch.full_like(score_cur, float("-inf"))
        best_so_far = torch.where(score_cur != score_cur, neg, score_cur).max().reshape(1)   # iteration 0 of the reference: the inputs
        stopped = torch.zeros(1, dtype=torch.int32, device=dev)
        live = torch.ones(B, dtype=torch.uint8, device=dev) if stop == "row" else None
        best = (torch.empty(B, device=dev), torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev))
        rows = max(max_iter, 1)
        tr_pos, tr_pick = (torch.full((rows, B), -1, dtype=torch.int32, device=dev) for _ in range(2))
        tr_taken = torch.zeros((rows, B), dtype=torch.uint8, device=dev)
        tr_score = torch.empty((rows + 1, B), dtype=torch.float32, device=dev)
        tr_score[0] = score_cur
        iters = 0
        for it in range(max_iter):
            self._scan_pass(kind, x_u8, score_fn, fused, ws, score_cur, live=live, best=best)
            kind.apply(best, x_u8, score_cur, best_so_far, stopped, x_best, score_best, stop=stop, live=live,
                       trace=(tr_pos[it], tr_pick[it], tr_score[it + 1], tr_taken[it]))
            iters = it + 1
            if int(stopped[0]) != 0:                                # the one word the host reads per iteration
                break
        kind.check_err(ws.err)
        trace = {"iters": iters, "position": tr_pos[:iters], kind.trace_key: tr_pick[:iters], "taken": tr_taken[:iters],
                 "score": tr_score[:iters + 1]}
        return x_best.long(), score_best, trace

    @staticmethod
    def _evolve_args(stop, max_iter):
        if stop not in ops.EVOLVE_STOP:
            raise ValueError(f"stop = {stop!r}: expected 'global' or 'row'")
        if int(max_iter) < 0:
            raise ValueError(f"max_iter must be >= 0, got {int(max_iter)}")
        return int(max_iter)

    @torch.no_grad()
    def ism_scores(self, x, pre_scorer_embedding, pre_scorer_head, reward_model=None, positions=None, compare=None, chunk_rows=None):
        """In-silico mutagenesis (reference score.py ISM_predict): the score of every single-base mutant of x [B, L] (tokens 0..3, on
        the GPU) -> fp32 [B, P, 4]; entry (b, j, a) is the score of row b with base a at positions[j], the entry of the row's own
        base its own score. The score is pre_scorer_head(pre_scorer_embedding(.)), or reward_model's if given (task 0 of a
        multi-task net). positions: None = all, or a strictly ascending list of ints in 0..L-1. compare: None, or "subtract" /
        "divide" / "log2FC" against the parent's score. chunk_rows: mutant rows per value-net pass (whole positions; default 32 x the
        CU count). Per chunk of positions: svdd_ism_mutants, the value net (a fused ConvGRU net at 104 < L <= 208 computes each
        mutant's tower on the row window around its one changed position and copies the rest from the parent's tower output: same
        bits as the whole tower), svdd_ism_fold. No mutant and no score crosses to the host."""
        if compare not in self.ISM_COMPARE:
            raise ValueError(f"compare = {compare!r}: expected None, 'subtract', 'divide' or 'log2FC'")
        x_u8, kind = self._ism_kind(x, positions, chunk_rows)
        return self._scan_scores(x_u8, kind, (pre_scorer_embedding, pre_scorer_head, reward_model), compare)

    @torch.no_grad()
    def evolve(self, x, pre_scorer_embedding, pre_scorer_head, reward_model=None, max_iter=10, positions=None, stop="global",
               chunk_rows=None):
        """Greedy directed evolution on the ISM table (reference design.py evolve(method="ism", for_each=True)): per iteration
        every row's 3 P single-base mutants are scored and the row's best one (the first in (position, allele) order among equal
        scores; a NaN never) is its pick.
          stop = "global"  the reference's rule: every row takes its pick whether or not it improves on the row's score; the run
                           stops at the first iteration whose best pick over the batch does not beat the best seen so far (that
                           iteration changes no row but is in the trace, as in the reference's dataframe).
          stop = "row"     a row takes its pick only if it strictly beats the row's score, otherwise it stops for good (its mutants
                           are not computed again); the run stops at the iteration in which no row moved.
        -> (x_best int64 [B, L], score_best fp32 [B], trace): the highest-scoring state along each row's trajectory (the first one
        among equals) and trace = {"iters": iterations executed (the stopping one included), "position", "allele" (token 0..3),
        "taken": [iters, B] (-1 / -1 / 0: a row without a pick), "score": [iters + 1, B], row 0 the input's scores, row i + 1 the
        picks' scores of iteration i}: the reference dataframe's best_in_iter rows. max_iter = 0 returns the input and its score.
        Per iteration: one pass of ism_scores' path folded into a per-row best, one svdd_evolve_apply launch; the host reads the
        one `stopped` word per iteration and nothing else before the end."""
        max_iter = self._evolve_args(stop, max_iter)
        x_u8, kind = self._ism_kind(x, positions, chunk_rows)
        return self._scan_evolve(x_u8, kind, (pre_scorer_embedding, pre_scorer_head, reward_model), max_iter, stop)

    # ------------------------------------------------------------- pattern scanning, pattern-driven evolution ----
    @staticmethod
    def _pattern_list(patterns):
        """patterns (strings over ACGT and / or integer sequences over 0..3, each of width 1..32) -> (uint8 numpy [K, 32] zero
        padded, int32 numpy [K]). No device."""
        from .motifs import MAX_WIDTH
        if isinstance(patterns, (str, bytes)) or not hasattr(patterns, "__len__"):
            raise ValueError("patterns must be a list of strings over ACGT and / or integer sequences over 0..3")
        if len(patterns) == 0:
            raise ValueError("patterns must not be empty")
        pat, widths = np.zeros((len(patterns), MAX_WIDTH), np.uint8), np.zeros(len(patterns), np.int32)
        for k, p in enumerate(patterns):
            if isinstance(p, str):
                tok = ["ACGT".find(c) for c in p]
                if any(t < 0 for t in tok):
                    raise ValueError(f"patterns[{k}] = {p!r}: a pattern is written over the letters ACGT")
            else:
                arr = np.asarray(p.detach().cpu() if isinstance(p, torch.Tensor) else p)
                if arr.ndim != 1 or (arr.size and arr.dtype.kind not in "iu"):
                    raise ValueError(f"patterns[{k}]: expected a string or a 1-D sequence of integer tokens, got {arr.dtype} {arr.shape}")
                tok = [int(t) for t in arr]
                if any(t < 0 or t > 3 for t in tok):
                    raise ValueError(f"patterns[{k}] holds a token outside 0..3")
            if not 1 <= len(tok) <= MAX_WIDTH:
                raise ValueError(f"patterns[{k}] has width {len(tok)}: a pattern has 1..{MAX_WIDTH} tokens")
            pat[k, :len(tok)], widths[k] = tok, len(tok)
        return pat, widths

    def _pattern_kind(self, x, patterns, reward_model, positions, chunk_rows, what):
        """pattern_scores' / evolve_patterns' input checks: the reward's type, the patterns, the shape, then _scan_inputs' with the
        starts at which the longest pattern fits -> (x u8 [B, L], the kind of the pattern mutants at `positions`)."""
        from .motifs import GuidedReward
        if isinstance(reward_model, GuidedReward):
            raise TypeError(f"{what}: a motifs.GuidedReward is not a net of this route (its motif term scores whole decodes): pass "
                            "the reward model it wraps")
        pat, widths = self._pattern_list(patterns)
        L, K, wmax = self._require_rows(x)[1], len(widths), int(widths.max())
        if wmax > L:
            raise ValueError(f"the longest pattern has {wmax} tokens, the sequences {L}: patterns must fit into the sequence")
        x_u8, pos_dev, P, Pc = self._scan_inputs(
            x, positions, chunk_rows, L - wmax + 1, K,
            f"positions are starts in 0..{L - wmax} (the longest pattern, {wmax} tokens, must fit)",
            "patterns are written into finished sequences")
        pat_dev, widths_dev = torch.from_numpy(pat).to(self.device), torch.from_numpy(widths).to(self.device)
        return x_u8, self._MutantKind(
            pos_dev, P, Pc, per_pos=K, width=K, copies=True, trace_key="pattern", pat_dev=pat_dev, widths_dev=widths_dev,
            mutants=lambda x, p0, pc, live, **out: ops.pattern_mutants(x, pos_dev[p0:p0 + pc], pat_dev, widths_dev, live,
                                                                       want_onehot=False, **out),
            fold=lambda sc, parent, x, p0, pc, **kw: ops.pattern_fold(sc, parent, P, K, p0, pc, **kw),
            apply=lambda best, *state, **kw: ops.pattern_apply(best, pos_dev, pat_dev, widths_dev, *state, **kw),
            check_err=ops.check_pattern_err)

    @torch.no_grad()
    def pattern_scores(self, x, patterns, pre_scorer_embedding, pre_scorer_head, reward_model=None, positions=None, compare=None,
                       chunk_rows=None):
        """Pattern scanning (reference design.py evolve(method="pattern")'s table; grelu's MotifScanDataset restated): the score of
        every row of x [B, L] (tokens 0..3, on the GPU) with each of `patterns` written into it at each start position -> fp32
        [B, P, K]; entry (b, j, k) is the score of row b with x[b, positions[j] : positions[j] + w_k] overwritten by pattern k
        (a replacement: the length stays L). A mutant that equals its parent has the parent's score, the same bits (on the
        windowed route it is not computed). patterns: a list of strings over ACGT and / or integer sequences over 0..3, widths 1..32, possibly different
        (motifs.consensus_patterns gives such a list). positions: None = every start at which the longest pattern fits
        (0 .. L - w_max), or a strictly ascending list of such starts. compare, reward_model: as ism_scores. chunk_rows: mutant rows
        per value-net pass (whole positions, never fewer than one; default 32 x the CU count). Per chunk of positions:
        svdd_pattern_mutants, the value net (a fused ConvGRU net at 104 < L <= 208 computes each mutant's tower on the rows around
        the positions it changed, the same bits as the whole tower), svdd_pattern_fold. No mutant and no score crosses to the host."""
        if compare not in self.ISM_COMPARE:
            raise ValueError(f"compare = {compare!r}: expected None, 'subtract', 'divide' or 'log2FC'")
        x_u8, kind = self._pattern_kind(x, patterns, reward_model, positions, chunk_rows, "pattern_scores")
        return self._scan_scores(x_u8, kind, (pre_scorer_embedding, pre_scorer_head, reward_model), compare)

    @torch.no_grad()
    def evolve_patterns(self, x, patterns, pre_scorer_embedding, pre_scorer_head, reward_model=None, max_iter=10, positions=None,
                        stop="global", chunk_rows=None):
        """Greedy directed evolution on the pattern table (reference design.py evolve(method="pattern", for_each=True)): per
        iteration every row's P K pattern mutants are scored (pattern_scores' path) and the row's best one (the first in (position,
        pattern) order among equal scores; a NaN never) is its pick. A pick may be a no-op: a pattern that is already there, with
        the row's own score.
          stop = "global"  the reference's rule: every row takes its pick whether or not it improves on the row's score; the run
                           stops at the first iteration whose best pick over the batch does not beat the best seen so far (that
                           iteration changes no row but is in the trace).
          stop = "row"     a row takes its pick only if it strictly beats the row's score, otherwise it stops for good (its mutants
                           are not computed again); the run stops at the iteration in which no row moved.
        -> (x_best int64 [B, L], score_best fp32 [B], trace), evolve's contract: the highest-scoring state along each row's
        trajectory (the first among equals) and trace = {"iters", "position" (the pick's start position), "pattern" (index into
        `patterns`), "taken": [iters, B] (-1 / -1 / 0: a row without a pick), "score": [iters + 1, B]}. max_iter = 0 returns the
        input and its score. Per iteration one pass folded into a per-row best and one svdd_pattern_apply launch; the host reads the
        one `stopped` word per iteration and nothing else before the end."""
        max_iter = self._evolve_args(stop, max_iter)
        x_u8, kind = self._pattern_kind(x, patterns, reward_model, positions, chunk_rows, "evolve_patterns")
        return self._scan_evolve(x_u8, kind, (pre_scorer_embedding, pre_scorer_head, reward_model), max_iter, stop)

    # ------------------------------------------------------------- gradient attributions ----
    ATTR_METHODS = ("gradient", "inputxgradient", "integratedgradients")
    ATTR_CHUNK_ROWS = 1024                # default rows per gradient pass: mean_score_input_grad's work buffers (save, gates, out, gout,
                                          # dxg and the seven tower activations) are 1.38 MB per row at L = 200, 1.4 GiB per pass

    @staticmethod
    def _attr_quadrature(n_steps, quadrature):
        """-> (alphas, weights) as float32 numpy arrays [S]. None: Gauss-Legendre on [0, 1] (captum's default rule), computed in
        float64 and rounded once."""
        if quadrature is None:
            node, weight = np.polynomial.legendre.leggauss(int(n_steps))
            return ((1.0 + node) / 2.0).astype(np.float32), (weight / 2.0).astype(np.float32)
        if not isinstance(quadrature, (tuple, list)) or len(quadrature) != 2:
            raise ValueError("quadrature must be None or a pair (alphas, weights)")
        a, w = (torch.as_tensor(q).detach().cpu().double().numpy() for q in quadrature)
        if a.ndim != 1 or w.ndim != 1 or a.size == 0 or a.size != w.size:
            raise ValueError(f"quadrature: alphas and weights must be 1-D of one (non-zero) length, got {a.shape} and {w.shape}")
        return a.astype(np.float32), w.astype(np.float32)

    def _attr_inputs(self, x, method, baseline, n_steps, quadrature, chunk_rows, return_delta):
        """Checks in an order that needs no device until the last one (as _scan_inputs) -> (x u8 [B, L], baseline | None, alphas,
        weights: fp32 device [S], chunk_rows)."""
        B, L = self._require_rows(x)
        if method not in self.ATTR_METHODS:
            raise ValueError(f"method = {method!r}: expected one of {self.ATTR_METHODS}")
        ig = method == "integratedgradients"
        if return_delta and not ig:
            raise ValueError(f"return_delta is the completeness gap of integrated gradients; method = {method!r} has none")
        if baseline is not None:
            if not isinstance(baseline, torch.Tensor) or baseline.dtype != torch.float32:
                raise ValueError(f"baseline must be None or an fp32 tensor, got {getattr(baseline, 'dtype', type(baseline))}")
            if tuple(baseline.shape) not in ((L, 4), (B, L, 4)):
                raise ValueError(f"baseline must be [{L}, 4] or [{B}, {L}, 4], got {tuple(baseline.shape)}")
        if ig:
            if quadrature is None and int(n_steps) <= 0:
                raise ValueError(f"n_steps must be positive, got {n_steps}")
            alphas, weights = self._attr_quadrature(n_steps, quadrature)
        else:
            alphas = weights = np.ones(1, np.float32)               # one pass at the input itself
        if chunk_rows is not None and int(chunk_rows) <= 0:
            raise ValueError(f"chunk_rows must be positive, got {chunk_rows}")
        x_u8, _ = self._refine_inputs(x, None)
        self._require_gpu()
        if baseline is not None:
            if baseline.device != self.device:
                raise ops.SvddError("baseline must be a tensor on the model's GPU (the SVDD hot path has no CPU fallback)")
            baseline = baseline.contiguous()
        dev = self.device
        return (x_u8, baseline, torch.from_numpy(alphas).to(dev), torch.from_numpy(weights).to(dev),
                self.ATTR_CHUNK_ROWS if chunk_rows is None else int(chunk_rows))

    def _attr_route(self, pre_scorer_embedding, pre_scorer_head, reward_model, L):
        """-> (fused net | None, score_fn). fused: the FusedValueNet whose mean_score_input_grad gives the pass's gradient without
        autograd (the reference-shaped ConvGRU net, one task, grad_ok(L): _classifier_fused_value's condition). score_fn: relaxed
        input fp32 [n, L, 4] -> task-0 scores [n], differentiable, always fp32: forward_grad of a fused ConvGRU net at any length its
        kernels take, else the modules themselves (the reward model is fed [n, 4, L], as in _design_scorer) inside
        _gru_backward_ready."""
        from .fused import FusedValueNet
        fn = (self.value_callable(pre_scorer_embedding, pre_scorer_head) if reward_model is None
              else self.reward_callable(reward_model))
        if isinstance(fn, FusedValueNet) and fn.tower_ok and fn.tail_ok and L <= 208 and all(p.numel() for p in fn.wpacks):
            fused = fn if fn.grad_ok(L) and fn.w_eff.shape[1] == 1 else None
            return fused, lambda xin: fn.forward_grad(xin).reshape(xin.shape[0], -1)[:, 0]
        if reward_model is None:
            mods = [m for m in (pre_scorer_embedding, pre_scorer_head) if isinstance(m, nn.Module)]
            run = lambda xin: pre_scorer_head(pre_scorer_embedding(xin))                        # noqa: E731
        else:
            mods = [reward_model] if isinstance(reward_model, nn.Module) else []
            run = lambda xin: reward_model(xin.transpose(1, 2))                                 # noqa: E731

        def score_fn(xin):
            with self._gru_backward_ready(mods, xin.is_cuda):
                s = run(xin).float().reshape(xin.shape[0], -1)[:, 0]
                if not xin.requires_grad:
                    return s
                return s, torch.autograd.grad(s.sum(), xin)[0]      # the backward pass inside the context too
        return None, score_fn

    def attributions(self, x, pre_scorer_embedding, pre_scorer_head, reward_model=None, method="inputxgradient", baseline=None,
                     n_steps=50, quadrature=None, chunk_rows=None, return_delta=False):
        """Per-nucleotide gradient attributions of a row's score (reference score.py get_attributions, the last step of the
        reference's evolution script): x [B, L] tokens 0..4 on the GPU -> fp32 [B, 4, L]. The score is PER ROW, task 0 of
        pre_scorer_head(pre_scorer_embedding(.)), or reward_model's if given (no 1 / B factor, unlike compute_gradient). MASK (4) is
        allowed: its one-hot row is zero, so its input x gradient / IG column is 0 with baseline None.
          method = "gradient"             d score / d onehot: all four bases per position (the hypothetical table)
                   "inputxgradient"       onehot * gradient (the reference script's choice)
                   "integratedgradients"  (onehot - baseline) * sum_k w_k grad(baseline + alpha_k (onehot - baseline))
          baseline    None = zeros (captum's default), or fp32 [L, 4] (shared) / [B, L, 4] (per row); the x input methods multiply by
                      (onehot - baseline)
          quadrature  None = Gauss-Legendre with n_steps nodes on [0, 1] (captum's default; float64 on the host, rounded once to
                      fp32), or a pair (alphas, weights) of equal-length 1-D tensors; n_steps is ignored by the one-pass methods
          chunk_rows  rows per gradient pass (default ATTR_CHUNK_ROWS = 1024: 1.4 GiB of work buffers at L = 200). On the fused route a
                      pass runs on a power-of-two number of rows (the largest <= chunk_rows, at most the next one >= the rows left;
                      the last pass is padded with copies of its first row), so that the 1 / n of mean_score_input_grad's mean is
                      undone exactly: the table does not depend on chunk_rows
          return_delta  (IG only) also the completeness gap per row, sum(attr[b]) - (score(x_b) - score(baseline_b)) fp32 [B]
        The B * S (row, step) pairs run in passes of svdd_attr_path, the gradient, svdd_attr_fold; nothing crosses to the host. The
        fused ConvGRU value net (one task, L = 200 or 50) takes mean_score_input_grad as it is, no autograd; any other net or length
        takes torch autograd of the sum of the pass's scores. The gradient is fp32 whatever self.precision says."""
        _refuse_motif_reward("attributions", pre_scorer_embedding, pre_scorer_head, reward_model)
        x_u8, baseline, alphas, weights, chunk_rows = self._attr_inputs(x, method, baseline, n_steps, quadrature, chunk_rows,
                                                                         return_delta)
        B, L = x_u8.shape
        S = alphas.numel()
        dev = self.device
        fused, score_fn = self._attr_route(pre_scorer_embedding, pre_scorer_head, reward_model, L)
        total = B * S
        cap = 1 << (chunk_rows.bit_length() - 1)                    # the largest power of two <= chunk_rows
        rows_buf = min(cap, 1 << (total - 1).bit_length()) if fused is not None else min(chunk_rows, total)
        path = torch.empty((rows_buf, L, 4), dtype=torch.float32, device=dev)
        acc = torch.empty((B, L, 4), dtype=torch.float32, device=dev)
        attr = torch.empty((B, 4, L), dtype=torch.float32, device=dev)
        rowsum = torch.empty(B, dtype=torch.float32, device=dev) if return_delta else None
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        mode = "gradient" if method == "gradient" else "times_input"
        path_base = baseline if method == "integratedgradients" else None      # the one-pass methods differentiate at the exact one-hot
        r0 = 0
        while r0 < total:
            left = total - r0
            if fused is not None:
                n_pass = min(cap, 1 << (left - 1).bit_length())
                n = min(n_pass, left)
                with torch.no_grad():
                    xin = ops.attr_path(x_u8, alphas, r0, n, path[:n_pass], baseline=path_base, n_pad=n_pass - n, err=err)
                    grad, scale = fused.mean_score_input_grad(xin), float(n_pass)
            else:
                n = min(rows_buf, left)
                with torch.no_grad():
                    ops.attr_path(x_u8, alphas, r0, n, path[:n], baseline=path_base, err=err)
                xin = path[:n].detach().requires_grad_(True)
                with torch.enable_grad():                           # the gradient of the SUM of the pass's scores: scale 1
                    out = score_fn(xin)
                    grad = out[1] if isinstance(out, tuple) else torch.autograd.grad(out.sum(), xin)[0]
                grad, scale = grad.contiguous(), 1.0
            with torch.no_grad():
                ops.attr_fold(grad, scale, weights, x_u8, r0, n, acc, attr, mode=mode, baseline=baseline, rowsum=rowsum)
            r0 += n
        ops.check_attr_err(err)
        if not return_delta:
            return attr
        with torch.no_grad():                                       # score(x) - score(baseline): one forward call on [x; baseline]
            ends = torch.empty((2 * B, L, 4), dtype=torch.float32, device=dev)
            ends[:B] = ops.transform_samples(x_u8)
            ends[B:] = 0.0 if baseline is None else baseline
            sc = score_fn(ends)
            return attr, rowsum - (sc[:B] - sc[B:])

    # ------------------------------------------------------------- Ledidi: gradient-based editing ----
    LEDIDI_BETAS, LEDIDI_ADAM_EPS, LEDIDI_WEIGHT_DECAY = (0.9, 0.999), 1e-8, 0.01      # torch.optim.AdamW's defaults

    def _ledidi_inputs(self, x, max_iter, batch_size, tau, l, lr, eps, early_stopping_iter, positions, target, chunk_rows, check_every,
                       noise):
        """Every check that needs no device, ValueError naming the argument -> (max_iter, S, editable bool list | None, target as a
        float64 numpy [B] | None)."""
        B, L = self._require_rows(x)
        if x.dtype.is_floating_point or x.dtype == torch.bool:
            raise ValueError(f"x must hold integer tokens, got {x.dtype}")
        if L > ops.LEDIDI_MAX_L:
            raise ValueError(f"x has L = {L} positions, beyond the {ops.LEDIDI_MAX_L} svdd_ledidi_step takes")
        S = int(batch_size)
        if not 1 <= S <= ops.LEDIDI_MAX_S:
            raise ValueError(f"batch_size must lie in 1..{ops.LEDIDI_MAX_S}, got {batch_size}")
        max_iter = int(max_iter)
        if not 0 <= max_iter < 2 ** 31 - 1:
            raise ValueError(f"max_iter must lie in 0..{2 ** 31 - 2} (the Philox counter's iteration word and the kernel's int), got {max_iter}")
        for name, val, positive in (("tau", tau, True), ("eps", eps, True), ("lr", lr, False), ("l", l, False)):
            if not math.isfinite(float(val)) or (positive and not float(val) > 0) or float(val) < 0:
                raise ValueError(f"{name} must be a finite number{' > 0' if positive else ' >= 0'}, got {val}")
        if int(early_stopping_iter) < 1:
            raise ValueError(f"early_stopping_iter must be >= 1, got {early_stopping_iter}")
        if int(check_every) < 1:
            raise ValueError(f"check_every must be >= 1, got {check_every}")
        if chunk_rows is not None and int(chunk_rows) <= 0:
            raise ValueError(f"chunk_rows must be positive, got {chunk_rows}")
        editable = None
        if positions is not None:
            pos = [int(p) for p in (positions.tolist() if isinstance(positions, torch.Tensor) else positions)]
            if any(p < 0 or p >= L for p in pos):
                raise ValueError(f"positions must lie in 0..{L - 1}, got {pos}")
            if len(set(pos)) != len(pos):
                raise ValueError(f"positions must not repeat, got {pos}")
            editable = [p in set(pos) for p in range(L)]
        tgt = None
        if target is not None:
            tgt = np.asarray(target.detach().cpu() if isinstance(target, torch.Tensor) else target, dtype=np.float64).reshape(-1)
            if tgt.size not in (1, B) or not np.isfinite(tgt).all():
                raise ValueError(f"target must be a finite float or hold {B} finite values, got {target}")
            tgt = np.broadcast_to(tgt, (B,)).astype(np.float32)
        if noise is not None:
            if not isinstance(noise, torch.Tensor) or noise.dtype != torch.float32 or tuple(noise.shape) != (max_iter + 1, B, S, L, 4):
                raise ValueError(f"noise must be an fp32 tensor of uniforms [{max_iter + 1}, {B}, {S}, {L}, 4] (max_iter + 1, B, "
                                 f"batch_size, L, 4), got {tuple(noise.shape) if isinstance(noise, torch.Tensor) else type(noise)}")
        lo, hi = torch.aminmax(x)
        if int(lo) < 0 or int(hi) > 3:
            raise ValueError("x holds a token outside 0..3: Ledidi edits finished sequences (A, C, G, T; MASK is refused)")
        return max_iter, S, editable, tgt

    def ledidi(self, x, pre_scorer_embedding, pre_scorer_head, reward_model=None, *, max_iter=1000, batch_size=10, tau=1.0, l=0.1,
               lr=1.0, eps=1e-4, early_stopping_iter=100, positions=None, target=None, chunk_rows=None, check_every=32,
               return_trace=False, noise=None):
        """Ledidi (reference design.py ledidi, the `ledidi` package's fit_transform): gradient-based editing of the sequences x [B, L]
        (tokens 0..3 on the GPU) towards a higher score, or with target (a float or [B]) towards that score, with as few edits as
        the weight l asks for. Per design: logit weights w [L, 4] on log(onehot(x) + eps), batch_size Gumbel-softmax samples per
        iteration at temperature tau, straight-through hard samples, total loss = output loss + l * (edits per sample), AdamW(lr) on
        w, the best iteration's samples kept, stop after early_stopping_iter iterations without a lower total loss. The score is
        pre_scorer_head(pre_scorer_embedding(.)), or reward_model's if given (task 0). Designs are independent and stop one by one.
          positions    None = every position may change, or the positions that may (the others are frozen: never sampled)
          chunk_rows   sample rows per scoring / gradient pass (whole designs; default ATTR_CHUNK_ROWS). On the fused route a pass runs
                       on a power-of-two number of rows (padded with copies of its first row), so no result depends on chunk_rows
          check_every  the host reads the one-word live count every check_every iterations; no result depends on it
          noise        None: Philox uniforms keyed by (philox_seed, row_offset + b, iteration, sample, position); or the uniforms
                       themselves, fp32 [max_iter + 1, B, batch_size, L, 4] on the GPU
        Per iteration and chunk of designs: the scores of the hard samples (forward_tokens on a fused net: the bits every other entry
        reports), their input gradient (mean_score_input_grad on the fused one-task ConvGRU net at L = 200 / 50, torch autograd
        otherwise: attributions' routes), one svdd_ledidi_step launch. -> LedidiResult."""
        _refuse_motif_reward("ledidi", pre_scorer_embedding, pre_scorer_head, reward_model)
        max_iter, S, editable, tgt = self._ledidi_inputs(x, max_iter, batch_size, tau, l, lr, eps, early_stopping_iter, positions, target,
                                                         chunk_rows, check_every, noise)
        x0, _ = self._refine_inputs(x, None)
        self._require_gpu()
        dev = self.device
        if noise is not None and noise.device != dev:
            raise ops.SvddError("noise must be a tensor on the model's GPU (the SVDD hot path has no CPU fallback)")
        B, L = x0.shape
        chunk_rows = self.ATTR_CHUNK_ROWS if chunk_rows is None else int(chunk_rows)
        patience, check_every = int(early_stopping_iter), int(check_every)
        fused, grad_fn = self._attr_route(pre_scorer_embedding, pre_scorer_head, reward_model, L)
        score_fn = self._design_scorer(pre_scorer_embedding, pre_scorer_head, reward_model)
        cap = 1 << (chunk_rows.bit_length() - 1) if fused is not None else chunk_rows
        per = max(1, cap // S)                                      # designs per pass: whole designs only, never less than one
        chunks = []
        for d0 in range(0, B, per):
            nd = min(per, B - d0)
            n_pass = 1 << (nd * S - 1).bit_length() if fused is not None else nd * S
            chunks.append((d0, nd, n_pass - nd * S, torch.empty((n_pass, L, 4), dtype=torch.float32, device=dev)))
        with torch.no_grad():
            target_dev = None if tgt is None else torch.from_numpy(tgt).to(dev)
            editable_dev = None if editable is None else torch.tensor(editable, dtype=torch.uint8, device=dev)
            score0 = score_fn(x0)
            # the loss of S copies of the start by the kernel's own formula (a sequential fp32 sum of S equal terms, ONE correctly
            # rounded division), so that an iteration that edits nothing ties with it and is no improvement. On the host in numpy:
            # a device division by a host scalar multiplies by the reciprocal, which is 1 ulp off for a fifth of the values at S = 10
            s0 = score0.cpu().numpy()
            term0 = s0 if tgt is None else (s0 - tgt) * (s0 - tgt)
            acc0 = np.zeros_like(s0)
            with np.errstate(all="ignore"):
                for _ in range(S):
                    acc0 = acc0 + term0
                q0 = acc0 / np.float32(S)
            output0 = torch.from_numpy(q0 if tgt is not None else -q0).to(dev)
            st = ops.LedidiState(x0, S, score0, output0)
            cfg = ops.LedidiConfig(S, tau=tau, l=l, lr=lr, eps=eps, patience=patience, betas=self.LEDIDI_BETAS,
                                   adam_eps=self.LEDIDI_ADAM_EPS, weight_decay=self.LEDIDI_WEIGHT_DECAY)
            sc = torch.empty((B, S), dtype=torch.float32, device=dev)
            err = torch.zeros(1, dtype=torch.int32, device=dev)
            trace = torch.full((max_iter + 1, 3, B), float("nan"), dtype=torch.float32, device=dev) if return_trace else None
            rng_of = lambda it: (ops.Rng(uniforms=noise[it]) if noise is not None                   # noqa: E731
                                 else ops.Rng(seed=self.philox_seed, row_offset=self.row_offset))
            tok_rows, sc_rows = st.tok.view(B * S, L), sc.view(B * S)
            for d0, nd, n_pad, xin in chunks:
                ops.ledidi_step(x0, st, cfg.at(0), xin, d0, nd, 0, rng=rng_of(0), editable=editable_dev, n_pad=n_pad, err=err)
        for i in range(max_iter + 1):
            more = i < max_iter
            for d0, nd, n_pad, xin in chunks:
                r0, r1 = d0 * S, (d0 + nd) * S
                with torch.no_grad():
                    sc_rows[r0:r1] = score_fn(tok_rows[r0:r1])
                if fused is not None:
                    with torch.no_grad():
                        grad, scale = fused.mean_score_input_grad(xin), float(xin.shape[0])
                else:
                    xg = xin.detach().requires_grad_(True)
                    with torch.enable_grad():                       # the gradient of the SUM of the pass's scores: scale 1
                        out = grad_fn(xg)
                        grad = out[1] if isinstance(out, tuple) else torch.autograd.grad(out.sum(), xg)[0]
                    grad, scale = grad.contiguous(), 1.0
                with torch.no_grad():
                    ops.ledidi_step(x0, st, cfg.at(i, scale), xin, d0, nd, i, rng=rng_of(i + 1) if more else None, grad=grad, sc=sc,
                                    target=target_dev, editable=editable_dev, n_pad=n_pad, sample=more,
                                    trace=None if trace is None else (trace[i, 0], trace[i, 1], trace[i, 2]), err=err)
            if (i + 1) % check_every == 0 and int(st.live[0]) == 0:  # the one word the host reads
                break
        ops.check_ledidi_err(err)
        # iterations the longest-running design executed: a stopped design ran best_iter + patience + 1 of them
        ran = torch.where(st.stopped != 0, st.best_iter + (patience + 1), torch.full_like(st.best_iter, max_iter + 1))
        n_iter = int(ran.max())
        if trace is not None:
            trace = trace[:n_iter].permute(0, 2, 1).contiguous()
        return LedidiResult(st.x_best, st.score_best, st.best_total, st.best_output, st.best_input, st.best_iter, n_iter, trace, x0,
                            score0)

    # ------------------------------------------------------------- exact work-skipping ----
    def _can_skip(self, fn, L, M):
        """The skipping paths hand the nets compacted batches whose size only the device knows: they need the
        hand-written kernels for the value / reward net and (PM, logits cache) the one-launch backbone kernel."""
        from .fused import FusedValueNet
        from .fused_trunk import FusedEnformerValueNet
        from .motifs import GuidedReward
        motif_only = isinstance(fn, GuidedReward) and fn.reward_model is None
        if isinstance(fn, GuidedReward):                            # svdd_motif_reward takes a device-side count itself: what matters
            fn = fn.reward_model                                    # is the net the wrapper holds; none at all (a pure motif objective) qualifies
        ok = (motif_only or (isinstance(fn, FusedValueNet) and fn.kernels_ok(L) and fn.w_eff.shape[1] == 1) or
              (isinstance(fn, FusedEnformerValueNet) and fn.head_w.shape[1] == 1))
        return (self.skip_unchanged and self.fuse_nets and self.value_batching == "batched" and M > 1 and ok and
                self.select_mode in ("argmax", "multinomial"))

    def _fused_backbone_or_none(self, L):
        if isinstance(self.backbone, CNNModel) and not self.time_conditioning and self.fuse_nets:
            fb = self._fused_backbone()
            if fb.kernel_ok(L):
                return fb
        return None

    class _SkipWorkspace:
        def __init__(self, B, M, dev):
            i32 = dict(dtype=torch.int32, device=dev)
            self.flags, self.live_idx, self.slot = (torch.empty(B * M, **i32) for _ in range(3))
            self.count3 = torch.zeros(3, **i32)           # [live candidates, of them in the list's first part, in its second] (svdd_compact_by_key split)
            self.count = self.count3[0:1]
            self.row_idx, self.row_slot = torch.empty(B, **i32), torch.empty(B, **i32)
            self.row_count = torch.zeros(1, **i32)
            self.parent_score, self.sel_score = torch.empty(B, device=dev), torch.empty(B, device=dev)
            self.changed, self.idx = torch.empty(B, **i32), torch.empty(B, **i32)
            self.parent_out, self.parent_out_lp, self.seq = None, None, None   # the parents' tower output (FusedValueNet)
            self.M = M
            self.n_live = torch.zeros(1, dtype=torch.int64, device=dev)
            self.n_changed = torch.zeros(1, dtype=torch.int64, device=dev)
            self.late = False                   # set by the sampler per step: the live candidates may exceed one GRU round (FusedValueNet.split_gru_rounds)
            self.late_on_device = False         # ... and the device sizes the two parts (FusedValueNet._late_step), not the host
            self.split_bufs = None              # persistent buffers (+ side stream) of that path
            self.prior_parent_out = None        # the all-MASK row's cached tower output [1, L, 64], where the sampler seeds from it
            self.prior_rows_identical = False   # set by the sampler when x is the prior: the parents' first tower pass runs on one row
            self.n_win_rows = None          # with skip_stats: rows the value net's tower computed (the candidates' row windows; with per-layer
                                            # ranges the FLOP-equivalent number of full-depth rows) ...
            self.n_tile_layers = None       # ... and its 16-row tiles summed over the six layers

    def _select_compact(self, sc, ws, cand, step):
        mode, rng = self._select_args(step)
        x_next, _, _, _ = ops.select_compact(sc, ws.slot, ws.parent_score, cand, mode=mode, rng=rng, sel_score=ws.sel_score,
                                             changed=ws.changed, idx=ws.idx)
        ws.parent_score, ws.sel_score = ws.sel_score, ws.parent_score       # the selected candidate is the next parent
        if ws.parent_out is not None and ws.seq is not None:                # ... and so is its tower output
            ops.advance_rows(ws.seq, ws.slot, ws.idx, ws.parent_out, ws.M)
        if self.skip_stats is not None:
            ws.n_live += ws.count
            ws.n_changed += ws.changed.sum()
        return x_next

    def _dense_scores(self, sc, ws, B, M):
        """[B, M] scores from the compacted ones (only for the trace: the loop itself never materialises them)."""
        live = ws.slot >= 0
        return torch.where(live, sc[ws.slot.clamp(min=0).long()], ws.parent_score.repeat_interleave(M)).view(B, M)

    def _finish_stats(self, ws, B, M, S, kind):
        if self.skip_stats is not None:
            self.skip_stats.update(kind=kind, steps=S, candidates=B * M * S, live_candidates=int(ws.n_live),
                                   row_steps=B * S, changed_row_steps=int(ws.n_changed),
                                   tower_window_rows=None if ws.n_win_rows is None else int(round(float(ws.n_win_rows))),
                                   tower_tile_layers=None if ws.n_tile_layers is None else int(ws.n_tile_layers))

    def _use_logits_cache(self, L):
        """Per-row logits cache of the SVDD-MC skipping loop. "auto": where several sequences share a backbone tile
        (L <= 104) — at L = 200 one workgroup owns one sequence and skipping rows frees CUs but saves no time."""
        return self.logits_cache == "on" or (self.logits_cache == "auto" and 208 // L >= 2)

    def _incremental_stem(self, B, L):
        """(FusedBackbone, its carried-stem state for this decode) where the SVDD-MC skipping loop forwards through
        svdd_backbone_incr2_f32 (see incremental_backbone), else (None, None)."""
        if self.incremental_backbone not in ("auto", "on", "off"):
            raise ValueError(f"incremental_backbone = {self.incremental_backbone!r}: expected 'auto', 'on' or 'off'")
        if self.incremental_backbone == "off" or _capturing():
            return None, None
        fb = self._fused_backbone_or_none(L)
        if fb is None or not fb.incremental_ok(B, L, any_batch=self.incremental_backbone == "on"):
            return None, None
        if self.incremental_items not in ("tight", "aligned"):
            raise ValueError(f"incremental_items = {self.incremental_items!r}: expected 'tight' or 'aligned'")
        return fb, fb.incremental_stem(B, L, self._incremental_depth(fb), tight=self.incremental_items == "tight")

    def _incremental_depth(self, fb):
        """incremental_depth as a number of carried layers of fb: "auto" = INCR_DEPTH_AUTO, held to what the backbone's dilations allow."""
        from .fused import INCR_DEPTH_AUTO, leading_dilation1, following_dilation4
        lead = leading_dilation1(fb.ol_dil)
        most = lead + following_dilation4(fb.ol_dil)
        if self.incremental_depth == "auto":
            return min(max(INCR_DEPTH_AUTO, lead), most)
        try:
            depth = int(self.incremental_depth)
        except (TypeError, ValueError):
            depth = -1
        if not lead <= depth <= most:
            raise ValueError(f"incremental_depth = {self.incremental_depth!r}: expected 'auto' or {lead} .. {most}")
        return depth

    def _controlled_sample_skipping(self, fn, x, cand, onehot, sched, B, L, S, M):
        """SVDD-MC with exact work-skipping (same tokens as the plain loop, bit for bit). 104 < L <= 208 (one sequence per
        tile): the value net's tower also shares the parent's rows (candidate_scores_compact); shorter sequences: the
        live candidates' token rows are gathered into a compact batch and scored whole (forward_tokens)."""
        from .fused import candidate_windows
        ws = self._SkipWorkspace(B, M, self.device)
        if self.skip_stats is not None:
            ws.n_win_rows = torch.zeros(1, dtype=torch.float64, device=self.device)
            ws.n_tile_layers = torch.zeros(1, dtype=torch.int64, device=self.device)
        from .fused import FusedValueNet
        dedup = self._prior_dedup_ok(x) and isinstance(fn, FusedValueNet)   # the parents are B copies of the all-MASK row
        share = hasattr(fn, "candidates_ok") and fn.candidates_ok(L, M)
        if dedup and self.seed_prior:   # that row's score and tower output are constants of the weights: computed once (FusedValueNet.prior_score), broadcast
            ws.parent_score.copy_(fn.prior_score(L, self.mask_index).expand(B))
            ws.prior_parent_out = fn.prior_tower(L, self.mask_index) if share else None
        elif dedup:                     # ... or once per decode, on one row
            ws.parent_score.copy_(fn.forward_tokens(x[:1].contiguous()).reshape(1).expand(B))
        else:
            ws.parent_score.copy_(fn.forward_tokens(x).reshape(B))           # scores of the parents
        ws.prior_rows_identical = dedup                                      # -> the parents' tower output too (candidate_scores_compact)
        fb = self._fused_backbone_or_none(L) if self._use_logits_cache(L) else None
        toks_c = None if share else torch.empty((B * M, L), dtype=torch.uint8, device=self.device)
        logits = None
        inc, stem = (None, None) if fb is not None else self._incremental_stem(B, L)
        if stem is not None:
            stem.stat.zero_()
            stem.forwards = 0
            if self.seed_prior and self._prior_dedup_ok(x):
                # the first forward fills the planes with B copies of what the all-MASK row gives — a constant of the weights, kept
                # by the fused backbone (prior_row): one broadcast launch leaves the stem and the logits as that forward would
                logits = inc.seed_incremental(stem, mask=self.mask_index)
        # the two-part late steps adapt to the decode in hand ON THE DEVICE: every step issues the same launches
        # (FusedValueNet._late_step) and the live counts the compaction leaves there size them — a trained value net, another M or L,
        # another chip change when the live candidates outgrow one GRU round, and a count read back by the host, which runs many
        # steps ahead of the GPU, came too late to say (profiles/prior_seed_late_steps_trace.txt)
        auto_late = share and self.late_steps_from == "auto" and not _capturing() and hasattr(fn, "gru_round_rows")
        ws.late_on_device = auto_late
        for i in range(S):
            if inc is not None:                                               # only the stem tiles the last select's tokens reach
                if i > 0 or not stem.valid:                                   # (step 0 of a seeded stem: its logits are there)
                    logits = inc.forward_incremental(x, stem, out=logits)
            elif fb is None or logits is None:
                logits = self._prior_logits(x) if i == 0 else self._backbone_logits(x)
            else:                                                             # only the rows the last select changed
                ops.compact_flags(ws.changed, ws.row_idx, ws.row_slot, ws.row_count)
                fb.forward_rows(x, count=ws.row_count, out=logits, row_idx=ws.row_idx, scatter=True)
            ops.propose(logits, x, sched[i, 2], sched[i, 1], M, self._rng(i, M, B, L, logits), cand=cand, onehot=onehot)
            if share:
                if auto_late:
                    ws.late = True                                           # every step; the device sizes the second part (often empty)
                else:                                                        # a number: the host-decided form from that fraction of the steps on
                    frac = 0.8 if self.late_steps_from == "auto" else float(self.late_steps_from)
                    ws.late = i >= int(frac * S)                             # late steps: (almost) every candidate is live
                sc = fn.candidate_scores_compact(onehot, cand, x, ws).reshape(-1)
            else:
                candidate_windows(cand, x, margin=0, flags=ws.flags)
                ops.compact_flags(ws.flags, ws.live_idx, ws.slot, ws.count)
                ops.gather_rows(cand.view(B * M, L), ws.live_idx, ws.count, toks_c)
                if getattr(fn, "share_level0", False):                       # the Enformer-shaped trunk: first level on the changed windows only
                    sc = fn.forward_tokens(toks_c, count=ws.count, shared=(x, ws.live_idx, M)).reshape(-1)
                else:
                    sc = fn.forward_tokens(toks_c, count=ws.count).reshape(-1)
            if self.trace is not None or self.state_trace is not None:
                self._record(logits, self._dense_scores(sc, ws, B, M), x)
            x = self._select_compact(sc, ws, cand, i)
        self._finish_stats(ws, B, M, S, "mc")
        if inc is None:
            return self._noise_removal(x)
        if self.config.sampling.noise_removal:
            logits = inc.forward_incremental(x, stem, out=logits)
        if self.skip_stats is not None:                                       # executed work of the carried stem, of what the one-launch kernel runs
            marked = stem.stat.tolist()
            self.skip_stats.update(backbone_stem_tile_layers=marked[0],
                                   backbone_stem_tile_layers_dense=stem.forwards * B * ((L + 15) // 16) * stem.lead,
                                   backbone_deep_tile_layers=marked[1],
                                   backbone_deep_tile_layers_dense=stem.forwards * B * ((L + 15) // 16) * stem.deep)
        return self._noise_removal(x, logits=logits)

    def _controlled_sample_generic_skipping(self, fn, x, cand, onehot, sched, B, L, S, M):
        """SVDD-MC work-skipping for an opaque value function: live candidates gathered into a smaller batch (its size is
        read back once per step), copies take the parent's score (= the score of the candidate selected a step earlier)."""
        from .fused import candidate_windows
        ws = self._SkipWorkspace(B, M, self.device)
        first = fn(ops.transform_samples(x))
        if first.numel() != B:
            raise ops.SvddError("skip_generic needs a single-task value function (one score per candidate); "
                                f"got {tuple(first.shape)} for a batch of {B}")
        ws.parent_score.copy_(first.reshape(B).float())
        sc = torch.zeros(B * M, device=self.device)
        for i in range(S):
            logits = self._prior_logits(x) if i == 0 else self._backbone_logits(x)
            ops.propose(logits, x, sched[i, 2], sched[i, 1], M, self._rng(i, M, B, L, logits), cand=cand, onehot=onehot)
            candidate_windows(cand, x, margin=0, flags=ws.flags)
            ops.compact_flags(ws.flags, ws.live_idx, ws.slot, ws.count)
            k = int(ws.count)                                                 # the one host round trip of the step
            if k:
                # batch sizes in steps of 256 rows (padded with repeats of the first live row): vendor libraries pick and
                # sometimes compile kernels per problem size, and k takes a new value at almost every step
                kp = min(B * M, -(-k // 256) * 256)
                idx = ws.live_idx[:kp].long()
                if kp > k:
                    idx = torch.cat([idx[:k], idx[:1].expand(kp - k)])
                sc[:k] = fn(onehot.index_select(0, idx)).reshape(kp)[:k].float()
            if self.trace is not None or self.state_trace is not None:
                self._record(logits, self._dense_scores(sc, ws, B, M), x)
            x = self._select_compact(sc, ws, cand, i)
        self._finish_stats(ws, B, M, S, "mc-generic")
        return self._noise_removal(x)

    def _tweedie_sample_skipping(self, rf, x, sched, B, L, S, M, fb):
        """SVDD-PM with exact work-skipping: per step ONE backbone forward, on the live candidates only."""
        dev = self.device
        ws = self._SkipWorkspace(B, M, dev)
        n = B * M
        cand = torch.empty((B, M, L), dtype=torch.uint8, device=dev)
        toks_c = torch.empty((n, L), dtype=torch.uint8, device=dev)
        lg_c = torch.empty((n, L, 5), dtype=torch.float32, device=dev)
        from .fused import FusedValueNet
        dedup = self._prior_dedup_ok(x) and isinstance(rf, FusedValueNet)     # the parents are B copies of the all-MASK row
        logits = (fb.forward_rows(x[:1].contiguous()).expand(B, L, self.vocab_size).contiguous() if dedup
                  else fb.forward_rows(x))                                    # parents' logits; advanced, never recomputed
        _, xh = ops.x0hat(logits, x, want_tokens=True, want_onehot=False)
        ws.parent_score.copy_(rf.forward_tokens(xh[:1].contiguous()).reshape(1).expand(B) if dedup
                              else rf.forward_tokens(xh).reshape(B))          # reward of the parents' x0-hat
        from .fused import candidate_windows
        for i in range(S):
            ops.propose(logits, x, sched[i, 2], sched[i, 1], M, self._rng(i, M, B, L, logits), cand=cand)
            candidate_windows(cand, x, margin=0, flags=ws.flags)
            ops.compact_flags(ws.flags, ws.live_idx, ws.slot, ws.count)
            fb.forward_rows(cand.view(n, L), count=ws.count, out=lg_c, row_idx=ws.live_idx, scatter=False)
            ops.gather_rows(cand.view(n, L), ws.live_idx, ws.count, toks_c)
            _, xh = ops.x0hat(lg_c, toks_c, want_tokens=True, want_onehot=False)   # :1415-1419 on the compacted rows
            sc = rf.forward_tokens(xh, count=ws.count).reshape(-1)                 # :1430
            if self.trace is not None or self.state_trace is not None:
                self._record(logits, self._dense_scores(sc, ws, B, M), x)
            x_next = self._select_compact(sc, ws, cand, i)
            ops.advance_rows(lg_c, ws.slot, ws.idx, logits, M)                # the selected candidate's logits are the next parent's
            x = x_next
        self._finish_stats(ws, B, M, S, "pm")
        return self._noise_removal(x, logits)

    @_decode_scope
    @torch.no_grad()
    def controlled_sample_tweedie(self, reward_model, num_steps=None, eps=1e-5, eval_sp_size=None, sample_M=10,
                                  options=True, task="dna"):
        """SVDD-PM decode (:1105-1145). NB the reference compares `options == "True"` (a string, :1414):
        the default `options=True` therefore takes the heuristic branch there too. reward_model may be a motifs.GuidedReward (a
        reward net, or None, plus a motif term): with options="True" it takes the same work-skipping loop."""
        B, L, S, sched, x = self._decode_start(num_steps, eps, eval_sp_size)
        M = sample_M
        rf = self.reward_callable(reward_model)
        fb = self._fused_backbone_or_none(L)
        if options == "True" and task != "rna_saluki" and fb is not None and self._can_skip(rf, L, M):
            return self._tweedie_sample_skipping(rf, x, sched, B, L, S, M, fb)
        for i in range(S):
            logits = self._prior_logits(x) if i == 0 else self._backbone_logits(x)
            cand, _, _ = ops.propose(logits, x, sched[i, 2], sched[i, 1], M, self._rng(i, M, B, L, logits))
            scores = self._tweedie_scores(cand, reward_model, options, task)
            self._record(logits, scores, x)
            x = self._select(scores, cand, i)
        return self._noise_removal(x)

    @_decode_scope
    @torch.no_grad()
    def controlled_sample_TDS(self, reward_model, alpha, num_steps=None, eps=1e-5, eval_sp_size=None, sample_M=10):
        """SMC/TDS baseline decode (:938-978)."""
        B, L, S, sched, x = self._decode_start(num_steps, eps, eval_sp_size)
        carry = self._tds_carry(reward_model, L)
        if carry is not None:
            carry["prior"] = True
        for i in range(S):
            if self.state_trace is not None:
                self.state_trace.append(x.detach().clone())
            x = self._tds_step(x, sched[i, 2], sched[i, 1], reward_model, alpha, i, carry)
        return self._noise_removal(x, carry.get("logits") if carry else None)

    # ------------------------------------------------------------------ ELBO scoring (ABI 13) ----
    # The continuous-time SUBS loss of the reference (diffusion_gosai.py:1660-1669, 738-749, 1709-1779) in its live configuration
    # (T = 0, time_conditioning off, antithetic sampling, no importance sampling / change of variables): for a clean batch x0,
    # draw t, mask x0 with move_chance(t), run the backbone on the masked rows, and weight -log p(x0 | xt) by dsigma / expm1(sigma).
    # svdd_elbo_mask draws the mask and svdd_elbo_nll evaluates the weighted SUBS loss and its sums; the backbone between them is
    # the samplers' own dispatch (_backbone_logits: precision and the DiT apply unchanged).
    #   replay (rng_mode "replay"): the reference's uniforms, from torch's CPU generator in the reference's order (torch.rand(n),
    #           then torch.rand(n, L), per call); the per-row scalars with the reference's fp32 torch ops on the host. Afterwards
    #           the generator is where the reference's call leaves it.
    #   philox: keyed by (philox_seed, row_offset + b, draw k, position), t stratified over each sequence's own draws: a function of
    #           the sequence and its index alone, whatever the chunking or sharding. A repeated call draws the same masks.
    ELBO_WAVES_PER_CHUNK = 32             # default rows per backbone launch = 32 x the CU count (8192 on MI355X): whole waves of workgroups

    def _elbo_checks(self, x0):
        """The configurations the ELBO path covers; -> x0 as u8 on the model's device."""
        self._require_gpu()
        tr = self.config.training
        if self.time_conditioning:
            raise NotImplementedError("ELBO scoring: time-conditioned backbones are not supported (the fused backbone runs at sigma = 0)")
        if self.T > 0:
            raise NotImplementedError("ELBO scoring: only the continuous-time loss (T = 0) is supported, not the discrete-time "
                                      "D3PM loss (diffusion_gosai.py:1713-1718, 1738-1746)")
        if getattr(tr, "importance_sampling", False) or getattr(tr, "change_of_variables", False):
            raise NotImplementedError("ELBO scoring: importance_sampling and change_of_variables are not supported")
        if not isinstance(x0, torch.Tensor) or not x0.is_cuda:
            raise ops.SvddError("x0 must be a GPU tensor (the ELBO path has no CPU fallback)")
        if x0.dim() != 2 or x0.shape[0] == 0 or x0.shape[1] == 0:
            raise ValueError(f"x0 must be [n, L] with n, L > 0, got {tuple(x0.shape)}")
        if x0.dtype != torch.uint8:
            lo, hi = torch.aminmax(x0)
            if int(lo) < 0 or int(hi) > 255:
                raise ops.SvddError("x0 holds a token outside 0..3")
            x0 = x0.to(torch.uint8)
        return x0.to(self.device).contiguous()

    def _elbo_scalars(self, e):
        """(t, sigma, dsigma, move_chance [n, 1], w) from the uniforms e = torch.rand(n), with the reference's fp32 torch ops on
        the CPU: _sample_t (:1660-1669), noise(t) and move_chance (:1725-1729), w = dsigma / expm1(sigma) (:1757)."""
        n = e.shape[0]
        if self.config.training.antithetic_sampling:
            offset = torch.arange(n, device=e.device) / n
            e = (e / n + offset) % 1
        t = (1 - self.sampling_eps) * e + self.sampling_eps
        sigma, dsigma = self.noise(t)
        move_chance = 1 - torch.exp(-sigma[:, None])
        return t, sigma, dsigma, move_chance, dsigma / torch.expm1(sigma)

    def _elbo_chunk_rows(self, chunk_rows):
        if chunk_rows is None:
            return self.ELBO_WAVES_PER_CHUNK * torch.cuda.get_device_properties(self.device).multi_processor_count
        if int(chunk_rows) <= 0:
            raise ValueError(f"chunk_rows must be positive, got {chunk_rows}")
        return int(chunk_rows)

    def _elbo_rows(self, xt, x0, w, K, want_tokens, want_mean, err):
        """One backbone launch on the masked rows xt [n K, L] and svdd_elbo_nll -> (nll | None, row_sum, seq_mean | None)."""
        return ops.elbo_nll(self._backbone_logits(xt), xt, x0, w, K, want_tokens=want_tokens, want_mean=want_mean, err=err)

    def _replay_draw(self, x0_u8, chunk, want_tokens, err):
        """One _forward_pass_diffusion of the reference in replay mode, over row chunks -> (nll [n, L] | None, row_sum [n])."""
        n, L = x0_u8.shape
        dev = x0_u8.device
        t, sigma, dsigma, mc, w = self._elbo_scalars(torch.rand(n))          # the reference's first draw
        u = torch.rand(n, L)                                                   # ... and its second (q_xt)
        mc_d, w_d = mc.view(-1).to(dev), w.to(dev)
        nll = torch.empty((n, L), dtype=torch.float32, device=dev) if want_tokens else None
        row_sum = torch.empty(n, dtype=torch.float64, device=dev)
        xt_all = torch.empty((n, L), dtype=torch.uint8, device=dev) if self.elbo_trace is not None else None
        for s0 in range(0, n, chunk):
            s1 = min(n, s0 + chunk)
            xt, *_ = ops.elbo_mask(x0_u8[s0:s1], 1, ops.Rng(uniforms=u[s0:s1].to(dev, non_blocking=True)), move_chance=mc_d[s0:s1])
            tok, rs, _ = self._elbo_rows(xt, x0_u8[s0:s1], w_d[s0:s1], 1, want_tokens, False, err)
            row_sum[s0:s1] = rs
            if want_tokens:
                nll[s0:s1] = tok
            if xt_all is not None:
                xt_all[s0:s1] = xt
        if self.elbo_trace is not None:
            self.elbo_trace.append(dict(t=t, sigma=sigma, dsigma=dsigma, move_chance=mc, w=w, xt=xt_all))
        return nll, row_sum

    @_decode_scope
    @torch.no_grad()
    def _sample_t(self, n, device):
        """t of the ELBO (:1660-1669): uniforms from torch's CPU generator (the reference's stream), antithetic offsets, fp32 ops on
        the host -> t fp32 [n] on `device`."""
        return self._elbo_scalars(torch.rand(n))[0].to(device)

    @_decode_scope
    @torch.no_grad()
    def q_xt(self, x, move_chance):
        """xt = where(torch.rand(*x.shape) < move_chance, MASK, x) (:738-749): the uniforms from torch's CPU generator, the compare
        and the masking in svdd_elbo_mask. move_chance fp32 [n, 1] or [n]; -> xt [n, L] with x's dtype, on the GPU."""
        self._require_gpu()
        x_u8 = self._elbo_checks(x)
        n, L = x_u8.shape
        u = torch.rand(n, L).to(x_u8.device)
        mc = move_chance.detach().float().reshape(-1).to(x_u8.device)
        xt, *_ = ops.elbo_mask(x_u8, 1, ops.Rng(uniforms=u), move_chance=mc.expand(n).contiguous() if mc.numel() == 1 else mc)
        return xt if x.dtype == torch.uint8 else xt.to(x.dtype)

    @_decode_scope
    @torch.no_grad()
    def _forward_pass_diffusion(self, x0):
        """The SUBS continuous-time loss of every token (:1709-1757): -log p(x0 | xt) * dsigma / expm1(sigma) where xt is masked,
        0 elsewhere -> fp32 [n, L]. Replay: the reference's draws (t, then the mask uniforms) from torch's CPU generator; Philox:
        svdd_elbo_mask with one draw per row, keyed by (philox_seed, row_offset + b)."""
        x0_u8 = self._elbo_checks(x0)
        chunk = self._elbo_chunk_rows(None)
        err = torch.zeros(1, dtype=torch.int32, device=x0_u8.device)
        if self.rng_mode == "replay":
            nll, _ = self._replay_draw(x0_u8, chunk, True, err)
        elif self.rng_mode == "philox":
            n, L = x0_u8.shape
            nll = torch.empty((n, L), dtype=torch.float32, device=x0_u8.device)
            for s0 in range(0, n, chunk):
                s1 = min(n, s0 + chunk)
                xt, t, mc, w, _ = ops.elbo_mask(x0_u8[s0:s1], 1, ops.Rng(seed=self.philox_seed, row_offset=self.row_offset + s0),
                                                eps=self.sampling_eps)
                nll[s0:s1] = self._elbo_rows(xt, x0_u8[s0:s1], w, 1, True, False, err)[0]
                if self.elbo_trace is not None:
                    self.elbo_trace.append(dict(t=t, move_chance=mc, w=w, xt=xt))
        else:
            raise ValueError(f"rng_mode {self.rng_mode!r}")
        ops.check_elbo_err(err)
        return nll

    @_decode_scope
    @torch.no_grad()
    def _loss(self, x0, attention_mask):
        """The reference's _loss for the diffusion parameterizations (:1759-1779) -> Loss(loss = sum(nlls) / count, nlls = loss *
        attention_mask, token_mask = attention_mask). attention_mask None fails like the reference (loss * None)."""
        if x0.shape[1] > self.config.model.length:
            raise NotImplementedError("Sub-sampling not implemented")                       # _maybe_sub_sample, :1681-1683
        loss = self._forward_pass_diffusion(x0)
        nlls = loss * attention_mask
        count = attention_mask.sum()
        token_nll = nlls.sum() / count
        return Loss(loss=token_nll, nlls=nlls, token_mask=attention_mask)

    @_decode_scope
    @torch.no_grad()
    def sequence_nll(self, x0, n_draws=1, chunk_rows=None):
        """ELBO estimate of -log p(x0) per sequence, in nats: fp64 [n], the mean over n_draws draws of the sum over positions of
        the token loss. Replay: n_draws consecutive _forward_pass_diffusion calls of the reference (each draws t for the whole
        batch, antithetic over its rows). Philox: the draws of a sequence are stratified over its own n_draws (t of draw k in the
        k-th of n_draws equal slices of (eps, 1]), so the value of a sequence depends on its tokens, philox_seed and row_offset +
        its index only. chunk_rows: rows per backbone launch (default 32 x the CU count; Philox: whole sequences with all their
        draws, so n_draws <= chunk_rows)."""
        x0_u8 = self._elbo_checks(x0)
        K = int(n_draws)
        if K <= 0:
            raise ValueError(f"n_draws must be positive, got {n_draws}")
        chunk = self._elbo_chunk_rows(chunk_rows)
        n, L = x0_u8.shape
        dev = x0_u8.device
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        if self.rng_mode == "replay":
            rows = [self._replay_draw(x0_u8, chunk, False, err)[1] for _ in range(K)]
            acc = rows[0].clone()
            for r in rows[1:]:
                acc += r                                                     # draw order, as svdd_elbo_nll's seq_mean
            out = acc / K
        elif self.rng_mode == "philox":
            if K > chunk:
                raise ValueError(f"n_draws ({K}) > chunk_rows ({chunk}): the draws of a sequence go through one backbone launch")
            per = chunk // K
            out = torch.empty(n, dtype=torch.float64, device=dev)
            for s0 in range(0, n, per):
                s1 = min(n, s0 + per)
                xc = x0_u8[s0:s1]
                xt, _, _, w, _ = ops.elbo_mask(xc, K, ops.Rng(seed=self.philox_seed, row_offset=self.row_offset + s0), eps=self.sampling_eps)
                out[s0:s1] = self._elbo_rows(xt, xc, w, K, False, True, err)[2]
        else:
            raise ValueError(f"rng_mode {self.rng_mode!r}")
        ops.check_elbo_err(err)
        return out

    def nll_metrics(self, x0, n_draws=1, chunk_rows=None):
        """The reference's test metrics (:50-71, 128-133), per token, in float64: nll = sum of the token losses / token count,
        bpd = nll / ln 2, ppl = exp(nll). With n_draws > 1 the token losses are averaged over the draws."""
        seq = self.sequence_nll(x0, n_draws=n_draws, chunk_rows=chunk_rows)
        nll = float(seq.sum()) / (seq.numel() * x0.shape[1])
        return {"nll": nll, "bpd": nll / math.log(2), "ppl": math.exp(nll)}
