"""Decode harness — mirror of the reference's `Enformer.BaseModel.controlled_decode*`
(reference Enformer.py:399-477, 479-557, 560-637, 639-716, 719-813) for the SVDD decode path.

The reference's `BaseModel.__init__` hard-wires checkpoint paths, Hydra and `.cuda()`
(Enformer.py:75-131); there are no checkpoints offline, so here the three nets are passed in:

    BaseModel(embedding, head, ref_model, reward_model, batch_size, task="dna", n_tasks=1)

`controlled_decode*` keep the reference's call order (guided batches first, then
`gen_batch_num * sample_M` un-guided baseline batches, then the top-k) and return the same
5-tuple: (samples list, value_func_preds [N], reward_model_preds [N], top_k_values, baseline_preds [N]).
The tokens of the baseline batches behind baseline_preds are kept in `baseline_samples`; `evaluate_nll` scores any of them
under the pretrained model (Diffusion.sequence_nll); `evaluate_quality` reports set-level metrics of them (svdd_amd.quality),
`evaluate_motifs` their motif content (svdd_amd.motifs); `select_library` picks the best of them that are no near copies of each other.
"""
import torch
from torch import nn

_M64 = (1 << 64) - 1


def batch_seed(base, k):
    """64-bit Philox key of batch k of a harness call whose model carries philox_seed = base: splitmix64 of
    (base, k). `base + k` would make batch k + 1 of seed s the same decode as batch k of seed s + 1, so runs at seeds
    0, 1, 2, ... would share all but one of their batches and understate the run-to-run variance."""
    z = (int(base) + 0x9E3779B97F4A7C15 * (int(k) + 1)) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


class BaseModel(nn.Module):
    def __init__(self, embedding, head, ref_model, reward_model, batch_size, task="dna", n_tasks=1,
                 val_batch_num=0, cdq=False, cdq_alpha=None):
        super().__init__()
        self.cdq = bool(cdq)                      # training: CD-Q targets (Enformer.py:226-259) instead of Monte-Carlo ones (:192-225)
        self.cdq_alpha = cdq_alpha                # None: the reference's mean over the draws; a number: alpha log mean exp(v / alpha)
        self.cdq_draws = 10                       # the reference's `for j in range(10)`, diffusion_gosai.py:846
        self.timed = False                        # time-conditioned value nets (Enformer.py:204-214) are not supported
        self.loss_fct = nn.MSELoss()
        self.task = task
        self.n_tasks = n_tasks
        self.embedding = embedding
        self.head = head
        self.ref_model = ref_model.eval()
        self.reward_model = reward_model.eval()
        for m in (self.ref_model, self.reward_model):
            for p in m.parameters():
                p.requires_grad_(False)
        self.NUM_SAMPLES_PER_BATCH = batch_size
        self.val_data_num = val_batch_num * batch_size
        if task == "rna_saluki":
            raise NotImplementedError("rna_saluki needs a data file the reference hard-codes by absolute path")
        # The reference pre-samples val_batch_num batches here to build value-fn eval data
        # (Enformer.py:135-160), which advances the global RNG before any decode; kept for stream parity.
        self.eval_time_step_batches, self.eval_time_step_targets = [], []
        if val_batch_num > 0:
            self._presample(val_batch_num)

    @torch.no_grad()
    def _presample(self, val_batch_num):
        steps = self.ref_model.config.sampling.steps
        per_t_samples = [[] for _ in range(steps)]
        per_t_targets = [[] for _ in range(steps)]
        for _ in range(val_batch_num):
            samples, mid = self.ref_model._sample(eval_sp_size=self.NUM_SAMPLES_PER_BATCH)
            target = self._reward(samples)
            for j, s in enumerate(mid + [samples]):
                per_t_samples[j].append(self.transform_samples(s))
                per_t_targets[j].append(target)
        self.eval_time_step_batches = [torch.cat(s, dim=0) for s in per_t_samples]
        self.eval_time_step_targets = [torch.cat(t, dim=0) for t in per_t_targets]

    def train(self, mode=True):
        """nn.Module.train would flip every child: the frozen nets (ref_model, reward_model) stay in eval mode, so that they never
        pick up dropout or batch statistics (the reference calls .eval() on them once and never trains the wrapper around them
        in another mode, Enformer.py:97-133)."""
        super().train(mode)
        self.ref_model.eval()
        self.reward_model.eval()
        return self

    def forward(self, x0=None, y=None):
        """The value function's loss (reference Enformer.py:163-267).
          training, not cdq  Monte-Carlo regression (:192-225): every state of an un-guided rollout is regressed onto r(x_0).
          training, cdq      CD-Q (:226-259): every state is regressed onto the mean (cdq_alpha: the soft log-mean-exp) of the value
                             net's own predictions on cdq_draws next states; the last state onto r(x_0).
          otherwise          loss_fct(head(embedding(x0)).view(-1), y.view(-1)) on the caller's batch (:260-265).
        The training set comes from ref_model.value_targets (one pass on the device, targets from EVAL-mode nets: see there); the
        loss itself runs the torch modules in their own (train) mode under autograd, as in the reference. Philox mode: the rollout is
        a function of ref_model.philox_seed - advance it between iterations."""
        if not self.training:
            return self.loss_fct(self.head(self.embedding(x0)).view(-1), y.view(-1))
        if self.timed:
            raise NotImplementedError("time-conditioned value nets (Enformer.py:204-214) are not supported")
        if self.n_tasks != 1:
            raise NotImplementedError("value-function training: one task only")
        vt = self.ref_model.value_targets(self.embedding, self.head, self.reward_model, mode="cdq" if self.cdq else "mc",
                                          draws=self.cdq_draws, reduce="mean" if self.cdq_alpha is None else "logmeanexp",
                                          alpha=1.0 if self.cdq_alpha is None else self.cdq_alpha,
                                          eval_sp_size=self.NUM_SAMPLES_PER_BATCH)
        self.last_targets = vt
        return self.loss_fct(self.head(self.embedding(vt.onehot)).view(-1), vt.y.view(-1))

    def transform_samples(self, samples, num_classes=4):
        return self.ref_model.transform_samples(samples, num_classes)        # Enformer.py:269-277

    def _reward(self, tokens):
        """reward_model(onehot.float().transpose(1, 2)) with the n_tasks convention of Enformer.py:446-449."""
        onehot = self.transform_samples(tokens).float().transpose(1, 2)
        pred = self.reward_model(onehot).detach()
        return pred[:, 0] if self.n_tasks == 1 else pred

    def _value(self, tokens):
        onehot = self.transform_samples(tokens).float()
        return self.head(self.embedding(onehot)).squeeze(2).detach()          # Enformer.py:443

    def _next_batch_seed(self):
        """Philox mode: the sampler is a pure function of (philox_seed, row, step), so consecutive batches would be
        copies of each other; the reference's batches differ because they share torch's global generator
        (Enformer.py:439-467). Batch k of a harness call therefore gets the key batch_seed(base, k) (deterministic given
        the model's philox_seed at entry, and never shared between different entry seeds); replay mode keeps drawing
        from the global generator like the reference."""
        m = self.ref_model
        if getattr(m, "rng_mode", "replay") == "philox":
            m.philox_seed = batch_seed(self._seed_base, self._batch_index)
        self._batch_index += 1

    def _decode(self, gen_batch_num, sample_M, guided, tweedie_quirks=False):
        self._seed_base, self._batch_index = int(getattr(self.ref_model, "philox_seed", 0)), 0
        try:
            return self._decode_inner(gen_batch_num, sample_M, guided, tweedie_quirks)
        finally:
            if hasattr(self.ref_model, "philox_seed"):
                self.ref_model.philox_seed = self._seed_base

    def _decode_inner(self, gen_batch_num, sample_M, guided, tweedie_quirks=False):
        """`tweedie_quirks`: what `controlled_decode_tweedie` does differently from its three siblings (pinned by
        tests/golden/g22_harness.npz, recorded from the reference's own method): `samples.extend(batch)` — a flat list of
        [L] rows instead of a list of [B, L] batches (Enformer.py:766 vs :441) — and `top_k_values = cat(baseline_preds)`,
        the top-k being commented out there (:802-811)."""
        samples, value_func_preds, reward_model_preds = [], [], []
        self.baseline_samples = []                                            # the batches behind baseline_preds (evaluate_nll)
        for _ in range(gen_batch_num):
            self._next_batch_seed()
            batch = guided()
            if tweedie_quirks:
                samples.extend(batch)
            else:
                samples.append(batch)
            value_func_preds.extend(self._value(batch))
            reward_model_preds.extend(self._reward(batch))
        print("Value-weighted sampling done.")
        baseline_preds, all_preds = [], []
        for i in range(gen_batch_num * sample_M):                             # Enformer.py:456-467
            self._next_batch_seed()
            batch = self.ref_model.decode_sample(eval_sp_size=self.NUM_SAMPLES_PER_BATCH)
            pred = self._reward(batch)
            if i < gen_batch_num:
                baseline_preds.extend(pred)
                self.baseline_samples.append(batch)
            all_preds.extend(pred)
        if tweedie_quirks:
            top_k_values = torch.cat(baseline_preds)                           # Enformer.py:802
        else:
            print("Baseline sampling done.")
            all_values = torch.cat(all_preds)
            k = int(len(all_values) / sample_M)                                # Enformer.py:471-475
            top_k_values, _ = torch.topk(all_values, k)
        return (samples, torch.cat(value_func_preds), torch.cat(reward_model_preds), top_k_values,
                torch.cat(baseline_preds))

    @torch.no_grad()
    def controlled_decode(self, gen_batch_num, sample_M):
        """SVDD-MC (reference Enformer.py:399-477)."""
        return self._decode(gen_batch_num, sample_M, lambda: self.ref_model.controlled_sample(
            self.embedding, self.head, eval_sp_size=self.NUM_SAMPLES_PER_BATCH, sample_M=sample_M))

    @torch.no_grad()
    def controlled_decode_refine(self, gen_batch_num, sample_M, rounds, t_renoise, frozen=None):
        """SVDD-MC followed by `rounds` rounds of re-mask refinement at noise level t_renoise (Diffusion.refine, accept = "improve";
        no reference counterpart): every guided batch is decoded like controlled_decode's, then refined under the same Philox key
        (the rounds use step keys of their own). frozen [NUM_SAMPLES_PER_BATCH, L] or None: positions no round re-masks. Returns
        what controlled_decode returns; `refine_stats` holds the per-batch stats of Diffusion.refine."""
        m = self.ref_model
        self.refine_stats = []

        def guided():
            x = m.controlled_sample(self.embedding, self.head, eval_sp_size=self.NUM_SAMPLES_PER_BATCH, sample_M=sample_M)
            x, _, stats = m.refine(x, self.embedding, self.head, rounds, t_renoise, sample_M=sample_M, frozen=frozen)
            self.refine_stats.append(stats)
            return x
        return self._decode(gen_batch_num, sample_M, guided)

    @torch.no_grad()
    def ism_predict(self, samples, positions=None, compare=None):
        """In-silico mutagenesis of finished designs under the harness's reward model (reference score.py ISM_predict): samples
        [B, L] tokens 0..3 -> fp32 [B, P, 4], the reward of every single-base mutant (Diffusion.ism_scores)."""
        return self.ref_model.ism_scores(samples, self.embedding, self.head, reward_model=self.reward_model, positions=positions,
                                         compare=compare)

    @torch.no_grad()
    def evolve(self, samples, max_iter=10, positions=None, stop="global"):
        """ISM-driven directed evolution of samples [B, L] under the harness's reward model (reference design.py evolve(method="ism",
        for_each=True); Diffusion.evolve) -> (x_best int64 [B, L], score_best fp32 [B], trace)."""
        return self.ref_model.evolve(samples, self.embedding, self.head, reward_model=self.reward_model, max_iter=max_iter,
                                     positions=positions, stop=stop)

    @torch.no_grad()
    def pattern_scan(self, samples, patterns, positions=None, compare=None):
        """What each of `patterns` is worth at each start position of finished designs under the harness's reward model (reference
        design.py evolve(method="pattern")'s table): samples [B, L] tokens 0..3 -> fp32 [B, P, K] (Diffusion.pattern_scores)."""
        return self.ref_model.pattern_scores(samples, patterns, self.embedding, self.head, reward_model=self.reward_model,
                                             positions=positions, compare=compare)

    @torch.no_grad()
    def evolve_patterns(self, samples, patterns, max_iter=10, positions=None, stop="global"):
        """Pattern-driven directed evolution of samples [B, L] under the harness's reward model (reference design.py
        evolve(method="pattern", for_each=True); Diffusion.evolve_patterns) -> (x_best int64 [B, L], score_best fp32 [B], trace)."""
        return self.ref_model.evolve_patterns(samples, patterns, self.embedding, self.head, reward_model=self.reward_model,
                                              max_iter=max_iter, positions=positions, stop=stop)

    def get_attributions(self, samples, method="inputxgradient", **kw):
        """Per-nucleotide attributions of samples [B, L] under the harness's reward model (reference score.py get_attributions;
        Diffusion.attributions: method "gradient" / "inputxgradient" / "integratedgradients", baseline, n_steps, quadrature,
        chunk_rows, return_delta) -> fp32 [B, 4, L]."""
        return self.ref_model.attributions(samples, self.embedding, self.head, reward_model=self.reward_model, method=method, **kw)

    def ledidi(self, samples, **kw):
        """Ledidi gradient-based editing of samples [B, L] under the harness's reward model (reference design.py ledidi;
        Diffusion.ledidi's keyword arguments) -> (tokens u8 [B, L], scores fp32 [B], edits int64 [B], report): each design's best
        sample by its own objective (design_pick) and report = {"ledidi_score_gain_mean": mean of score - start score,
        "ledidi_edits_mean", "ledidi_improved_fraction": designs whose total loss fell below the start's, "ledidi_iters"}."""
        from .diffusion import design_pick
        res = self.ref_model.ledidi(samples, self.embedding, self.head, reward_model=self.reward_model, **kw)
        tokens, scores, edits = design_pick(res, kw.get("target"))
        report = {"ledidi_score_gain_mean": float((scores - res.score0).mean()), "ledidi_edits_mean": float(edits.float().mean()),
                  "ledidi_improved_fraction": float((res.best_iter >= 0).float().mean()), "ledidi_iters": res.n_iter}
        return tokens, scores, edits, report

    @torch.no_grad()
    def controlled_decode_tweedie(self, gen_batch_num, sample_M, options):
        """SVDD-PM (reference Enformer.py:719-813)."""
        return self._decode(gen_batch_num, sample_M, lambda: self.ref_model.controlled_sample_tweedie(
            self.reward_model, eval_sp_size=self.NUM_SAMPLES_PER_BATCH, sample_M=sample_M, options=options,
            task=self.task), tweedie_quirks=True)

    @torch.no_grad()
    def controlled_decode_motif(self, gen_batch_num, sample_M, motif_reward, options="True"):
        """SVDD-PM towards (or away from) motifs (svdd_amd.motifs; not in the reference): every guided batch is decoded
        under GuidedReward(self.reward_model, motif_reward), the reward net's score plus the motif term. Returns what
        controlled_decode_tweedie returns, the predictions being the plain reward model's; `motif_terms` holds per guided batch the
        motif term of its designs (fp32 [NUM_SAMPLES_PER_BATCH], on the device)."""
        from .motifs import GuidedReward
        guided_reward = GuidedReward(self.reward_model, motif_reward)
        self.motif_terms = []

        def guided():
            x = self.ref_model.controlled_sample_tweedie(guided_reward, eval_sp_size=self.NUM_SAMPLES_PER_BATCH, sample_M=sample_M,
                                                         options=options, task=self.task)
            self.motif_terms.append(motif_reward.term(x))
            return x
        return self._decode(gen_batch_num, sample_M, guided, tweedie_quirks=True)

    @torch.no_grad()
    def controlled_decode_TDS(self, gen_batch_num, sample_M, alpha):
        """SMC/TDS baseline (reference Enformer.py:479-557)."""
        return self._decode(gen_batch_num, sample_M, lambda: self.ref_model.controlled_sample_TDS(
            self.reward_model, alpha, eval_sp_size=self.NUM_SAMPLES_PER_BATCH, sample_M=sample_M))

    def _decode_guided_with_grad(self, gen_batch_num, sample_M, guided):
        """_decode for samplers whose guided decodes back-propagate: the gen_batch_num guided batches run first with autograd on (each
        with the Philox key _decode would give it), then the evaluation / baseline part under no_grad. Scoring consumes no RNG, so
        decoding all guided batches first keeps the reference's RNG order."""
        m = self.ref_model
        base, out = int(getattr(m, "philox_seed", 0)), []
        try:
            for k in range(gen_batch_num):
                if getattr(m, "rng_mode", "replay") == "philox":
                    m.philox_seed = batch_seed(base, k)           # the key _decode would give guided batch k
                out.append(guided())
        finally:
            if hasattr(m, "philox_seed"):
                m.philox_seed = base
        batches = iter(out)
        with torch.no_grad():
            return self._decode(gen_batch_num, sample_M, lambda: next(batches))

    def controlled_decode_DPS(self, gen_batch_num, sample_M, guidance_scale):
        """DPS baseline (reference Enformer.py:560-637). The guided decodes back-propagate through the backbone
        and the reward net, so they run with autograd on; the evaluation / baseline part runs under no_grad."""
        return self._decode_guided_with_grad(gen_batch_num, sample_M, lambda: self.ref_model.controlled_sample_DPS(
            self.reward_model, guidance_scale, eval_sp_size=self.NUM_SAMPLES_PER_BATCH, sample_M=sample_M))

    def controlled_decode_classfier(self, gen_batch_num, guidance_scale, sample_M=10):
        """Classifier guidance (reference Enformer.py:639-716): gen_batch_num guided batches (sample_M is not passed to the sampler,
        as in the reference), then gen_batch_num * sample_M un-guided baseline batches, then the top-k. The guided decodes need
        autograd only where the value net's gradient does not run on the fused kernels. The value net is used in the mode it is in:
        unlike the reference's decode_classfier.py for task "rna", nothing here switches it to train mode."""
        return self._decode_guided_with_grad(gen_batch_num, sample_M, lambda: self.ref_model.controlled_sample_classfier(
            self.embedding, self.head, eval_sp_size=self.NUM_SAMPLES_PER_BATCH, guidance_scale=guidance_scale))

    @torch.no_grad()
    def evaluate_nll(self, samples, n_draws=1):
        """ELBO estimate of -log p(x) under the pretrained model (ref_model.sequence_nll), in nats per sequence: fp64 [N]. `samples`:
        an [N, L] tensor, or a list of [B, L] batches or [L] rows as controlled_decode* return them (or `baseline_samples`)."""
        m = self.ref_model
        if isinstance(samples, (list, tuple)):
            samples = torch.cat([s.reshape(-1, s.shape[-1]).to(m.device) for s in samples])
        return m.sequence_nll(samples.to(m.device), n_draws=n_draws)

    @torch.no_grad()
    def evaluate_quality(self, samples, refs=None, train=None, k=3):
        """Set-level quality of decoded designs (svdd_amd.quality.sample_quality; the reference's on_validation_epoch_end numbers
        plus diversity and novelty) -> a flat dict. `samples` as in evaluate_nll; refs {name: tokens [N', L'] or k-mer counts
        [4^k]}: kmer_pearsonr_<name>, and for the token sets ws_scores_<name>, the 1-D Wasserstein distance between the harness's
        reward predictions on the designs and on that set; train [N, L]: the novelty keys."""
        from . import quality
        dev = self.ref_model.device
        if isinstance(samples, (list, tuple)):
            samples = torch.cat([torch.as_tensor(s).reshape(-1, s.shape[-1]).to(dev) for s in samples])
        samples = torch.as_tensor(samples).to(dev)
        n = self.NUM_SAMPLES_PER_BATCH

        def reward(t):
            t = torch.as_tensor(t).to(dev).long()
            pred = torch.cat([self._reward(t[i:i + n]) for i in range(0, t.shape[0], n)])
            return pred if self.n_tasks == 1 else pred[:, 0]
        token_refs = {name: r for name, r in (refs or {}).items() if getattr(r, "ndim", 0) == 2}
        return quality.sample_quality(samples, refs=refs, train=train, k=k, scores=reward(samples),
                                      ref_scores={name: reward(r) for name, r in token_refs.items()})

    @torch.no_grad()
    def select_library(self, samples, k, min_dist, revcomp=False):
        """The k best designs that are no near copies of each other (svdd_amd.quality.select_diverse; not in the
        reference): walk the designs from the highest reward prediction down and keep one when it is at least min_dist
        substitutions from every design kept (revcomp: on either strand) -> (tokens [P, L], scores [P], idx [P], report), P <= k,
        idx the kept rows of `samples` in pick order, report the flat dict of quality.library_quality. The scores are the
        harness's reward model's, task 0, as evaluate_quality computes them. `samples` as in evaluate_nll."""
        from . import quality
        return self._select_library(samples, k, min_dist, revcomp, quality.select_diverse)

    @torch.no_grad()
    def select_library_edit(self, samples, k, min_dist, revcomp=False):
        """select_library under a minimum EDIT distance (svdd_amd.quality.select_diverse_edit): a design is kept when it
        is at least min_dist edits (substitution, insertion, deletion) from every design kept, so a design and its copy shifted by
        a base or two are one family -> (tokens [P, L], scores [P], idx [P], report), report the flat dict of
        quality.library_quality_edit."""
        from . import quality
        return self._select_library(samples, k, min_dist, revcomp, quality.select_diverse_edit)

    def _select_library(self, samples, k, min_dist, revcomp, select):
        from . import quality
        dev = self.ref_model.device
        if isinstance(samples, (list, tuple)):
            samples = torch.cat([torch.as_tensor(s).reshape(-1, s.shape[-1]).to(dev) for s in samples])
        samples = torch.as_tensor(samples).to(dev)
        n = self.NUM_SAMPLES_PER_BATCH
        pred = torch.cat([self._reward(samples[i:i + n].long()) for i in range(0, samples.shape[0], n)])
        scores = (pred if self.n_tasks == 1 else pred[:, 0]).reshape(-1).float()
        sel, _, report = quality._library(samples, scores, k, min_dist, revcomp, select)
        idx = sel.picked[:k]
        return samples[idx], scores[idx], idx, report

    @torch.no_grad()
    def evaluate_edit(self, samples, edit_cap, train=None):
        """Near copies of decoded designs by edit distance (svdd_amd.quality.edit_quality; not in the reference) -> a flat dict:
        edit_near_batch_fraction, and with train [N, L'] edit_near_train_fraction, edit_near_train_min and (equal lengths)
        hamming_missed_fraction, all within edit_cap edits. `samples` as in evaluate_nll."""
        from . import quality
        dev = self.ref_model.device
        if isinstance(samples, (list, tuple)):
            samples = torch.cat([torch.as_tensor(s).reshape(-1, s.shape[-1]).to(dev) for s in samples])
        return quality.edit_quality(torch.as_tensor(samples).to(dev), edit_cap, train=train)

    @torch.no_grad()
    def evaluate_motifs(self, samples, mset, refs=None):
        """Motif content of decoded designs (svdd_amd.motifs; not in the reference) -> a flat dict: motif_spearman_<name> for every
        set of refs {name: tokens [N', L'] or motif frequencies [M]} (the rank correlation, over the motifs of `mset`, of the share
        of rows with a hit), motifs_per_row_mean (hits per design, both strands) and motifs_reachable. `samples` as in evaluate_nll."""
        from . import motifs
        dev = self.ref_model.device
        if isinstance(samples, (list, tuple)):
            samples = torch.cat([torch.as_tensor(s).reshape(-1, s.shape[-1]).to(dev) for s in samples])
        return motifs.motif_report(torch.as_tensor(samples).to(dev), mset, refs=refs)
