"""Torch-tensor front end of the C ABI (include/svdd_hip.h): raw pointers of CUDA(HIP) tensors
are handed to libsvdd_hip.so on torch's current stream. No fallbacks: tensors must live on the
GPU, and the library must be present.

Token tensors are uint8 (0..3 = A,C,G,T; 4 = MASK). `[B,L,5]` float tensors may be contiguous
(layout BLV) or a permuted view of a `[B,5,L]` buffer (layout BVL, what a Conv1d backbone
returns after `.permute(0, 2, 1)`, reference models/dnaconv.py:201); both are consumed in place.
"""
import ctypes
from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib
from ._lib import (LAYOUT_BLV, LAYOUT_BVL, RNG_PHILOX, RNG_REPLAY, SELECT_ARGMAX,  # noqa: F401
                   SELECT_MULTINOMIAL, SvddError, SvddRng)

MASK = 4


@dataclass
class Rng:
    """Uniform source for the categorical draws.

    replay : uniforms tensor = M consecutive blocks in the same memory layout as the logits
             (the bytes `M x rand_like(q_xs)` produce from torch's CPU mt19937 stream).
    philox : counter-based, keyed by (seed, step, row_offset + b, m, l)."""
    uniforms: Optional[torch.Tensor] = None
    seed: int = 0
    row_offset: int = 0
    step: int = 0
    uniforms_layout: Optional[int] = None      # None: same layout as the logits passed to propose()
    uniforms_rows: int = 0                     # replay: > 0 = the blocks hold a WHOLE batch of that many rows; ours start at row_offset

    def c_struct(self, logits_layout=LAYOUT_BLV):
        if self.uniforms is not None:
            ul = logits_layout if self.uniforms_layout is None else self.uniforms_layout
            return SvddRng(RNG_REPLAY, 0, self.uniforms.data_ptr(), 0, self.row_offset if self.uniforms_rows else 0, ul,
                           self.uniforms_rows)
        return SvddRng(RNG_PHILOX, self.step, None, self.seed & 0xFFFFFFFFFFFFFFFF, self.row_offset, 0, 0)


def _need(t, dtype, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise SvddError(f"{name} must be a GPU tensor (the SVDD hot path has no CPU fallback)")
    if t.dtype != dtype:
        raise SvddError(f"{name} must be {dtype}, got {t.dtype}")
    return t


def layout_of(t):
    """(tensor-to-pass, layout) for a logical [R,L,5] fp32 tensor."""
    assert t.dim() == 3 and t.shape[2] == 5, t.shape
    if t.is_contiguous():
        return t, LAYOUT_BLV
    if t.transpose(1, 2).is_contiguous():
        return t, LAYOUT_BVL
    return t.contiguous(), LAYOUT_BLV


def _empty_like_layout(t, layout):
    if layout == LAYOUT_BLV:
        return torch.empty(t.shape, dtype=torch.float32, device=t.device)
    R, L, V = t.shape
    return torch.empty((R, V, L), dtype=torch.float32, device=t.device).transpose(1, 2)


def propose(logits, x, dm, mcs, M, rng, want_q=False, cand=None, onehot=None):
    """-> (cand u8 [B,M,L], onehot f32 [B*M,L,4], q_xs f32 [B,L,5] (same strides as logits) | None)."""
    logits = _need(logits, torch.float32, "logits")
    x = _need(x, torch.uint8, "x").contiguous()
    B, L = x.shape
    logits, layout = layout_of(logits)
    assert logits.shape == (B, L, 5), (logits.shape, x.shape)
    if cand is None:
        cand = torch.empty((B, M, L), dtype=torch.uint8, device=x.device)
    if onehot is None:
        onehot = torch.empty((B * M, L, 4), dtype=torch.float32, device=x.device)
    q = _empty_like_layout(logits, layout) if want_q else None
    if rng.uniforms is not None:
        u = _need(rng.uniforms, torch.float32, "uniforms")
        rows = rng.uniforms_rows if rng.uniforms_rows else B       # (a shard of a batch of uniforms_rows rows: the whole batch's blocks)
        assert u.is_contiguous() and u.numel() == M * rows * L * 5 and rng.row_offset * bool(rng.uniforms_rows) + B <= rows, (u.shape, M, B, L)
    rs = rng.c_struct(layout)
    _lib.call("svdd_propose", logits, x, float(dm), float(mcs), B, L, M, layout, ctypes.byref(rs), cand, onehot, q)
    return cand, onehot, q


def sample_categorical(q, x, M, rng):
    """M categorical draws from a caller-built q [B,L,5] (>= 0), merged with copy_flag -> (cand, onehot)."""
    q = _need(q, torch.float32, "q")
    x = _need(x, torch.uint8, "x").contiguous()
    B, L = x.shape
    q, layout = layout_of(q)
    cand = torch.empty((B, M, L), dtype=torch.uint8, device=x.device)
    onehot = torch.empty((B * M, L, 4), dtype=torch.float32, device=x.device)
    rs = rng.c_struct(layout)
    _lib.call("svdd_sample_categorical", q, x, B, L, M, layout, ctypes.byref(rs), cand, onehot)
    return cand, onehot


def classifier_propose(logits, x, grad4, dm, mcs, scale, rng, want_onehot=True, want_q=False, x_next=None, onehot=None):
    """One classifier-guidance draw per position (svdd_classifier_propose): w = q_xs + scale * cat(grad4, 0), signed, one categorical
    draw, merged with copy_flag. grad4 fp32 [B,L,4]. -> (x_next u8 [B,L], onehot f32 [B,L,4] | None, un-guided q_xs f32 [B,L,5] (same
    strides as logits) | None)."""
    logits = _need(logits, torch.float32, "logits")
    x = _need(x, torch.uint8, "x").contiguous()
    g = _need(grad4, torch.float32, "grad4").contiguous()
    B, L = x.shape
    logits, layout = layout_of(logits)
    assert logits.shape == (B, L, 5) and g.shape == (B, L, 4), (logits.shape, g.shape, x.shape)
    if x_next is None:
        x_next = torch.empty((B, L), dtype=torch.uint8, device=x.device)
    if want_onehot and onehot is None:
        onehot = torch.empty((B, L, 4), dtype=torch.float32, device=x.device)
    q = _empty_like_layout(logits, layout) if want_q else None
    if rng.uniforms is not None:
        u = _need(rng.uniforms, torch.float32, "uniforms")
        rows = rng.uniforms_rows if rng.uniforms_rows else B
        assert u.is_contiguous() and u.numel() == rows * L * 5 and rng.row_offset * bool(rng.uniforms_rows) + B <= rows, (u.shape, B, L)
    rs = rng.c_struct(layout)
    _lib.call("svdd_classifier_propose", logits, layout, x, g, float(dm), float(mcs), float(scale), B, L, ctypes.byref(rs), x_next,
              onehot if want_onehot else None, q)
    return x_next, (onehot if want_onehot else None), q


def elbo_mask(x0, K, rng, eps=1e-3, move_chance=None, want_scalars=True, want_count=False, xt=None):
    """svdd_elbo_mask: K masked copies of x0 u8 [n, L] -> xt u8 [n K, L] (row k n + b = draw k of sequence b) and per row
    (t, move_chance, w) f32 [n K] (Philox; replay: None, the caller holds them) and the masked count i32 [n K] | None.
    replay: rng.uniforms = K blocks of n L fp32 ([b][l]: torch.rand(n, L)), move_chance f32 [n K] given.
    philox: keyed by (rng.seed, rng.row_offset + b, k, l); t stratified over each sequence's own K draws."""
    x0 = _need(x0, torch.uint8, "x0").contiguous()
    n, L = x0.shape
    dev = x0.device
    replay = rng.uniforms is not None
    if replay:
        u = _need(rng.uniforms, torch.float32, "uniforms")
        mc_in = _need(move_chance, torch.float32, "move_chance").contiguous()
        assert u.is_contiguous() and u.numel() == K * n * L and mc_in.numel() == K * n, (u.shape, mc_in.shape, K, n, L)
        want_scalars = False
    elif move_chance is not None:
        raise SvddError("elbo_mask: move_chance is the replay mode's input; Philox computes it")
    if xt is None:
        xt = torch.empty((K * n, L), dtype=torch.uint8, device=dev)
    t, mc, w = ((torch.empty(K * n, dtype=torch.float32, device=dev) for _ in range(3)) if want_scalars else (None, None, None))
    cnt = torch.empty(K * n, dtype=torch.int32, device=dev) if want_count else None
    rs = rng.c_struct()
    _lib.call("svdd_elbo_mask", x0, n, L, K, float(eps), ctypes.byref(rs), mc_in if replay else None, xt, t, mc, w, cnt)
    return xt, t, mc, w, cnt


def elbo_nll(logits, xt, x0, w, K=1, want_tokens=True, want_mean=False, err=None):
    """svdd_elbo_nll: logits [n K, L, 5] (either layout, as subs_logp), xt u8 [n K, L], x0 u8 [n, L], w f32 [n K] ->
    (nll f32 [n K, L] | None, row_sum f64 [n K], seq_mean f64 [n] | None). err: a caller-zeroed device int32 [1] the kernel sets
    for a token > 3 in x0 (checked by the caller later); None: checked here (one synchronisation)."""
    logits = _need(logits, torch.float32, "logits")
    xt = _need(xt, torch.uint8, "xt").contiguous()
    x0 = _need(x0, torch.uint8, "x0").contiguous()
    w = _need(w, torch.float32, "w").contiguous()
    n, L = x0.shape
    logits, layout = layout_of(logits)
    assert logits.shape == (K * n, L, 5) and xt.shape == (K * n, L) and w.numel() == K * n, (logits.shape, xt.shape, w.shape, K, n)
    dev = x0.device
    nll = torch.empty((K * n, L), dtype=torch.float32, device=dev) if want_tokens else None
    row_sum = torch.empty(K * n, dtype=torch.float64, device=dev)
    mean = torch.empty(n, dtype=torch.float64, device=dev) if want_mean else None
    check_here = err is None
    if check_here:
        err = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.call("svdd_elbo_nll", logits, layout, xt, x0, w, n, L, K, nll, row_sum, mean, err)
    if check_here:
        check_elbo_err(err)
    return nll, row_sum, mean


def check_elbo_err(err):
    """Raise if svdd_elbo_nll flagged a token > 3 in x0 (SVDD_E_ARG)."""
    if int(err[0]) != 0:
        _lib.check(_lib.E_ARG, "svdd_elbo_nll: x0 holds a token > 3")


def refine_remask(x_new, move_chance, rng, x_old=None, score_new=None, score_old=None, frozen=None, x_keep=None, score_keep=None,
                  accepted=None, x_t=None, nmasked=None, err=None, remask=True):
    """svdd_refine_remask, the round boundary of re-mask refinement, one launch: per row keep x_new iff score_new > score_old (only
    when x_old, score_new and score_old are all given; a NaN or a tie keeps x_old; otherwise x_new is kept), then x_t = MASK where
    u < move_chance and frozen == 0, else the kept row. -> (x_t u8 [B, L] | None, x_keep u8 [B, L] | None, score_keep f32 [B] | None).
    x_keep may be x_old. accepted / nmasked: caller-owned i32 [B] outputs (new row kept / MASK tokens of x_t). move_chance: ONE
    fp32 scalar the caller computed with the reference's fp32 torch ops. remask=False: the accept step alone (x_t is None, rng unused).
    replay: rng.uniforms = torch.rand(B, L) ([b][l]); philox: keyed by (rng.seed, rng.row_offset + b, round = rng.step, l).
    err: a caller-zeroed device int32 [1] the kernel sets for a token > 4 (checked by the caller later); None: checked here (one
    synchronisation)."""
    x_new = _need(x_new, torch.uint8, "x_new").contiguous()
    B, L = x_new.shape
    dev = x_new.device
    judged = x_old is not None and score_new is not None and score_old is not None
    for name, t in (("x_old", x_old), ("frozen", frozen), ("x_keep", x_keep), ("x_t", x_t)):
        if t is not None and not (_need(t, torch.uint8, name).is_contiguous() and tuple(t.shape) == (B, L)):
            raise SvddError(f"{name} must be a contiguous u8 [{B}, {L}] tensor, got {tuple(t.shape)}")
    for name, t, dt in (("score_new", score_new, torch.float32), ("score_old", score_old, torch.float32),
                        ("score_keep", score_keep, torch.float32), ("accepted", accepted, torch.int32), ("nmasked", nmasked, torch.int32)):
        if t is not None and not (_need(t, dt, name).is_contiguous() and t.numel() == B):
            raise SvddError(f"{name} must be a contiguous [{B}] tensor, got {tuple(t.shape)}")
    if judged and x_keep is None:
        x_keep = torch.empty((B, L), dtype=torch.uint8, device=dev)
    if score_new is not None and score_keep is None:
        score_keep = torch.empty(B, dtype=torch.float32, device=dev)
    rs = None
    if remask:
        if x_t is None:
            x_t = torch.empty((B, L), dtype=torch.uint8, device=dev)
        if rng.uniforms is not None:
            u = _need(rng.uniforms, torch.float32, "uniforms")
            assert u.is_contiguous() and u.numel() == B * L and not rng.uniforms_rows, (u.shape, B, L, rng.uniforms_rows)
        rs = ctypes.byref(rng.c_struct())
    else:
        x_t = None
    check_here = err is None
    if check_here:
        err = torch.zeros(1, dtype=torch.int32, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)         # this entry takes its stream as an explicit argument
    _lib.call("svdd_refine_remask", x_new, x_old, score_new, score_old, frozen, float(move_chance), B, L, rs, x_keep, score_keep,
              accepted, x_t, nmasked if remask else None, err, stream)
    if check_here:
        check_refine_err(err)
    return x_t, x_keep, score_keep


def check_refine_err(err):
    """Raise if svdd_refine_remask flagged a token > 4 (SVDD_E_ARG)."""
    if int(err[0]) != 0:
        _lib.check(_lib.E_ARG, "svdd_refine_remask: a row holds a token > 4")


TARGET_REDUCE = {"mean": _lib.TARGET_MEAN, "logmeanexp": _lib.TARGET_LOGMEANEXP}


def value_target(scores, cand, reduce="mean", alpha=1.0, x_next=None, onehot_next=None, target=None):
    """svdd_value_target, the step boundary of a CD-Q rollout, one launch: x_next = cand[:, M - 1] (the reference continues from its
    last draw), onehot_next = its one-hot (MASK rows zero) and target[b] = the reduction of scores[b, :] — "mean": the reference's
    sequential fp32 sum in ascending m and one division (Enformer.py:235-238), bit for bit; "logmeanexp": alpha log mean exp(s / alpha).
    -> (x_next u8 [B, L], onehot_next f32 [B, L, 4] | None, target f32 [B] | None). cand u8 [B, M, L]; scores f32 [B, M] or None (no
    target: step 0 of a rollout). x_next / onehot_next / target: caller-owned outputs (slices of a training-set slab); x_next and
    target are allocated when missing, onehot_next is written only when given."""
    cand = _need(cand, torch.uint8, "cand").contiguous()
    if cand.dim() != 3:
        raise SvddError(f"cand must be u8 [B, M, L], got {tuple(cand.shape)}")
    B, M, L = cand.shape
    dev = cand.device
    if reduce not in TARGET_REDUCE:
        raise ValueError(f"reduce = {reduce!r}: expected 'mean' or 'logmeanexp'")
    if x_next is None:
        x_next = torch.empty((B, L), dtype=torch.uint8, device=dev)
    elif not (_need(x_next, torch.uint8, "x_next").is_contiguous() and tuple(x_next.shape) == (B, L)):
        raise SvddError(f"x_next must be a contiguous u8 [{B}, {L}] tensor, got {tuple(x_next.shape)}")
    if onehot_next is not None and not (_need(onehot_next, torch.float32, "onehot_next").is_contiguous()
                                        and onehot_next.numel() == B * L * 4):
        raise SvddError(f"onehot_next must be a contiguous f32 [{B}, {L}, 4] tensor, got {tuple(onehot_next.shape)}")
    if scores is None:
        if target is not None:
            raise SvddError("value_target: a target needs scores")
    else:
        scores = _need(scores, torch.float32, "scores").contiguous()
        if scores.numel() != B * M:
            raise SvddError(f"scores must be f32 [{B}, {M}], got {tuple(scores.shape)}")
        if target is None:
            target = torch.empty(B, dtype=torch.float32, device=dev)
        elif not (_need(target, torch.float32, "target").is_contiguous() and target.numel() == B):
            raise SvddError(f"target must be a contiguous f32 [{B}] tensor, got {tuple(target.shape)}")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)         # this entry takes its stream as an explicit argument
    _lib.call("svdd_value_target", scores, cand, B, L, M, TARGET_REDUCE[reduce], float(alpha), x_next, onehot_next, target, stream)
    return x_next, onehot_next, target


EVOLVE_STOP = {"global": _lib.EVOLVE_GLOBAL, "row": _lib.EVOLVE_ROW}


def _this_stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)           # the ISM entries take their stream as an explicit argument


def _is(t, dtype, shape, name):
    if not (_need(t, dtype, name).is_contiguous() and tuple(t.shape) == tuple(shape)):
        raise SvddError(f"{name} must be a contiguous {dtype} {list(shape)} tensor, got {t.dtype} {tuple(t.shape)}")
    return t


# The argument checks the ISM entries (svdd_ism_mutants / _fold / svdd_evolve_apply) share with their pattern siblings.
def _mutant_parents(x, positions):
    x = _need(x, torch.uint8, "x").contiguous()
    if x.dim() != 2:
        raise SvddError(f"x must be u8 [B, L], got {tuple(x.shape)}")
    return x, _need(positions, torch.int32, "positions").contiguous()


def _mutant_buffers(x, M, live, cand, onehot, want_onehot, err):
    """live and the outputs of a mutants entry with M mutants per row -> (cand, onehot, err, whether err is checked here)."""
    (B, L), dev = x.shape, x.device
    if live is not None:
        _is(live, torch.uint8, (B,), "live")
    cand = torch.empty((B, M, L), dtype=torch.uint8, device=dev) if cand is None else _is(cand, torch.uint8, (B, M, L), "cand")
    if onehot is None and want_onehot:
        onehot = torch.empty((B * M, L, 4), dtype=torch.float32, device=dev)
    elif onehot is not None:
        _is(onehot, torch.float32, (B * M, L, 4), "onehot")
    if err is None:
        return cand, onehot, torch.zeros(1, dtype=torch.int32, device=dev), True
    return cand, onehot, err, False


def _best_triple(best, B, second):
    """best = (best_score f32 [B], best_pos i32 [B], `second` i32 [B]) of a fold entry, checked."""
    bs, bp, b2 = best
    _is(bs, torch.float32, (B,), "best_score"), _is(bp, torch.int32, (B,), "best_pos"), _is(b2, torch.int32, (B,), second)
    return bs, bp, b2


def _evolve_stop(stop, x):
    if stop not in EVOLVE_STOP:
        raise ValueError(f"stop = {stop!r}: expected 'global' or 'row'")
    return _need(x, torch.uint8, "x").shape


def _evolve_state(x, score_cur, best_so_far, stopped, x_best, score_best, live, trace, second):
    """The state an apply entry updates in place, checked -> the trace's four rows (None each without a trace)."""
    B, L = x.shape
    _is(x, torch.uint8, (B, L), "x"), _is(x_best, torch.uint8, (B, L), "x_best")
    _is(score_cur, torch.float32, (B,), "score_cur"), _is(score_best, torch.float32, (B,), "score_best")
    _is(best_so_far, torch.float32, (1,), "best_so_far"), _is(stopped, torch.int32, (1,), "stopped")
    if live is not None:
        _is(live, torch.uint8, (B,), "live")
    if trace is None:
        return None, None, None, None
    tp, t2, ts, tt = trace
    _is(tp, torch.int32, (B,), "trace position"), _is(t2, torch.int32, (B,), f"trace {second}")
    _is(ts, torch.float32, (B,), "trace score"), _is(tt, torch.uint8, (B,), "trace taken")
    return tp, t2, ts, tt


def ism_mutants(x, positions, live=None, cand=None, onehot=None, want_onehot=True, err=None):
    """svdd_ism_mutants: the 3 P single-base mutants of every row of x u8 [B, L] at positions i32 [P] (device, ascending), in
    ISMDataset(drop_ref=True) order: mutant (b, j, k) = row b with positions[j] set to the k-th base that is not the parent's.
    -> (cand u8 [B, 3P, L], onehot f32 [B * 3P, L, 4] | None). live u8 [B]: a row with live[b] == 0 gets exact copies. err: a
    caller-zeroed device int32 [1] the kernel sets for a parent token > 3 or a position outside 0..L-1 (checked by the caller later
    with check_ism_err); None: checked here (one synchronisation)."""
    x, positions = _mutant_parents(x, positions)
    (B, L), P = x.shape, positions.numel()
    cand, onehot, err, check_here = _mutant_buffers(x, 3 * P, live, cand, onehot, want_onehot, err)
    _lib.call("svdd_ism_mutants", x, positions, live, B, L, P, cand, onehot, err, _this_stream())
    if check_here:
        check_ism_err(err)
    return cand, onehot


def check_ism_err(err):
    """Raise if svdd_ism_mutants flagged a parent token > 3 or a position out of range (SVDD_E_ARG)."""
    if int(err[0]) != 0:
        _lib.check(_lib.E_ARG, "svdd_ism_mutants: a row holds a token > 3, or a position is outside 0..L-1")


def ism_fold(scores, parent_score, x, positions, p0, Pc, slot=None, live=None, ism=None, best=None):
    """svdd_ism_fold: fold the scores of the mutants of positions[p0 : p0 + Pc] into ism f32 [B, P, 4] (or None) and the running
    best = (best_score f32 [B], best_pos i32 [B], best_allele i32 [B]) (or None). scores: dense f32 [B, 3 Pc], or with slot (i32
    [B * 3 Pc], svdd_compact_flags' map) the compacted scores: mutant i has scores[slot[i]], or the parent's score where slot[i] < 0.
    The chunk with p0 == 0 starts the running best at (-inf, -1, -1); fold chunks in ascending p0."""
    x = _need(x, torch.uint8, "x")
    B, L = x.shape
    P = positions.numel()
    scores = _need(scores, torch.float32, "scores")
    if not x.is_contiguous() or not scores.is_contiguous() or (slot is None and scores.numel() != B * 3 * Pc):
        raise SvddError(f"ism_fold: x [{B}, {L}] and scores [{B}, {3 * Pc}] must be contiguous, got scores {tuple(scores.shape)}")
    _is(_need(positions, torch.int32, "positions"), torch.int32, (P,), "positions")
    _is(parent_score, torch.float32, (B,), "parent_score")
    if slot is not None:
        _is(slot, torch.int32, (B * 3 * Pc,), "slot")
    if live is not None:
        _is(live, torch.uint8, (B,), "live")
    if ism is not None:
        _is(ism, torch.float32, (B, P, 4), "ism")
    bs, bp, ba = (None, None, None) if best is None else _best_triple(best, B, "best_allele")
    _lib.call("svdd_ism_fold", scores, slot, parent_score, x, positions, live, B, L, P, int(p0), int(Pc), ism, bs, bp, ba, _this_stream())


def evolve_apply(best, x, score_cur, best_so_far, stopped, x_best, score_best, stop="global", live=None, trace=None):
    """svdd_evolve_apply, one iteration's boundary of ISM-driven evolution, one launch: best = (best_score, best_pos, best_allele)
    of svdd_ism_fold; x u8 [B, L], score_cur f32 [B], live u8 [B] (required for stop = "row"), best_so_far f32 [1], stopped i32 [1],
    x_best u8 [B, L], score_best f32 [B] are updated in place; trace = (position i32 [B], allele i32 [B], score f32 [B], taken u8 [B])
    of this iteration or None. Nothing is written once stopped[0] != 0."""
    B, L = _evolve_stop(stop, x)
    bs, bp, ba = _best_triple(best, B, "best_allele")
    tp, ta, ts, tt = _evolve_state(x, score_cur, best_so_far, stopped, x_best, score_best, live, trace, "allele")
    _lib.call("svdd_evolve_apply", bs, bp, ba, B, L, EVOLVE_STOP[stop], x, score_cur, live, best_so_far, stopped, x_best, score_best,
              tp, ta, ts, tt, _this_stream())


def _pattern_args(patterns, widths):
    """patterns u8 [K, 32] and widths i32 [K] of the three pattern entries -> K."""
    _need(patterns, torch.uint8, "patterns"), _need(widths, torch.int32, "widths")
    K = widths.numel()
    _is(patterns, torch.uint8, (K, _lib.PATTERN_MAX_WIDTH), "patterns"), _is(widths, torch.int32, (K,), "widths")
    return K


def pattern_mutants(x, positions, patterns, widths, live=None, cand=None, onehot=None, want_onehot=True, err=None):
    """svdd_pattern_mutants: the P K pattern mutants of every row of x u8 [B, L]: mutant (b, j, k) = row b with
    x[b, positions[j] : positions[j] + widths[k]] overwritten by patterns[k, :widths[k]] (the pattern index runs fastest).
    positions i32 [P] (device, ascending starts), patterns u8 [K, 32], widths i32 [K]. -> (cand u8 [B, P K, L], onehot f32
    [B * P K, L, 4] | None). live u8 [B]: a row with live[b] == 0 gets exact copies. err: a caller-zeroed device int32 [1] the kernel
    sets for a parent token > 3, a pattern token > 3 or a window that leaves the row (checked by the caller later with
    check_pattern_err); None: checked here (one synchronisation)."""
    x, positions = _mutant_parents(x, positions)
    (B, L), P = x.shape, positions.numel()
    K = _pattern_args(patterns, widths)
    cand, onehot, err, check_here = _mutant_buffers(x, P * K, live, cand, onehot, want_onehot, err)
    _lib.call("svdd_pattern_mutants", x, positions, patterns, widths, live, B, L, P, K, cand, onehot, err, _this_stream())
    if check_here:
        check_pattern_err(err)
    return cand, onehot


def check_pattern_err(err):
    """Raise if svdd_pattern_mutants flagged a token > 3 in a row or a pattern, or a pattern that does not fit at a position."""
    if int(err[0]) != 0:
        _lib.check(_lib.E_ARG, "svdd_pattern_mutants: a row or a pattern holds a token > 3, or a pattern's window lies outside 0..L-1")


def pattern_fold(scores, parent_score, P, K, p0, Pc, slot=None, live=None, table=None, best=None):
    """svdd_pattern_fold: fold the scores of the mutants of positions[p0 : p0 + Pc] into table f32 [B, P, K] (or None) and the
    running best = (best_score f32 [B], best_pos i32 [B]: the index into positions, best_pattern i32 [B]) (or None). scores: dense
    f32 [B, Pc K], or with slot (i32 [B * Pc K], svdd_compact_flags' map) the compacted scores: mutant i has scores[slot[i]], or
    the parent's score where slot[i] < 0. The chunk with p0 == 0 starts the running best at (-inf, -1, -1); fold in ascending p0."""
    parent_score = _need(parent_score, torch.float32, "parent_score")
    B = parent_score.numel()
    P, K, p0, Pc = int(P), int(K), int(p0), int(Pc)
    _is(parent_score, torch.float32, (B,), "parent_score")
    scores = _need(scores, torch.float32, "scores")
    if not scores.is_contiguous() or (slot is None and scores.numel() != B * Pc * K):
        raise SvddError(f"pattern_fold: scores must be contiguous f32 [{B}, {Pc * K}], got {tuple(scores.shape)}")
    if slot is not None:
        _is(slot, torch.int32, (B * Pc * K,), "slot")
    if live is not None:
        _is(live, torch.uint8, (B,), "live")
    if table is not None:
        _is(table, torch.float32, (B, P, K), "table")
    bs, bp, bk = (None, None, None) if best is None else _best_triple(best, B, "best_pattern")
    _lib.call("svdd_pattern_fold", scores, slot, parent_score, live, B, P, K, p0, Pc, table, bs, bp, bk, _this_stream())


def pattern_apply(best, positions, patterns, widths, x, score_cur, best_so_far, stopped, x_best, score_best, stop="global", live=None,
                  trace=None):
    """svdd_pattern_apply, one iteration's boundary of pattern-driven evolution, one launch: best = (best_score, best_pos,
    best_pattern) of svdd_pattern_fold; x u8 [B, L], score_cur f32 [B], live u8 [B] (required for stop = "row"), best_so_far f32
    [1], stopped i32 [1], x_best u8 [B, L], score_best f32 [B] are updated in place; trace = (start position i32 [B], pattern i32
    [B], score f32 [B], taken u8 [B]) of this iteration or None. Nothing is written once stopped[0] != 0."""
    B, L = _evolve_stop(stop, x)
    positions = _need(positions, torch.int32, "positions")
    P = positions.numel()
    _is(positions, torch.int32, (P,), "positions")
    K = _pattern_args(patterns, widths)
    bs, bp, bk = _best_triple(best, B, "best_pattern")
    tp, tk, ts, tt = _evolve_state(x, score_cur, best_so_far, stopped, x_best, score_best, live, trace, "pattern")
    _lib.call("svdd_pattern_apply", bs, bp, bk, positions, patterns, widths, B, L, P, K, EVOLVE_STOP[stop], x, score_cur, live,
              best_so_far, stopped, x_best, score_best, tp, tk, ts, tt, _this_stream())


ATTR_MODE = {"gradient": _lib.ATTR_GRADIENT, "times_input": _lib.ATTR_TIMES_INPUT}


def _attr_baseline(baseline, B, L):
    """-> baseline_rows of the two attribution entries: baseline f32 [L, 4] (1), [B, L, 4] (B) or None (0: zeros)."""
    if baseline is None:
        return 0
    _need(baseline, torch.float32, "baseline")
    if not baseline.is_contiguous() or tuple(baseline.shape) not in ((L, 4), (B, L, 4)):
        raise SvddError(f"baseline must be a contiguous fp32 [{L}, 4] or [{B}, {L}, 4] tensor, got {tuple(baseline.shape)}")
    return 1 if baseline.dim() == 2 else B


def attr_path(x, alpha, r0, n_rows, out, baseline=None, n_pad=0, err=None):
    """svdd_attr_path: the interpolants base + alpha[k] * (onehot(x[b]) - base) of the (row, step) pairs r0 .. r0 + n_rows - 1
    (pair r = b * S + k, S = alpha.numel()) into out f32 [n_rows + n_pad, L, 4] (caller-owned); the n_pad rows after them are
    copies of row 0. x u8 [B, L] (4 = MASK: a zero one-hot row), alpha f32 [S], baseline f32 [L, 4] / [B, L, 4] / None (zeros).
    err: a caller-zeroed device int32 [1] the kernel sets for a token > 4 (check_attr_err), or None."""
    x = _need(x, torch.uint8, "x")
    if x.dim() != 2 or not x.is_contiguous():
        raise SvddError(f"x must be a contiguous u8 [B, L] tensor, got {tuple(x.shape)}")
    B, L = x.shape
    S = _need(alpha, torch.float32, "alpha").numel()
    _is(alpha, torch.float32, (S,), "alpha")
    _is(out, torch.float32, (int(n_rows) + int(n_pad), L, 4), "out")
    if err is not None:
        _is(err, torch.int32, (1,), "err")
    _lib.call("svdd_attr_path", x, baseline, _attr_baseline(baseline, B, L), alpha, B, L, S, int(r0), int(n_rows), int(n_pad), out,
              err, _this_stream())
    return out


def check_attr_err(err):
    """Raise if svdd_attr_path flagged a token > 4 (SVDD_E_ARG)."""
    if int(err[0]) != 0:
        _lib.check(_lib.E_ARG, "svdd_attr_path: a row holds a token > 4")


def attr_fold(grad, scale, weight, x, r0, n_rows, acc, attr, mode="times_input", baseline=None, rowsum=None):
    """svdd_attr_fold: acc[b] += weight[k] * (scale * grad[i]) for the pairs r0 .. r0 + n_rows - 1 of svdd_attr_path's order (grad
    f32 [>= n_rows, L, 4]; a row starts from 0 at its step 0), and every row whose last step is among them finished into attr f32
    [B, 4, L]: acc itself (mode "gradient") or (onehot(x) - baseline) * acc ("times_input"); rowsum f32 [B] or None: the finished
    rows' sums. acc f32 [B, L, 4], attr and rowsum are caller-owned; fold passes in ascending r0."""
    if mode not in ATTR_MODE:
        raise ValueError(f"mode = {mode!r}: expected 'gradient' or 'times_input'")
    x = _need(x, torch.uint8, "x")
    if x.dim() != 2 or not x.is_contiguous():
        raise SvddError(f"x must be a contiguous u8 [B, L] tensor, got {tuple(x.shape)}")
    B, L = x.shape
    S = _need(weight, torch.float32, "weight").numel()
    _is(weight, torch.float32, (S,), "weight")
    _need(grad, torch.float32, "grad")
    if not grad.is_contiguous() or grad.dim() != 3 or grad.shape[0] < int(n_rows) or tuple(grad.shape[1:]) != (L, 4):
        raise SvddError(f"grad must be a contiguous fp32 [>= {n_rows}, {L}, 4] tensor, got {tuple(grad.shape)}")
    _is(acc, torch.float32, (B, L, 4), "acc"), _is(attr, torch.float32, (B, 4, L), "attr")
    if rowsum is not None:
        _is(rowsum, torch.float32, (B,), "rowsum")
    _lib.call("svdd_attr_fold", grad, float(scale), weight, x, baseline, _attr_baseline(baseline, B, L), B, L, S, int(r0), int(n_rows),
              ATTR_MODE[mode], acc, attr, rowsum, _this_stream())


LEDIDI_MAX_L, LEDIDI_MAX_S = 1024, 64                                     # svdd_ledidi_step (include/svdd_hip.h)


class LedidiConfig:
    """The hyper-parameters of svdd_ledidi_step as the kernel takes them: every derived constant is computed here in float64 and
    rounded once to fp32 (struct svdd_ledidi_cfg). at(i, scale) -> the struct for the launch that closes iteration i (AdamW step
    count i + 1)."""

    def __init__(self, S, tau=1.0, l=0.1, lr=1.0, eps=1e-4, patience=100, betas=(0.9, 0.999), adam_eps=1e-8, weight_decay=0.01):
        import math
        self.S, self.lr, self.betas = int(S), float(lr), (float(betas[0]), float(betas[1]))
        self.c = _lib.SvddLedidiCfg(tau=float(tau), l=float(l), la=math.log(1.0 + float(eps)), lb=math.log(float(eps)), scale=1.0,
                                    decay=1.0 - float(lr) * float(weight_decay), w1=1.0 - self.betas[0], beta2=self.betas[1],
                                    w2=1.0 - self.betas[1], adam_eps=float(adam_eps), step_size=float(lr), bc2_sqrt=1.0,
                                    patience=int(patience))

    def at(self, i, scale=1.0):
        import math
        t = int(i) + 1
        self.c.scale = float(scale)
        self.c.step_size = self.lr / (1.0 - self.betas[0] ** t)
        self.c.bc2_sqrt = math.sqrt(1.0 - self.betas[1] ** t)
        return self.c


class LedidiState:
    """The caller-owned buffers of svdd_ledidi_step for B designs of S samples at length L: the logit weights and AdamW moments
    (zero), the samples' softmax, the hard samples and their edit counts, the best-so-far fields, the patience counters and the live
    count. best_total / best_output start from output0 [B] fp32 (the output loss of the start sequences), x_best / score_best from
    the S copies of x0 and score0."""

    def __init__(self, x0, S, score0, output0):
        B, L = x0.shape
        dev = x0.device
        self.B, self.L, self.S = B, L, S
        self.w, self.m, self.v = (torch.zeros((B, L, 4), dtype=torch.float32, device=dev) for _ in range(3))
        self.y = torch.zeros((B, S, L, 4), dtype=torch.float32, device=dev)
        self.tok = x0[:, None, :].expand(B, S, L).contiguous()
        self.edits = torch.zeros((B, S), dtype=torch.int32, device=dev)
        self.best_total, self.best_output = output0.clone(), output0.clone()
        self.best_input = torch.zeros(B, dtype=torch.float32, device=dev)
        self.best_iter = torch.full((B,), -1, dtype=torch.int32, device=dev)
        self.x_best = self.tok.clone()
        self.score_best = score0[:, None].expand(B, S).contiguous()
        self.wo, self.stopped = (torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(2))
        self.live = torch.full((1,), B, dtype=torch.int32, device=dev)


def ledidi_step(x0, st, cfg, xin, d0, nd, iter, rng=None, grad=None, sc=None, target=None, editable=None, n_pad=0, sample=True,
                trace=None, err=None):
    """svdd_ledidi_step, one launch for the designs d0 .. d0 + nd - 1 of x0 u8 [B, L] on the state st (LedidiState, updated in place).
    grad f32 [>= nd S, L, 4] (the chunk's gradient pass, row (d - d0) S + s) and sc f32 [B, S] given: close iteration `iter` (losses,
    best-so-far, patience, AdamW), then with sample draw iteration iter + 1's samples; grad None: draw iteration `iter`'s samples only.
    cfg: the struct LedidiConfig.at(iter, scale) returns. xin f32 [nd S + n_pad, L, 4]: the chunk's one-hot rows, pads = copies of
    row 0. rng: ops.Rng, replay (uniforms f32 [B, S, L, 4] of the sampled iteration) or philox (seed, row_offset). target f32 [B],
    editable u8 [L], trace = (total, out, inp) f32 [B] each, err i32 [1] (caller-zeroed; a start token > 3): each may be None."""
    x0 = _need(x0, torch.uint8, "x0")
    B, L, S = st.B, st.L, st.S
    _is(x0, torch.uint8, (B, L), "x0")
    d0, nd, n_pad = int(d0), int(nd), int(n_pad)
    _is(xin, torch.float32, (nd * S + n_pad, L, 4), "xin")
    for name, t, dtype, shape in (("w", st.w, torch.float32, (B, L, 4)), ("m", st.m, torch.float32, (B, L, 4)),
                                  ("v", st.v, torch.float32, (B, L, 4)), ("y", st.y, torch.float32, (B, S, L, 4)),
                                  ("tok", st.tok, torch.uint8, (B, S, L)), ("edits", st.edits, torch.int32, (B, S)),
                                  ("best_total", st.best_total, torch.float32, (B,)), ("best_output", st.best_output, torch.float32, (B,)),
                                  ("best_input", st.best_input, torch.float32, (B,)), ("best_iter", st.best_iter, torch.int32, (B,)),
                                  ("x_best", st.x_best, torch.uint8, (B, S, L)), ("score_best", st.score_best, torch.float32, (B, S)),
                                  ("wo", st.wo, torch.int32, (B,)), ("stopped", st.stopped, torch.int32, (B,)),
                                  ("live", st.live, torch.int32, (1,))):
        _is(t, dtype, shape, name)
    if grad is not None:
        _need(grad, torch.float32, "grad")
        if not grad.is_contiguous() or grad.dim() != 3 or grad.shape[0] < nd * S or tuple(grad.shape[1:]) != (L, 4):
            raise SvddError(f"grad must be a contiguous fp32 [>= {nd * S}, {L}, 4] tensor, got {tuple(grad.shape)}")
        _is(sc, torch.float32, (B, S), "sc")
    if target is not None:
        _is(target, torch.float32, (B,), "target")
    if editable is not None:
        _is(editable, torch.uint8, (L,), "editable")
    if err is not None:
        _is(err, torch.int32, (1,), "err")
    tt = to = ti = None
    if trace is not None:
        tt, to, ti = trace
        for name, t in (("trace total", tt), ("trace out", to), ("trace in", ti)):
            _is(t, torch.float32, (B,), name)
    rs = None
    if sample:
        if rng is None:
            raise SvddError("ledidi_step: sampling needs an Rng")
        if rng.uniforms is not None:
            _is(rng.uniforms, torch.float32, (B, S, L, 4), "rng.uniforms")
        rs = ctypes.byref(rng.c_struct())
    _lib.call("svdd_ledidi_step", x0, editable, grad, sc, target, ctypes.byref(cfg), rs, B, L, S, d0, nd, n_pad, int(iter),
              int(bool(sample)), st.w, st.m, st.v, st.y, st.tok, xin, st.edits, st.best_total, st.best_output, st.best_input,
              st.best_iter, st.x_best, st.score_best, st.wo, st.stopped, st.live, tt, to, ti, err, _this_stream())


def check_ledidi_err(err):
    """Raise if svdd_ledidi_step flagged a start token > 3 (SVDD_E_ARG)."""
    if int(err[0]) != 0:
        _lib.check(_lib.E_ARG, "svdd_ledidi_step: a start sequence holds a token > 3")


KMER_MAX_K, PACK_MAX_L = 6, 1024                                          # svdd_kmer_counts / svdd_pack_tokens (include/svdd_hip.h)
NN_KEY_INIT = -1                                                         # all ones: the value svdd_hamming_nn's nn_key starts from


def _tokens2d(x, name="x"):
    x = _need(x, torch.uint8, name)
    if x.dim() != 2 or not x.is_contiguous() or x.numel() == 0:
        raise SvddError(f"{name} must be a contiguous non-empty u8 [N, L] tensor, got {tuple(x.shape)}")
    return x


def kmer_counts(x, k, counts, skipped=None):
    """svdd_kmer_counts: ADD the k-mer counts of x u8 [N, L] to counts i64 [4^k] (bin = the lexicographic rank of the ACGT string)
    and the number of windows that hold a token > 3 to skipped i64 [1] (or None). Both are the caller's and start from what they
    hold. k > L: no windows, nothing written."""
    if not isinstance(k, int) or isinstance(k, bool) or not 1 <= k <= KMER_MAX_K:
        raise ValueError(f"k = {k!r}: expected an int in 1 .. {KMER_MAX_K}")
    x = _tokens2d(x)
    _is(counts, torch.int64, (4 ** k,), "counts")
    if skipped is not None:
        _is(skipped, torch.int64, (1,), "skipped")
    _lib.call("svdd_kmer_counts", x, x.shape[0], x.shape[1], k, counts, skipped, _this_stream())
    return counts, skipped


def packed_words(L):
    return (int(L) + 15) // 16


def pack_tokens(x, packed=None, err=None):
    """svdd_pack_tokens: x u8 [N, L] (tokens 0..3, L <= 1024) -> packed int32 [N, ceil(L / 16)] (the bits of the u32 words: position
    l in word l // 16 at bits 2 (l % 16); padding bits zero). err: a caller-zeroed device int32 [1] the kernel sets for a token > 3
    (checked by the caller later with check_pack_err); None: checked here (one synchronisation)."""
    x = _tokens2d(x)
    N, L = x.shape
    if L > PACK_MAX_L:
        raise SvddError(f"pack_tokens: L = {L} > {PACK_MAX_L}")
    W = packed_words(L)
    packed = torch.empty((N, W), dtype=torch.int32, device=x.device) if packed is None else _is(packed, torch.int32, (N, W), "packed")
    check_here = err is None
    if check_here:
        err = torch.zeros(1, dtype=torch.int32, device=x.device)
    else:
        _is(err, torch.int32, (1,), "err")
    _lib.call("svdd_pack_tokens", x, N, L, packed, err, _this_stream())
    if check_here:
        check_pack_err(err)
    return packed


def check_pack_err(err):
    """Raise if svdd_pack_tokens flagged a token > 3 (SVDD_E_ARG)."""
    if int(err[0]) != 0:
        _lib.check(_lib.E_ARG, "svdd_pack_tokens: a row holds a token > 3 (MASK included)")


def hamming_nn(q, db, L, nn_key=None, hist=None, q_base=0, db_base=0, exclude_diag=False):
    """svdd_hamming_nn on packed rows (pack_tokens): q int32 [B, W], db int32 [N, W], W = ceil(L / 16). nn_key i64 [B] (or None),
    started by the caller at NN_KEY_INIT, is lowered to (distance << 32) | (db_base + j) of the nearest database row (the lowest
    index among ties); hist i64 [L + 1] (or None) is ADDED the number of pairs at each distance. exclude_diag: the pairs with
    q_base + i == db_base + j are left out. Decode a key with nn_decode."""
    W = packed_words(L)
    if not 1 <= int(L) <= PACK_MAX_L:
        raise SvddError(f"hamming_nn: L = {L} outside 1 .. {PACK_MAX_L}")
    _need(q, torch.int32, "q"), _need(db, torch.int32, "db")
    if q.dim() != 2 or db.dim() != 2 or q.shape[1] != W or db.shape[1] != W or not q.is_contiguous() or not db.is_contiguous() \
            or q.shape[0] == 0 or db.shape[0] == 0:
        raise SvddError(f"hamming_nn: q and db must be contiguous non-empty int32 [*, {W}] tensors, got {tuple(q.shape)} and {tuple(db.shape)}")
    B, N = q.shape[0], db.shape[0]
    if nn_key is None and hist is None:
        raise SvddError("hamming_nn: give nn_key, hist or both")
    if nn_key is not None:
        _is(nn_key, torch.int64, (B,), "nn_key")
    if hist is not None:
        _is(hist, torch.int64, (int(L) + 1,), "hist")
    _lib.call("svdd_hamming_nn", q, db, B, N, int(L), int(q_base), int(db_base), int(bool(exclude_diag)), nn_key, hist, _this_stream())
    return nn_key, hist


def edit_nn(q, db, Lq, Ld, cap, nn_key=None, hist=None, q_base=0, db_base=0, exclude_diag=False):
    """svdd_edit_nn on packed rows (pack_tokens): q int32 [B, ceil(Lq / 16)], db int32 [N, ceil(Ld / 16)]; the Levenshtein distance
    of every pair, cap in 0 .. max(Lq, Ld). nn_key i64 [B] (or None), started by the caller at NN_KEY_INIT or at any earlier key, is
    lowered to (distance << 32) | (db_base + j) of the nearest database row within cap (the lowest index among ties; a pair beyond
    cap never touches it); hist i64 [cap + 2] (or None) is ADDED the number of pairs at each distance 0 .. cap and, in its last
    bin, the pairs beyond. exclude_diag: the pairs with q_base + i == db_base + j are left out. Decode a key with nn_decode."""
    Lq, Ld = int(Lq), int(Ld)
    if not 1 <= Lq <= PACK_MAX_L or not 1 <= Ld <= PACK_MAX_L:
        raise SvddError(f"edit_nn: Lq = {Lq}, Ld = {Ld} outside 1 .. {PACK_MAX_L}")
    if not isinstance(cap, int) or isinstance(cap, bool) or not 0 <= cap <= max(Lq, Ld):
        raise SvddError(f"edit_nn: cap = {cap!r} outside 0 .. max(Lq, Ld) = {max(Lq, Ld)}")
    Wq, Wd = packed_words(Lq), packed_words(Ld)
    _need(q, torch.int32, "q"), _need(db, torch.int32, "db")
    if q.dim() != 2 or db.dim() != 2 or q.shape[1] != Wq or db.shape[1] != Wd or not q.is_contiguous() or not db.is_contiguous() \
            or q.shape[0] == 0 or db.shape[0] == 0:
        raise SvddError(f"edit_nn: q and db must be contiguous non-empty int32 [*, {Wq}] and [*, {Wd}] tensors, got {tuple(q.shape)} "
                        f"and {tuple(db.shape)}")
    B, N = q.shape[0], db.shape[0]
    if nn_key is None and hist is None:
        raise SvddError("edit_nn: give nn_key, hist or both")
    if nn_key is not None:
        _is(nn_key, torch.int64, (B,), "nn_key")
    if hist is not None:
        _is(hist, torch.int64, (cap + 2,), "hist")
    _lib.call("svdd_edit_nn", q, db, B, N, Lq, Ld, cap, int(q_base), int(db_base), int(bool(exclude_diag)), nn_key, hist, _this_stream())
    return nn_key, hist


def nn_decode(nn_key):
    """nn_key i64 [B] of hamming_nn -> (dist i32 [B], idx i64 [B]); a key nobody lowered (no pair) gives (-1, -1)."""
    none = nn_key == NN_KEY_INIT
    dist = torch.where(none, torch.full_like(nn_key, -1), nn_key >> 32).to(torch.int32)
    idx = torch.where(none, torch.full_like(nn_key, -1), nn_key & 0xFFFFFFFF)
    return dist, idx


FIRST_INIT = 2 ** 31 - 1                                                 # INT32_MAX: the value svdd_within's `first` starts from
PICK_MAX_ROWS = 4096                                                     # rows of one svdd_greedy_pick block (include/svdd_hip.h)


def _int_in(v, lo, hi, what):
    if not isinstance(v, int) or isinstance(v, bool) or not lo <= v <= hi:
        raise SvddError(f"{what} = {v!r} outside {lo} .. {hi}")
    return v


def within(q, db, L, radius, q_rc=None, db_count=None, first=None, mask=None):
    """svdd_within on packed rows (pack_tokens): q int32 [B, W], db int32 [N, W], W = ceil(L / 16); q_rc int32 [B, W] (or None): the
    packed reverse complements of q's rows, which makes the distance the smaller of the two strands'. A pair is a hit when its
    distance is <= radius (0 .. L - 1). db_count int32 [1] on the device (or None): only the rows j < min(N, db_count) exist.
    first int32 [B] (or None), started by the caller at FIRST_INIT, is lowered to the lowest hit; mask int32 [B, mask_words] (or
    None), mask_words >= ceil(N / 32), is WRITTEN in full: bit j of row i = (i, j) is a hit."""
    L = _int_in(L, 1, PACK_MAX_L, "within: L")
    radius = _int_in(radius, 0, L - 1, "within: radius")
    W = packed_words(L)
    _need(q, torch.int32, "q"), _need(db, torch.int32, "db")
    if q.dim() != 2 or db.dim() != 2 or q.shape[1] != W or db.shape[1] != W or not q.is_contiguous() or not db.is_contiguous() \
            or q.shape[0] == 0 or db.shape[0] == 0:
        raise SvddError(f"within: q and db must be contiguous non-empty int32 [*, {W}] tensors, got {tuple(q.shape)} and {tuple(db.shape)}")
    B, N = q.shape[0], db.shape[0]
    if q_rc is not None:
        _is(q_rc, torch.int32, (B, W), "q_rc")
    if db_count is not None:
        _is(db_count, torch.int32, (1,), "db_count")
    if first is None and mask is None:
        raise SvddError("within: give first, mask or both")
    if first is not None:
        _is(first, torch.int32, (B,), "first")
    mask_words = 0
    if mask is not None:
        _need(mask, torch.int32, "mask")
        if mask.dim() != 2 or mask.shape[0] != B or mask.shape[1] * 32 < N or not mask.is_contiguous():
            raise SvddError(f"within: mask must be a contiguous int32 [{B}, >= {(N + 31) // 32}] tensor, got {tuple(mask.shape)}")
        mask_words = mask.shape[1]
    _lib.call("svdd_within", q, q_rc, db, db_count, B, N, L, radius, first, mask, mask_words, _this_stream())
    return first, mask


def greedy_pick(mask, first, rows, L, base, k, count, reps, picked_rank, rep_pick):
    """svdd_greedy_pick: the serial walk of greedy selection over one block of T <= PICK_MAX_ROWS rows in rank order. mask int32
    [T, >= ceil(T / 32)] (within of the block against itself), first int32 [T] (or None; within of the block against reps), rows
    int32 [T, W] the block's packed rows, base the rank of its first row, k >= 1 the number of picks wanted. State, advanced in
    place: count int32 [1], reps int32 [cap, W], picked_rank int32 [cap]. rep_pick int32 [T] is WRITTEN: the number of the pick
    that represents each row (its own if it is picked), -1 for a row that is left over once min(k, cap) picks exist."""
    L = _int_in(L, 1, PACK_MAX_L, "greedy_pick: L")
    k = _int_in(k, 1, 2 ** 31 - 1, "greedy_pick: k")
    base = _int_in(base, 0, 2 ** 31 - 1, "greedy_pick: base")
    W = packed_words(L)
    _need(rows, torch.int32, "rows")
    if rows.dim() != 2 or rows.shape[1] != W or not rows.is_contiguous() or not 1 <= rows.shape[0] <= PICK_MAX_ROWS:
        raise SvddError(f"greedy_pick: rows must be a contiguous int32 [1 .. {PICK_MAX_ROWS}, {W}] tensor, got {tuple(rows.shape)}")
    T = rows.shape[0]
    _int_in(base, 0, 2 ** 31 - 1 - T, "greedy_pick: base")
    _need(mask, torch.int32, "mask")
    if mask.dim() != 2 or mask.shape[0] != T or mask.shape[1] * 32 < T or not mask.is_contiguous():
        raise SvddError(f"greedy_pick: mask must be a contiguous int32 [{T}, >= {(T + 31) // 32}] tensor, got {tuple(mask.shape)}")
    if first is not None:
        _is(first, torch.int32, (T,), "first")
    _is(count, torch.int32, (1,), "count")
    _need(reps, torch.int32, "reps")
    if reps.dim() != 2 or reps.shape[1] != W or reps.shape[0] == 0 or not reps.is_contiguous():
        raise SvddError(f"greedy_pick: reps must be a contiguous non-empty int32 [cap, {W}] tensor, got {tuple(reps.shape)}")
    cap = reps.shape[0]
    _is(picked_rank, torch.int32, (cap,), "picked_rank"), _is(rep_pick, torch.int32, (T,), "rep_pick")
    _lib.call("svdd_greedy_pick", mask, mask.shape[1], first, rows, T, L, base, k, count, reps, picked_rank, cap, rep_pick, _this_stream())
    return rep_pick


def edit_within(q, db, L, radius, both_strands=False, db_count=None, first=None, mask=None):
    """svdd_edit_within on packed rows (pack_tokens) of one length: q int32 [B, W], db int32 [N, W], W = ceil(L / 16). A pair is a
    hit when its Levenshtein distance (with both_strands: the smaller of that and the distance of the query's reverse complement)
    is <= radius (0 .. L - 1). db_count, first and mask as for within: db_count int32 [1] on the device (or None): only the rows
    j < min(N, db_count) exist; first int32 [B] (or None), started by the caller at FIRST_INIT, is lowered to the lowest hit; mask
    int32 [B, mask_words] (or None), mask_words >= ceil(N / 32), is WRITTEN in full: bit j of row i = (i, j) is a hit."""
    L = _int_in(L, 1, PACK_MAX_L, "edit_within: L")
    radius = _int_in(radius, 0, L - 1, "edit_within: radius")
    W = packed_words(L)
    _need(q, torch.int32, "q"), _need(db, torch.int32, "db")
    if q.dim() != 2 or db.dim() != 2 or q.shape[1] != W or db.shape[1] != W or not q.is_contiguous() or not db.is_contiguous() \
            or q.shape[0] == 0 or db.shape[0] == 0:
        raise SvddError(f"edit_within: q and db must be contiguous non-empty int32 [*, {W}] tensors, got {tuple(q.shape)} and "
                        f"{tuple(db.shape)}")
    B, N = q.shape[0], db.shape[0]
    if db_count is not None:
        _is(db_count, torch.int32, (1,), "db_count")
    if first is None and mask is None:
        raise SvddError("edit_within: give first, mask or both")
    if first is not None:
        _is(first, torch.int32, (B,), "first")
    mask_words = 0
    if mask is not None:
        _need(mask, torch.int32, "mask")
        if mask.dim() != 2 or mask.shape[0] != B or mask.shape[1] * 32 < N or not mask.is_contiguous():
            raise SvddError(f"edit_within: mask must be a contiguous int32 [{B}, >= {(N + 31) // 32}] tensor, got {tuple(mask.shape)}")
        mask_words = mask.shape[1]
    _lib.call("svdd_edit_within", q, db, db_count, B, N, L, radius, int(bool(both_strands)), first, mask, mask_words, _this_stream())
    return first, mask


def edit_pairs(q, db, idx, Lq, Ld, cap, both_strands=False, dist=None):
    """svdd_edit_pairs on packed rows (pack_tokens): q int32 [B, ceil(Lq / 16)], db int32 [N, ceil(Ld / 16)], idx int32 [B] -> dist
    int32 [B], WRITTEN in full: the Levenshtein distance of q's row i and db's row idx[i] (with both_strands: the smaller of that
    and the distance of the query's reverse complement), -1 where idx[i] is outside 0 .. N - 1 or the distance exceeds cap
    (0 .. max(Lq, Ld))."""
    Lq = _int_in(Lq, 1, PACK_MAX_L, "edit_pairs: Lq")
    Ld = _int_in(Ld, 1, PACK_MAX_L, "edit_pairs: Ld")
    cap = _int_in(cap, 0, max(Lq, Ld), "edit_pairs: cap")
    Wq, Wd = packed_words(Lq), packed_words(Ld)
    _need(q, torch.int32, "q"), _need(db, torch.int32, "db")
    if q.dim() != 2 or db.dim() != 2 or q.shape[1] != Wq or db.shape[1] != Wd or not q.is_contiguous() or not db.is_contiguous() \
            or q.shape[0] == 0 or db.shape[0] == 0:
        raise SvddError(f"edit_pairs: q and db must be contiguous non-empty int32 [*, {Wq}] and [*, {Wd}] tensors, got "
                        f"{tuple(q.shape)} and {tuple(db.shape)}")
    B, N = q.shape[0], db.shape[0]
    _is(idx, torch.int32, (B,), "idx")
    dist = torch.empty(B, dtype=torch.int32, device=q.device) if dist is None else _is(dist, torch.int32, (B,), "dist")
    _lib.call("svdd_edit_pairs", q, db, idx, B, N, Lq, Ld, cap, int(bool(both_strands)), dist, _this_stream())
    return dist


MOTIF_MAX_W = 32                                                      # svdd_motif_scan (include/svdd_hip.h)


@dataclass
class MotifTables:
    """A motif set on the device, as svdd_motif_scan reads it: pwm i16 [M, 32, 4] (A, C, G, T), width i32 [M], threshold i32 [M].
    Built by motifs.MotifSet.to_device, which has checked the widths (the kernel only clamps them)."""
    pwm: torch.Tensor
    width: torch.Tensor
    threshold: torch.Tensor


def motif_scan(packed, L, mset_dev, both_strands=True, hits=None, rows_hit=None, row_hits=None, row_best=None):
    """svdd_motif_scan on packed rows (pack_tokens): packed int32 [N, ceil(L / 16)], mset_dev a MotifTables of M motifs. hits and
    rows_hit i64 [M] are ADDED the hits / the rows with a hit; row_hits i32 [N, M] and row_best i64 [N, M] (decode: motif_best_decode)
    are written. Any of the four may be None, not all. -> (hits, rows_hit, row_hits, row_best)."""
    if not 1 <= int(L) <= PACK_MAX_L:
        raise SvddError(f"motif_scan: L = {L} outside 1 .. {PACK_MAX_L}")
    if not isinstance(mset_dev, MotifTables):
        raise SvddError(f"motif_scan: mset_dev must be an ops.MotifTables (motifs.MotifSet.to_device), got {type(mset_dev).__name__}")
    W = packed_words(L)
    _need(packed, torch.int32, "packed")
    if packed.dim() != 2 or packed.shape[1] != W or packed.shape[0] == 0 or not packed.is_contiguous():
        raise SvddError(f"motif_scan: packed must be a contiguous non-empty int32 [N, {W}] tensor, got {tuple(packed.shape)}")
    N = packed.shape[0]
    _need(mset_dev.width, torch.int32, "width")
    M = mset_dev.width.numel()
    if M == 0:
        raise SvddError("motif_scan: an empty motif set")
    _is(mset_dev.width, torch.int32, (M,), "width")
    _is(mset_dev.threshold, torch.int32, (M,), "threshold")
    _is(mset_dev.pwm, torch.int16, (M, MOTIF_MAX_W, 4), "pwm")
    if hits is None and rows_hit is None and row_hits is None and row_best is None:
        raise SvddError("motif_scan: give at least one of hits, rows_hit, row_hits, row_best")
    if hits is not None:
        _is(hits, torch.int64, (M,), "hits")
    if rows_hit is not None:
        _is(rows_hit, torch.int64, (M,), "rows_hit")
    if row_hits is not None:
        _is(row_hits, torch.int32, (N, M), "row_hits")
    if row_best is not None:
        _is(row_best, torch.int64, (N, M), "row_best")
    _lib.call("svdd_motif_scan", packed, N, int(L), mset_dev.pwm, mset_dev.width, mset_dev.threshold, M, int(bool(both_strands)),
              hits, rows_hit, row_hits, row_best, _this_stream())
    return hits, rows_hit, row_hits, row_best


def motif_best_decode(row_best):
    """row_best i64 [...] of motif_scan -> (score i32, start i32, strand i8): strand 0 forward, 1 reverse; a key of 0 (no window:
    L < w) gives (INT32_MIN, -1, -1)."""
    none = row_best == 0
    score = (((row_best >> 32) & 0xFFFFFFFF) - (1 << 31)).to(torch.int32)
    where = ~row_best & 0xFFFFFFFF                                         # 2 start + strand
    start = torch.where(none, torch.full_like(where, -1), where >> 1).to(torch.int32)
    strand = torch.where(none, torch.full_like(where, -1), where & 1).to(torch.int8)
    return score, start, strand


@dataclass
class MotifCoefs:
    """The per-motif integer coefficients of svdd_motif_reward on the device, int32 [M] each: hit_coef, hit_cap (>= 0), margin_coef,
    margin_floor (>= 0). Built by motifs.MotifReward.to_device, which has checked the signs and the int64 bound."""
    hit_coef: torch.Tensor
    hit_cap: torch.Tensor
    margin_coef: torch.Tensor
    margin_floor: torch.Tensor


def motif_reward(tok, mset_dev, coefs, unit, count=None, base=None, out=None, term=None, err=None, both_strands=True):
    """svdd_motif_reward: tok u8 [n, L] (finished rows, L <= 1024), mset_dev a MotifTables of M motifs, coefs a MotifCoefs, unit a
    float -> (out f32 [n] | None, term i64 [n] | None): out[r] = base[r] + float(T(r)) * unit and term[r] = T(r), the integer motif
    term of include/svdd_hip.h. count: int32 device tensor [1], rows >= count[0] are neither read nor written (None: all rows).
    base f32 [n] or None (0); out may be base itself. out = None allocates it unless term is given (term only). err: a caller-zeroed
    device int32 [1] the kernel sets for a token > 3 (checked by the caller later with check_pack_err); None: not reported."""
    if not isinstance(mset_dev, MotifTables):
        raise SvddError(f"motif_reward: mset_dev must be an ops.MotifTables (motifs.MotifSet.to_device), got {type(mset_dev).__name__}")
    if not isinstance(coefs, MotifCoefs):
        raise SvddError(f"motif_reward: coefs must be an ops.MotifCoefs (motifs.MotifReward.to_device), got {type(coefs).__name__}")
    if isinstance(unit, torch.Tensor) or not isinstance(unit, (int, float)) or isinstance(unit, bool) or not 0.0 < float(unit) < float("inf"):
        raise SvddError(f"motif_reward: unit = {unit!r}: expected a positive finite number")
    tok = _tokens2d(tok, "tok")
    n, L = tok.shape
    if L > PACK_MAX_L:
        raise SvddError(f"motif_reward: L = {L} outside 1 .. {PACK_MAX_L}")
    _need(mset_dev.width, torch.int32, "width")
    M = mset_dev.width.numel()
    if M == 0:
        raise SvddError("motif_reward: an empty motif set")
    _is(mset_dev.width, torch.int32, (M,), "width")
    _is(mset_dev.threshold, torch.int32, (M,), "threshold")
    _is(mset_dev.pwm, torch.int16, (M, MOTIF_MAX_W, 4), "pwm")
    for name in ("hit_coef", "hit_cap", "margin_coef", "margin_floor"):
        _is(getattr(coefs, name), torch.int32, (M,), name)
    if count is not None:
        _is(count, torch.int32, (1,), "count")
    if base is not None:
        _is(base, torch.float32, (n,), "base")
    if term is not None:
        _is(term, torch.int64, (n,), "term")
    if err is not None:
        _is(err, torch.int32, (1,), "err")
    if out is None and term is None:
        out = torch.empty(n, dtype=torch.float32, device=tok.device)
    elif out is not None:
        _is(out, torch.float32, (n,), "out")
    _lib.call("svdd_motif_reward", tok, n, L, count, mset_dev.pwm, mset_dev.width, mset_dev.threshold, M, int(bool(both_strands)),
              coefs.hit_coef, coefs.hit_cap, coefs.margin_coef, coefs.margin_floor, base, float(unit), out, term, err, _this_stream())
    return out, term


def select(scores, cand, mode=SELECT_ARGMAX, rng=None, want_soft=True, x_next=None):
    """-> (x_next u8 [B,L], soft f32 [B,M] | None, idx i32 [B])."""
    cand = _need(cand, torch.uint8, "cand").contiguous()
    B, M, L = cand.shape
    scores = _need(scores, torch.float32, "scores").contiguous()
    assert scores.numel() == B * M, (scores.shape, cand.shape)
    if x_next is None:
        x_next = torch.empty((B, L), dtype=torch.uint8, device=cand.device)
    soft = torch.empty((B, M), dtype=torch.float32, device=cand.device) if want_soft else None
    idx = torch.empty((B,), dtype=torch.int32, device=cand.device)
    rs = rng.c_struct() if rng is not None else None
    _lib.call("svdd_select", scores, cand, B, L, M, mode, ctypes.byref(rs) if rs is not None else None, x_next, soft, idx)
    return x_next, soft, idx


def select_compact(scores_c, slot, parent_score, cand, mode=SELECT_ARGMAX, rng=None, x_next=None, sel_score=None,
                   changed=None, idx=None):
    """svdd_select_compact: select on the scores of the LIVE candidates only. scores_c f32 [>= count] (compacted),
    slot i32 [B*M] (position in scores_c, or -1 for a copy of the parent), parent_score f32 [B].
    -> (x_next u8 [B,L], idx i32 [B], sel_score f32 [B], changed i32 [B])."""
    cand = _need(cand, torch.uint8, "cand").contiguous()
    B, M, L = cand.shape
    dev = cand.device
    scores_c = _need(scores_c, torch.float32, "scores").contiguous()
    x_next = torch.empty((B, L), dtype=torch.uint8, device=dev) if x_next is None else x_next
    idx = torch.empty((B,), dtype=torch.int32, device=dev) if idx is None else idx
    sel_score = torch.empty((B,), dtype=torch.float32, device=dev) if sel_score is None else sel_score
    changed = torch.empty((B,), dtype=torch.int32, device=dev) if changed is None else changed
    rs = rng.c_struct() if rng is not None else None
    _lib.call("svdd_select_compact", scores_c, slot, parent_score, cand, B, L, M, mode, ctypes.byref(rs) if rs is not None else None,
              x_next, None, idx, sel_score, changed)
    return x_next, idx, sel_score, changed


def compact_flags(flags, live_idx, slot, count):
    """Stable device-side compaction (svdd_compact_flags): live_idx[k] = i, slot[i] = k for the k-th non-zero flag,
    slot[i] = -1 otherwise, count[0] = number of non-zero flags. All int32 device tensors; nothing returns to the host."""
    _lib.call("svdd_compact_flags", flags, flags.numel(), live_idx, slot, count)


def compact_by_key(key, live_idx, slot, count, split=0):
    """The same compaction ordered by key, largest first, stable inside a key (svdd_compact_by_key): key[i] > 0 = live.
    split > 0: count has 3 entries and also receives the lengths of the list's parts [0, split) and [split, ...)."""
    assert split == 0 or count.numel() >= 3
    _lib.call("svdd_compact_by_key", key, key.numel(), live_idx, slot, count, int(split))


def gather_rows(src, idx, count, dst):
    """dst[i] = src[idx[i]] for i < count[0] (row tensors of equal row size, contiguous)."""
    n = src.shape[0]
    row_bytes = src[0].numel() * src.element_size()
    _lib.call("svdd_gather_rows", src, idx, count, n, row_bytes, dst)
    return dst


def advance_rows(src, slot, sel, dst, M):
    """The selected candidate becomes the next parent: dst[b] = src[slot[b*M + sel[b]]] where that slot is >= 0."""
    B = dst.shape[0]
    row_bytes = dst[0].numel() * dst.element_size()
    _lib.call("svdd_advance_rows", src, slot, sel, B, M, row_bytes, dst)
    return dst


def x0hat(logits, xt, want_tokens=False, want_onehot=True):
    """-> (onehot_t f32 [R,4,L] | None, x0hat u8 [R,L] | None)."""
    logits = _need(logits, torch.float32, "logits")
    xt = _need(xt, torch.uint8, "xt").contiguous()
    R, L = xt.shape
    logits, layout = layout_of(logits)
    oh = torch.empty((R, 4, L), dtype=torch.float32, device=xt.device) if want_onehot else None
    xh = torch.empty((R, L), dtype=torch.uint8, device=xt.device) if want_tokens else None
    _lib.call("svdd_x0hat", logits, xt, R, L, layout, oh, xh)
    return oh, xh


def finalize(logits, x):
    """Noise-removal argmax -> int64 [B,L] (the API's LongTensor)."""
    logits = _need(logits, torch.float32, "logits")
    x = _need(x, torch.uint8, "x").contiguous()
    B, L = x.shape
    logits, layout = layout_of(logits)
    out = torch.empty((B, L), dtype=torch.int64, device=x.device)
    _lib.call("svdd_finalize", logits, x, B, L, layout, out, None)
    return out


def transform_samples(tok, transposed=False):
    """tokens u8 [R,L] -> one-hot f32 [R,L,4] (or [R,4,L]); MASK rows are zero."""
    tok = _need(tok, torch.uint8, "tok").contiguous()
    R, L = tok.shape
    out = torch.empty((R, 4, L) if transposed else (R, L, 4), dtype=torch.float32, device=tok.device)
    _lib.call("svdd_transform_samples", tok, R, L, int(bool(transposed)), out)
    return out


def subs_logp(logits, x):
    """Diffusion.forward()'s SUBS re-parameterisation -> log p(x0|xt), same strides as logits."""
    logits = _need(logits, torch.float32, "logits")
    x = _need(x, torch.uint8, "x").contiguous()
    B, L = x.shape
    logits, layout = layout_of(logits)
    out = _empty_like_layout(logits, layout)
    _lib.call("svdd_subs_logp", logits, x, B, L, layout, out)
    return out


def dps_probs(logits, x):
    """softmax(E)[..., 0:4] of a DPS step, E = keep * onehot(x) + (1 - keep) * log p(x0 | x) (reference diffusion_gosai.py:1325-1328):
    logits fp32 [B, L, 5] contiguous (the backbone's raw output), x u8 [B, L] -> fp32 [B, L, 4], the reward net's input."""
    logits = _need(logits, torch.float32, "logits")
    x = _need(x, torch.uint8, "x").contiguous()
    assert logits.is_contiguous() and logits.shape == (*x.shape, 5)
    B, L = x.shape
    out = torch.empty((B, L, 4), dtype=torch.float32, device=x.device)
    _lib.call("svdd_dps_probs", logits, x, B, L, out)
    return out


def dps_probs_bwd(logits, x, dprobs4):
    """d loss / d probs4 [B, L, 4] -> (d loss / d logits [B, L, 5] — what the backbone's gradient kernel takes; zero at unmasked
    positions — , direct [B, L, 5] = the gradient through `keep * x_onehot`, zero at masked positions)."""
    x = _need(x, torch.uint8, "x").contiguous()
    B, L = x.shape
    g = dprobs4.contiguous().float()
    assert logits.is_contiguous() and logits.shape == (B, L, 5) and g.shape == (B, L, 4)
    dlogits = torch.empty((B, L, 5), dtype=torch.float32, device=x.device)
    direct = torch.empty_like(dlogits)
    _lib.call("svdd_dps_probs_bwd", logits, x, g, B, L, dlogits, direct)
    return dlogits, direct


def dps_guided_q(logits, x, grad_backbone, grad_direct, dm, mcs, scale):
    """The guided transition weights of a DPS step (reference :1306-1314): exp(log p) * dm with q[MASK] = mcs, times
    exp(scale * (x_grad - x_grad[MASK])), x_grad = grad_backbone + grad_direct -> fp32 [B, L, 5]."""
    x = _need(x, torch.uint8, "x").contiguous()
    B, L = x.shape
    gb, gd = grad_backbone.contiguous().float(), grad_direct.contiguous().float()
    assert logits.is_contiguous() and logits.shape == (B, L, 5) and gb.shape == (B, L, 5) and gd.shape == (B, L, 5)
    q = torch.empty((B, L, 5), dtype=torch.float32, device=x.device)
    _lib.call("svdd_dps_guided_q", logits, x, gb, gd, float(dm), float(mcs), float(scale), B, L, q)
    return q


def tds_resample(reward_num, reward_den, alpha, sample, u):
    """-> (x_next u8 [B,L], idx i32 [B]); u = the B float64 uniforms np.random.choice consumes."""
    num = _need(reward_num, torch.float32, "reward_num").contiguous()
    den = _need(reward_den, torch.float32, "reward_den").contiguous()
    sample = _need(sample, torch.uint8, "sample").contiguous()
    u = _need(u, torch.float64, "u").contiguous()
    B, L = sample.shape
    assert num.numel() == B and den.numel() == B and u.numel() == B
    x_next = torch.empty_like(sample)
    idx = torch.empty((B,), dtype=torch.int32, device=sample.device)
    work = torch.empty((2 * B,), dtype=torch.float64, device=sample.device)
    _lib.call("svdd_tds_resample", num, den, float(alpha), sample, u, B, L, x_next, idx, work)
    return x_next, idx


# ------------------------------------------------------------------------------------------------ replay RNG on the device
_TORCH_STATE_BYTES = 5056       # THGeneratorState: u64 seed | i32 left | i32 seeded | u64 next | u64 state[624] | 3 doubles + i32 (Box-Muller cache)


def mt_state_from_torch(state_u8):
    """torch.get_rng_state() (CPU generator, the legacy 5056-byte layout) -> int64 numpy [625]: 624 words + pos.
    at::mt19937 draws with `if (--left == 0) next_state(); y = state[next++]`: pos = 625 - left (manual_seed leaves left = 1:
    pos = 624, twist first)."""
    import numpy as np
    a = state_u8.numpy() if isinstance(state_u8, torch.Tensor) else np.asarray(state_u8)
    if a.size != _TORCH_STATE_BYTES or not int(a[12:16].view(np.int32)[0]):
        raise SvddError("unexpected torch CPU generator state layout (want the 5056-byte mt19937 state, seeded)")
    left = int(a[8:12].view(np.int32)[0])
    words = a[24:24 + 624 * 8].view(np.uint64)
    if not (1 <= left <= 624) or int(words.max()) >> 32:
        raise SvddError("unexpected torch CPU generator state contents")
    out = np.empty(625, dtype=np.int64)
    out[:624] = words
    out[624] = 625 - left
    return out


def mt_state_to_torch(words_pos, template_u8):
    """Inverse: [625] (624 words + pos) -> a 5056-byte torch CPU generator state (seed and the Box-Muller cache of
    `template_u8` kept)."""
    import numpy as np
    a = np.array(template_u8.numpy() if isinstance(template_u8, torch.Tensor) else template_u8, dtype=np.uint8, copy=True)
    pos = int(words_pos[624])
    if not 1 <= pos <= 624:      # (the kernel returns pos in [1, 624] whenever it drew anything: left = 625 - pos in [1, 624])
        raise SvddError(f"mt19937 state with pos = {pos} has no torch representation")
    a[8:12].view(np.int32)[0] = 625 - pos
    a[16:24].view(np.uint64)[0] = pos
    a[24:24 + 624 * 8].view(np.uint64)[:] = np.asarray(words_pos[:624], dtype=np.uint64)
    return torch.from_numpy(a)


# ---- side streams, process-wide -----------------------------------------------------------------------------------------------
# Every component that runs parts of a step concurrently (the C4 trunk's two chains, the late steps' second GRU part, the SVDD-PM
# two-part step, the device replay generator) takes its side streams from ONE list per device, for the life of the process.
# Why a list and a test (round 6, tools/c4_stream_probe.py, profiles/r06_c4_stream_probe.txt): HIP maps streams onto FOUR hardware
# queues, in the order in which they are first used, and two streams on one hardware queue do not run concurrently — nor does a side
# stream that shares the queue of the stream the decode itself runs on. Which queue a stream got used to depend on how many streams
# anything in the process had touched before: the C4 trunk's two chains measured 65 instead of 80 seq/s whenever 4 k other streams
# had been used first, and bench.py's C4 leg lost 20 % in round 6 when an earlier leg stopped creating a stream per decode.
# side_stream() therefore PROBES its candidates once: a candidate is kept only if a marker on it is not held up by a sleeping kernel
# on the current stream, nor by one on a candidate already kept (same hardware queue = in-order = the marker waits). ~10 ms, once.
_SIDE_STREAMS = {}
SIDE_SLOTS = 3                                        # three other hardware queues exist beside the main stream's
SIDE_TRUNK_A, SIDE_TRUNK_B, SIDE_REPLAY = 0, 1, 2     # who uses which slot (the split GRU / PM paths share slot 0)


def _held_up_by(busy, cand, ms=0.4):
    """True when a marker on stream `cand` has to wait for a sleeping kernel on stream `busy` (they share a hardware queue)."""
    e0, e1, ec = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    torch.cuda.synchronize()
    e0.record(busy)
    with torch.cuda.stream(busy):
        torch.cuda._sleep(int(ms * 2.0e6))            # ~ms at 2 GHz
    e1.record(busy)
    ec.record(cand)
    torch.cuda.synchronize()
    return e0.elapsed_time(ec) > 0.5 * e0.elapsed_time(e1)


def _probe_side_streams(dev, want):
    import os
    cur = torch.cuda.current_stream(dev)
    kept, tried = [], 0
    probe = os.environ.get("SVDD_SIDE_STREAM_PROBE", "1") != "0" and not torch.cuda.is_current_stream_capturing()
    while len(kept) < want and tried < 12:
        st = torch.cuda.Stream(device=dev)
        tried += 1
        with torch.cuda.stream(st):
            torch.zeros(1, device=dev)                # first use: this is when HIP binds the stream to a hardware queue
        try:
            if probe and (_held_up_by(cur, st) or any(_held_up_by(k, st) for k in kept)):
                continue
        except Exception:                             # noqa: BLE001  (no _sleep in this build, ...): take the streams as they come
            probe = False
        kept.append(st)
    while len(kept) < want:                           # fewer free hardware queues than slots: the remaining slots share
        kept.append(kept[len(kept) % max(len(kept), 1)] if kept else torch.cuda.Stream(device=dev))
    return kept


def side_stream(device, slot=0):
    """The `slot`-th side stream of `device` (slots 0 .. SIDE_SLOTS - 1; made and probed at the first call, never destroyed)."""
    dev = torch.device(device)
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    if key not in _SIDE_STREAMS:
        _SIDE_STREAMS[key] = _probe_side_streams(torch.device("cuda", key), SIDE_SLOTS)
    return _SIDE_STREAMS[key][slot % SIDE_SLOTS]


class DeviceReplayStream:
    """torch's global CPU generator continued ON THE DEVICE for the span of one decode (rng_mode = "replay"): the state
    (2.5 KB) is uploaded at open(), `uniforms(n)` returns the next n floats of the stream as a device tensor (K8
    `svdd_mt19937_uniform_f32`: one workgroup, launched on a side stream ONE CALL AHEAD so that it runs under the nets of the
    current diffusion step), and close() writes the advanced state back into torch's generator — after it, torch.rand() on
    the host continues exactly where the reference's run would. Token-exact with the host replay (tests/test_kernels_gpu.py).
    Contract: between open and close() nothing else may draw from torch's CPU generator (the reference's eval-mode hot path does
    not either: rand_like in _sample_categorical is its only consumer); a value function that did (dropout in
    train mode) would see the pre-decode state — use Diffusion.replay_rng = "host" for such a net."""

    def __init__(self, device):
        self.dev = torch.device(device)
        self.template = torch.get_rng_state()
        import numpy as np
        st = mt_state_from_torch(self.template)
        self.state = torch.from_numpy(st.astype(np.uint32).view(np.int32).copy()).to(self.dev)          # [625] u32 bits
        key = self.dev.index if self.dev.index is not None else torch.cuda.current_device()
        self.side = side_stream(self.dev, SIDE_REPLAY)      # one side stream per device for the life of the process
        self.side.wait_stream(torch.cuda.current_stream(self.dev))
        self.bufs = {}            # n -> [two device buffers]
        self.flip = 0
        self.ahead = None         # (n, tensor, state snapshot before it was drawn, event) of the block generated ahead of need
        self.drawn = 0

    def _generate(self, n, snapshot):
        """Enqueue the next n floats on the side stream -> (tensor, snapshot | None, event)."""
        pair = self.bufs.setdefault(n, [torch.empty(n, dtype=torch.float32, device=self.dev) for _ in range(2)])
        out = pair[self.flip]
        self.flip ^= 1
        with torch.cuda.stream(self.side):
            snap = self.state.clone() if snapshot else None
            _lib.call("svdd_mt19937_uniform_f32", self.state, out, n)       # (the current stream here is the side stream)
            ev = torch.cuda.Event()
            ev.record(self.side)
        return out, snap, ev

    def uniforms(self, n, prefetch=True):
        """The next n floats of the stream, usable on the CURRENT stream. prefetch: also start the n after them (a decode asks
        for the same n at every step); an unused prefetch is rolled back at close()."""
        cur = torch.cuda.current_stream(self.dev)
        if self.ahead is not None and self.ahead[0] == n:
            _, out, _, ev = self.ahead
            self.ahead = None
        else:
            self._rollback()
            self.side.wait_stream(cur)          # the buffer about to be overwritten may still be read by an earlier K1
            out, _, ev = self._generate(n, False)
        cur.wait_event(ev)
        self.drawn += n
        if prefetch:
            # the prefetch overwrites the OTHER buffer of the pair, last read by the K1 of the previous call: order after it
            self.side.wait_stream(cur)
            o2, snap, e2 = self._generate(n, True)
            self.ahead = (n, o2, snap, e2)
        return out

    def _rollback(self):
        if self.ahead is not None:
            _, _, snap, _ = self.ahead
            with torch.cuda.stream(self.side):
                self.state.copy_(snap)
            self.ahead = None

    def close(self):
        """Write the advanced state back into torch's global CPU generator (one small D2H copy + sync)."""
        self._rollback()
        self.side.synchronize()
        if self.drawn:
            import numpy as np
            st = self.state.cpu().numpy().view(np.uint32).astype(np.int64)
            torch.set_rng_state(mt_state_to_torch(st, self.template))
        torch.cuda.current_stream(self.dev).wait_stream(self.side)
