"""-m gpu: template-constrained design and re-mask refinement (ABI 16).

  kernel   svdd_refine_remask against the numpy restatement tests/refine_ref.py, bit for bit, in sentinel-guarded buffers
  engine   decoding from a given state (controlled_sample_from / decode_sample_from), renoise and refine on the reference's tiny
           nets, on the full-size L = 50 nets (hand-written kernels: the skipping loop with its logits cache) and at L = 200 (one
           sequence per tile: the shared tower and the carried stem)
  fixtures the reference's own q_xt + per-step updates driven from a start state (tests/golden/make_golden_refine.py), replayed
"""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

from tests.conftest import load_golden
from tests import e2e_parity
from tests import refine_ref as RR
from tests.kernel_harness import DEV, _Buf, _st

pytestmark = pytest.mark.gpu
MASK = 4


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


# ------------------------------------------------------------------------------------------------ the kernel ----
PAIRS = [(1.0, 1.0), (1.0, 0.5), (np.nan, 0.0), (2.0, np.nan), (-np.inf, -np.inf), (np.inf, 1e30), (0.5, np.inf), (-np.inf, -1.0),
         (1.0, -np.inf), (np.inf, np.inf), (-0.0, 0.0), (3.0, 2.9999998)]                 # ties, NaN, +-inf, a 1-ulp win


def _scores(B, shift, rng):
    sn, so = rng.standard_normal(B).astype(np.float32), rng.standard_normal(B).astype(np.float32)
    for b in range(min(B, len(PAIRS))):
        sn[b], so[b] = PAIRS[(b + shift) % len(PAIRS)]
    return sn, so


def _launch(x_new, mc, u=None, seed=0, row_offset=0, round=0, x_old=None, sn=None, so=None, frozen=None, alias=False,
            want_xt=True, want_keep=True, misalign=0, alias_score=False):
    """One svdd_refine_remask launch through the raw C entry, every output in a guarded sentinel buffer -> dict of numpy outputs
    (None where the buffer was not passed). alias: x_keep IS x_old. alias_score: score_keep IS score_old (what Diffusion.refine passes
    at every boundary). misalign: byte offset of the x_new / x_t rows' base."""
    from svdd_amd import _lib
    L_ = _lib.lib()
    B, L = x_new.shape
    hold = []

    def up(a, off=0):
        if a is None:
            return None
        t = torch.zeros(a.size * a.itemsize + 8, dtype=torch.uint8, device=DEV)
        t[off:off + a.size * a.itemsize] = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(DEV)
        hold.append(t)
        return t.data_ptr() + off

    judged = x_old is not None and sn is not None and so is not None
    keep = _Buf(B * L, torch.uint8) if (want_keep or judged) else None
    if alias:
        keep.body().copy_(torch.from_numpy(x_old.reshape(-1)).to(DEV))
    skeep = _Buf(B) if sn is not None else None
    if alias_score:
        skeep.body().copy_(torch.from_numpy(so).to(DEV))
    acc, nm = _Buf(B, torch.int32), _Buf(B, torch.int32) if want_xt else None
    xt = _Buf(B * L + 8, torch.uint8) if want_xt else None
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    rs = None
    if want_xt:
        if u is not None:
            rs = _lib.SvddRng(_lib.RNG_REPLAY, 0, up(np.asarray(u, np.float32)), 0, 0, 0, 0)
        else:
            rs = _lib.SvddRng(_lib.RNG_PHILOX, round, None, seed & 0xFFFFFFFFFFFFFFFF, row_offset, 0, 0)
    p = lambda b, off=0: None if b is None else b.ptr + off                                   # noqa: E731
    rc = L_.svdd_refine_remask(up(x_new, misalign), keep.ptr if alias else up(x_old), up(sn), skeep.ptr if alias_score else up(so),
                               up(frozen if want_xt else None),
                               float(mc), B, L, None if rs is None else ctypes.byref(rs), p(keep), p(skeep), p(acc),
                               p(xt, misalign), p(nm), err.data_ptr(), _st())
    _lib.check(rc, "svdd_refine_remask")
    torch.cuda.synchronize()
    out = dict(err=int(err[0]))
    for name, b, n in (("x_keep", keep, B * L), ("score_keep", skeep, B), ("accepted", acc, B), ("nmasked", nm, B)):
        if b is not None:
            b.assert_written(name)
            out[name] = b.cpu().numpy()
        else:
            out[name] = None
    if xt is not None:
        mask = torch.zeros(B * L + 8, dtype=torch.bool)
        mask[misalign:misalign + B * L] = True
        xt.assert_written_where("x_t", mask)
        out["x_t"] = xt.cpu().numpy()[misalign:misalign + B * L].reshape(B, L)
    else:
        out["x_t"] = None
    if out["x_keep"] is not None:
        out["x_keep"] = out["x_keep"].reshape(B, L)
    return out


def _same(got, ref, what):
    for k in ("x_keep", "x_t", "accepted", "nmasked"):
        if got[k] is not None:
            assert ref[k] is not None and np.array_equal(got[k], ref[k]), (what, k)
    if got["score_keep"] is not None:
        assert got["score_keep"].tobytes() == np.asarray(ref["score_keep"], np.float32).tobytes(), (what, "score_keep")
    assert got["err"] == ref["err"], (what, "err")


@pytest.mark.parametrize("mode", ["replay", "philox"])
@pytest.mark.parametrize("B", [1, 3, 257])
@pytest.mark.parametrize("L", [1, 3, 4, 5, 63, 64, 65, 200, 257])
def test_refine_remask_kernel_matches_the_restatement(L, B, mode):
    """Every shape (Philox block tails, unaligned rows, more rows than a workgroup's four waves) x frozen NULL / random / all ones
    x accept off / on (planted ties, NaN, +-inf) / on with x_keep aliasing x_old: tokens, scores, counts, bit for bit."""
    rng = np.random.default_rng(1000 * L + B)
    x_new = rng.integers(0, 5, (B, L)).astype(np.uint8)                       # MASK tokens in the input stay MASK
    x_old = rng.integers(0, 5, (B, L)).astype(np.uint8)
    seed, off, rnd = 0x9E3779B97F4A7C15 ^ (L * 7919 + B), 5 + B, (L + B) % 7
    mc = float(np.float32(0.2997))
    if mode == "replay":
        u = rng.random((B, L), dtype=np.float32)
        u[0, 0] = np.float32(mc)                                              # the compare is strict: u == move_chance does not mask
        if L > 1:
            u[0, 1] = np.nextafter(np.float32(mc), np.float32(0))
        kw = dict(u=u)
    else:
        u = RR.philox_uniforms(seed, off, B, L, rnd)
        kw = dict(seed=seed, row_offset=off, round=rnd)
    sn, so = _scores(B, L, rng)
    for fname, frozen in (("none", None), ("random", (rng.random((B, L)) < 0.4).astype(np.uint8) * 3), ("ones", np.ones((B, L), np.uint8))):
        _same(_launch(x_new, mc, frozen=frozen, **kw), RR.boundary(x_new, u, mc, frozen), ("off", fname))
        _same(_launch(x_new, mc, frozen=frozen, sn=sn, **kw), RR.boundary(x_new, u, mc, frozen, score_new=sn), ("off+score", fname))
        ref = RR.boundary(x_new, u, mc, frozen, x_old, sn, so)
        _same(_launch(x_new, mc, frozen=frozen, x_old=x_old, sn=sn, so=so, **kw), ref, ("on", fname))
        _same(_launch(x_new, mc, frozen=frozen, x_old=x_old, sn=sn, so=so, alias=True, **kw), ref, ("alias", fname))
        _same(_launch(x_new, mc, frozen=frozen, x_old=x_old, sn=sn, so=so, alias=True, alias_score=True, **kw), ref, ("alias both", fname))
    # accept alone (no x_t), and the re-mask alone (no x_keep)
    ref = RR.boundary(x_new, u, mc, None, x_old, sn, so)
    got = _launch(x_new, mc, x_old=x_old, sn=sn, so=so, want_xt=False)
    assert got["x_t"] is None and np.array_equal(got["x_keep"], ref["x_keep"]) and np.array_equal(got["accepted"], ref["accepted"])
    got = _launch(x_new, mc, want_keep=False, **kw)
    assert got["x_keep"] is None and np.array_equal(got["x_t"], RR.remask(x_new, u, mc)[0])
    for m in (0.0, 1.0):                                                      # nothing / every open position
        fz = (rng.random((B, L)) < 0.5).astype(np.uint8)
        _same(_launch(x_new, m, frozen=fz, **kw), RR.boundary(x_new, u, m, fz), ("mc", m))


@pytest.mark.parametrize("L", [64, 200])
def test_refine_remask_rows_at_an_odd_address_take_the_byte_path(L):
    """A multiple-of-4 length in buffers that are not 4-byte aligned: same results as the aligned launch."""
    rng = np.random.default_rng(L)
    B = 5
    x_new, x_old = rng.integers(0, 4, (B, L)).astype(np.uint8), rng.integers(0, 4, (B, L)).astype(np.uint8)
    sn, so = _scores(B, 1, rng)
    fz = (rng.random((B, L)) < 0.3).astype(np.uint8)
    for kw in (dict(u=rng.random((B, L), dtype=np.float32)), dict(seed=77, row_offset=2, round=3)):
        a = _launch(x_new, 0.45, frozen=fz, x_old=x_old, sn=sn, so=so, **kw)
        for mis in (1, 2, 3):
            b = _launch(x_new, 0.45, frozen=fz, x_old=x_old, sn=sn, so=so, misalign=mis, **kw)
            assert all(np.array_equal(a[k], b[k]) for k in ("x_keep", "x_t", "accepted", "nmasked"))


def test_refine_remask_philox_is_keyed_by_the_global_row_and_the_round():
    B, L, seed = 9, 203, 20240607
    rng = np.random.default_rng(3)
    x = rng.integers(0, 4, (B, L)).astype(np.uint8)
    whole = _launch(x, 0.5, seed=seed, row_offset=10, round=2)
    lo, hi = _launch(x[:3], 0.5, seed=seed, row_offset=10, round=2), _launch(x[3:], 0.5, seed=seed, row_offset=13, round=2)
    assert np.array_equal(whole["x_t"], np.concatenate([lo["x_t"], hi["x_t"]]))          # split at an odd row
    assert np.array_equal(whole["nmasked"], np.concatenate([lo["nmasked"], hi["nmasked"]]))
    other = _launch(x, 0.5, seed=seed, row_offset=10, round=3)
    assert (other["x_t"] != whole["x_t"]).mean() > 0.3                                   # rounds 2 and 3 draw different masks
    assert np.array_equal(whole["x_t"], RR.remask(x, RR.philox_uniforms(seed, 10, B, L, 2), 0.5)[0])
    # the stream is its own: the restatement's counters (word 3 = 1) reproduce the kernel, and none of them is a counter of
    # svdd_propose at the same seed / row / step; the mask is not what propose's first uniforms would give
    mine = set(zip(*[np.asarray(c).reshape(-1).tolist() for c in RR.philox_counters(10, B, L, 2)]))
    theirs = set(zip(*[np.asarray(c).reshape(-1).tolist() for c in RR.propose_counters(10, B, L, 2, 0)]))
    assert not mine & theirs
    for v in range(4):
        assert not np.array_equal(whole["x_t"], RR.remask(x, RR.propose_uniforms(seed, 10, B, L, 2, 0)[..., v], 0.5)[0])


def test_refine_remask_flags_a_token_above_mask_and_refuses_bad_arguments():
    from svdd_amd import _lib, ops
    x = np.zeros((3, 10), np.uint8)
    assert _launch(x, 0.5, seed=1)["err"] == 0
    x[2, 7] = 5
    got = _launch(x, 0.5, seed=1)
    assert got["err"] == 1 and got["x_keep"][2, 7] == 5
    xd = dev(x)
    with pytest.raises(ops.SvddError, match="token > 4"):
        ops.refine_remask(xd, 0.5, ops.Rng(seed=1))
    L_, one = _lib.lib(), dev(np.zeros(64, np.uint8))
    fbuf = dev(np.zeros(16, np.float32))
    p, q, f = one.data_ptr(), one.data_ptr() + 16, fbuf.data_ptr()
    ph = _lib.SvddRng(_lib.RNG_PHILOX, 0, None, 1, 0, 0, 0)
    call = lambda *a: L_.svdd_refine_remask(*a, _st())                                    # noqa: E731
    ok = (p, None, None, None, None, 0.5, 1, 4, ctypes.byref(ph), None, None, None, q, None, None)
    assert call(*ok) == _lib.OK
    bad = {"x_new null": (None,) + ok[1:], "no output": ok[:12] + (None,) + ok[13:], "mc > 1": ok[:5] + (1.5,) + ok[6:],
           "mc nan": ok[:5] + (float("nan"),) + ok[6:], "B = 0": ok[:6] + (0,) + ok[7:], "no rng": ok[:8] + (None,) + ok[9:],
           "x_t is x_new": ok[:12] + (p,) + ok[13:], "x_keep is x_new": ok[:9] + (p,) + ok[10:],
           "x_t is frozen": ok[:4] + (q,) + ok[5:], "frozen is x_new": ok[:4] + (p,) + ok[5:],
           "frozen is x_keep": ok[:4] + (q + 16,) + ok[5:9] + (q + 16,) + ok[10:],
           "judged without score_keep": (p, q, f, f) + ok[4:9] + (q + 16, None, None, None, None, None),
           "score_keep without score_new": ok[:10] + (f,) + ok[11:],
           "round > 65535": ok[:8] + (ctypes.byref(_lib.SvddRng(_lib.RNG_PHILOX, 65536, None, 1, 0, 0, 0)),) + ok[9:],
           "replay without uniforms": ok[:8] + (ctypes.byref(_lib.SvddRng(_lib.RNG_REPLAY, 0, None, 0, 0, 0, 0)),) + ok[9:],
           "uniforms_rows": ok[:8] + (ctypes.byref(_lib.SvddRng(_lib.RNG_REPLAY, 0, f, 0, 0, 0, 8)),) + ok[9:]}
    for what, a in bad.items():
        assert call(*a) == _lib.E_ARG, what
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the engine ----
@pytest.fixture(scope="module")
def nets():
    """name -> (model, embedding, head, B, S, M): the reference's tiny nets (PyTorch modules: the plain loop), the full-size nets at
    L = 50 (hand-written kernels: skipping loop, logits cache, one-row prior) and at L = 200 (shared tower, carried stem)."""
    from svdd_amd import synthetic
    out = {"tiny": e2e_parity.tiny_engine(load_golden("nets_tiny.npz"), 50, 8, DEV) + (8, 8, 4)}
    out["full50"] = synthetic.build("rna", DEV)[:3] + (8, 8, 4)
    out["full200"] = synthetic.build("dna", DEV)[:3] + (4, 6, 4)
    assert e2e_parity.uses_hand_written_kernels(*out["full50"][:3], 50) and e2e_parity.uses_hand_written_kernels(*out["full200"][:3], 200)
    return out


@contextlib.contextmanager
def knobs(model, **kw):
    keep = {k: getattr(model, k) for k in kw}
    for k, v in kw.items():
        setattr(model, k, v)
    try:
        yield model
    finally:
        for k, v in keep.items():
            setattr(model, k, v)


def _start_state(B, L, seed, p_mask=0.4):
    """Random tokens with 40 % MASK, rows all different (rows 0 and 1 in particular)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 4, (B, L), generator=g)
    x[torch.rand((B, L), generator=g) < p_mask] = MASK
    x[0, :4], x[1, :4] = torch.tensor([0, 1, MASK, 2]), torch.tensor([3, MASK, 1, 0])
    assert len({tuple(r.tolist()) for r in x}) == B
    return x.to(DEV)


@pytest.mark.parametrize("name", ["tiny", "full50"])
@pytest.mark.parametrize("mode", ["replay", "philox"])
def test_from_the_all_mask_state_at_t1_is_the_plain_decode(nets, name, mode):
    model, emb, head, B, S, M = nets[name]
    L = model.config.model.length
    prior = torch.full((B, L), MASK, dtype=torch.int64, device=DEV)
    with knobs(model, rng_mode=mode, philox_seed=5):
        runs = []
        for f in (lambda: model.controlled_sample(emb, head, num_steps=S, eval_sp_size=B, sample_M=M),
                  lambda: model.controlled_sample_from(prior, emb, head, t_start=1.0, num_steps=S, sample_M=M),
                  lambda: model.controlled_sample_from(prior.to(torch.uint8), emb, head, num_steps=S, sample_M=M),
                  lambda: model.decode_sample(num_steps=S, eval_sp_size=B),
                  lambda: model.decode_sample_from(prior, t_start=1.0, num_steps=S)):
            torch.manual_seed(123)
            x = f()
            runs.append((x, torch.rand(2)))
        for a, b in ((0, 1), (0, 2), (3, 4)):
            assert torch.equal(runs[a][0], runs[b][0]) and torch.equal(runs[a][1], runs[b][1])
        assert runs[1][0].dtype == torch.int64 and int(runs[1][0].max()) <= 3
    with knobs(model, rng_mode="philox", philox_seed=5):                      # num_steps None: ceil(t_start * config steps)
        model.config.sampling.steps, keep = 8, model.config.sampling.steps
        try:
            a = model.controlled_sample_from(prior, emb, head, t_start=1.0, sample_M=M)
            assert torch.equal(a, model.controlled_sample(emb, head, eval_sp_size=B, sample_M=M))
            model.skip_stats = {}
            model.controlled_sample_from(_start_state(B, L, 1), emb, head, t_start=0.3, sample_M=M)
            if name != "tiny":
                assert model.skip_stats["steps"] == 3                         # ceil(0.3 * 8)
        finally:
            model.config.sampling.steps, model.skip_stats = keep, None


@pytest.mark.parametrize("name", ["tiny", "full50", "full200"])
def test_from_a_state_whose_rows_differ_every_shortcut_setting_gives_the_same_tokens(nets, name):
    """skip_unchanged, logits_cache, incremental_backbone, dedup_prior each on and off from a start state with different rows: the
    same tokens (a surviving "row 0 stands for all rows" shortcut would make dedup_prior = True differ from False, and rows alike);
    every non-MASK token of x_init is in the result, in both samplers."""
    model, emb, head, B, S, M = nets[name]
    L = model.config.model.length
    x_init = _start_state(B, L, 7)
    base = dict(rng_mode="philox", philox_seed=31, skip_unchanged=True, logits_cache="auto", dedup_prior=True,
                incremental_backbone="on" if name == "full200" else "auto")
    outs = {}
    for label, kw in (("base", {}), ("skip off", dict(skip_unchanged=False)), ("cache on", dict(logits_cache="on")),
                      ("cache off", dict(logits_cache="off")), ("incr off", dict(incremental_backbone="off")),
                      ("incr on", dict(incremental_backbone="on")), ("dedup off", dict(dedup_prior=False)),
                      ("all off", dict(skip_unchanged=False, logits_cache="off", incremental_backbone="off", dedup_prior=False))):
        with knobs(model, **{**base, **kw}):
            model.skip_stats = {}
            outs[label] = model.controlled_sample_from(x_init, emb, head, t_start=0.6, num_steps=S, sample_M=M)
            stats, model.skip_stats = model.skip_stats, None
            if name == "full200" and label in ("base", "incr on"):
                assert stats.get("backbone_stem_tile_layers", 0) > 0          # the carried stem really ran from the non-prior start
    for label, x in outs.items():
        assert torch.equal(x, outs["base"]), label
    x = outs["base"]
    kept = x_init != MASK
    assert torch.equal(x[kept], x_init[kept]) and int(x.max()) <= 3
    assert not torch.equal(x[0], x[1])
    with knobs(model, **base):
        un = model.decode_sample_from(x_init, t_start=0.6, num_steps=S)
        with knobs(model, dedup_prior=False):
            assert torch.equal(un, model.decode_sample_from(x_init, t_start=0.6, num_steps=S))
        assert torch.equal(un[kept], x_init[kept]) and int(un.max()) <= 3 and not torch.equal(un[0], un[1])
        # the all-MASK shortcuts come back for the next decode from the prior
        a = model.controlled_sample(emb, head, num_steps=S, eval_sp_size=B, sample_M=M)
        assert model._from_state is False
        with knobs(model, dedup_prior=False):
            assert torch.equal(a, model.controlled_sample(emb, head, num_steps=S, eval_sp_size=B, sample_M=M))


@pytest.mark.parametrize("name", ["tiny", "full50"])
def test_renoise_is_q_xt_under_a_frozen_mask(nets, name):
    model, emb, head, B, S, M = nets[name]
    L = model.config.model.length
    x0 = _start_state(B, L, 11, p_mask=0.0)
    frozen = torch.rand((B, L), generator=torch.Generator().manual_seed(2)) < 0.3
    mc = model._move_chance(0.3)
    with knobs(model, rng_mode="replay"):
        torch.manual_seed(9)
        xt = model.renoise(x0, 0.3, frozen.to(DEV))
        after = torch.rand(2)
        torch.manual_seed(9)
        u = torch.rand(B, L)
        assert torch.equal(after, torch.rand(2))                              # the generator is where q_xt would leave it
        assert xt.dtype == x0.dtype and np.array_equal(xt.cpu().numpy(), RR.remask(x0.cpu().numpy(), u.numpy(), mc, frozen.numpy())[0])
        torch.manual_seed(9)
        plain = model.renoise(x0, 0.3)
        torch.manual_seed(9)
        assert torch.equal(plain, model.q_xt(x0, torch.full((B, 1), mc)))     # no frozen mask: the ELBO path's q_xt
    with knobs(model, rng_mode="philox", philox_seed=77, row_offset=3):
        xt = model.renoise(x0.to(torch.uint8), 0.3, frozen.to(DEV), round=2)
        ref = RR.remask(x0.cpu().numpy(), RR.philox_uniforms(77, 3, B, L, 2), mc, frozen.numpy())[0]
        assert xt.dtype == torch.uint8 and np.array_equal(xt.cpu().numpy(), ref)


@pytest.fixture(scope="module")
def refine_runs(nets):
    """Per net: the start designs and refine(...) at rounds 0..3 with one seed, computed once."""
    out = {}
    for name in ("tiny", "full50"):
        model, emb, head, B, S, M = nets[name]
        with knobs(model, rng_mode="philox", philox_seed=404):
            x0 = model.controlled_sample(emb, head, num_steps=S, eval_sp_size=B, sample_M=M)
            score0 = model._design_scorer(emb, head, None)(model._tokens_u8(x0))
            runs = {r: model.refine(x0, emb, head, r, 0.3, num_steps=4, sample_M=M) for r in (0, 1, 2, 3)}
        out[name] = (x0, score0, runs)
    return out


@pytest.mark.parametrize("name", ["tiny", "full50"])
def test_refine_improves_monotonically_and_counts_what_it_did(nets, refine_runs, name):
    model, emb, head, B, S, M = nets[name]
    L = model.config.model.length
    x0, score0, runs = refine_runs[name]
    x, sc, stats = runs[0]
    assert torch.equal(x, x0) and torch.equal(sc, score0) and stats["accepted"] == [] and stats["masked"] == []      # rounds = 0
    prev = score0
    for r in (1, 2, 3):
        x, sc, stats = runs[r]
        print(f"refine {name} rounds {r}: accepted {stats['accepted']} masked {stats['masked']} mean score {float(sc.mean()):.6f}")
        assert x.dtype == torch.int64 and int(x.max()) <= 3 and sc.shape == (B,) and sc.dtype == torch.float32
        assert bool((sc >= prev).all()), (r, sc, prev)                        # exact: one kernel path gives every score
        assert torch.equal(sc, model._design_scorer(emb, head, None)(model._tokens_u8(x)))       # the score IS the returned row's
        assert len(stats["accepted"]) == len(stats["masked"]) == r and stats["accepted"][:r - 1] == runs[r - 1][2]["accepted"]
        prev = sc
    # a recount from the returned states: an accepted row scores strictly higher, so its tokens changed; round 0's mask is renoise's
    x1, sc1, st1 = runs[1]
    assert st1["accepted"][0] == int((x1 != x0).any(1).sum()) == int((sc1 > score0).sum())
    with knobs(model, rng_mode="philox", philox_seed=404):
        assert st1["masked"][0] == int((model.renoise(x0, 0.3, round=0) == MASK).sum())
        # accept = "always": every row takes its new version each round
        xa, sa, sta = model.refine(x0, emb, head, 2, 0.3, num_steps=4, sample_M=M, accept="always")
        assert sta["accepted"] == [B, B] and torch.equal(sa, model._design_scorer(emb, head, None)(model._tokens_u8(xa)))
        # frozen all ones: nothing is re-masked, whatever the number of rounds
        xf, sf, stf = model.refine(x0, emb, head, 3, 0.3, num_steps=4, sample_M=M, frozen=torch.ones((B, L), dtype=torch.bool, device=DEV))
        assert torch.equal(xf, x0) and torch.equal(sf, score0) and stf["masked"] == [0, 0, 0] and stf["accepted"] == [0, 0, 0]
        # a frozen flank survives every round, accepted or not
        fz = torch.zeros((B, L), dtype=torch.uint8, device=DEV)
        fz[:, :L // 2] = 1
        xh, _, _ = model.refine(x0, emb, head, 2, 0.9, num_steps=4, sample_M=M, frozen=fz, accept="always")
        assert torch.equal(xh[:, :L // 2], x0[:, :L // 2]) and not torch.equal(xh, x0)
        # the reward model as the judge
        if name == "full50":
            from svdd_amd.value_nets import RewardModel
            xr, sr, _ = model.refine(x0, emb, head, 1, 0.3, num_steps=4, sample_M=M, reward_model=RewardModel(emb, head))
            assert torch.equal(xr, x1) and torch.equal(sr, sc1)


@pytest.mark.parametrize("name", ["tiny", "full50"])
def test_refine_rows_do_not_depend_on_how_the_batch_is_split(nets, refine_runs, name):
    """Through distributed.sharded_sample, the way DESIGN 4g documents it: the from-state methods take the rank's rows of the start
    state (model.row_offset is the rank's first global row while the sampler runs), not an eval_sp_size."""
    from svdd_amd import distributed
    model, emb, head, B, S, M = nets[name]
    x0, _, runs = refine_runs[name]
    x, sc, _ = runs[2]
    x_init = _start_state(B, model.config.model.length, 21)
    with knobs(model, rng_mode="philox", philox_seed=404):
        whole = model.controlled_sample_from(x_init, emb, head, t_start=0.6, num_steps=S, sample_M=M)
        for rank in (0, 1):
            lo = 4 * rank
            rows = lambda t, n: t[model.row_offset:model.row_offset + n]                                   # noqa: E731
            out = {}
            xs = distributed.sharded_sample(
                model, B, lambda eval_sp_size: out.setdefault("r", model.refine(rows(x0, eval_sp_size), emb, head, 2, 0.3, num_steps=4,
                                                                                sample_M=M))[0], rank=rank, world=2)
            ss = out["r"][1]
            assert model.row_offset == 0 and model._shard is None
            assert torch.equal(xs, x[lo:lo + 4]), lo
            # (the tiny nets run as PyTorch modules, whose vendor kernels are chosen per batch size: their scores agree to round-off;
            #  the hand-written kernels give a row the same bits in any batch)
            assert torch.equal(ss, sc[lo:lo + 4]) if name == "full50" else torch.allclose(ss, sc[lo:lo + 4], rtol=1e-5, atol=1e-6), lo
            part = distributed.sharded_sample(model, B, lambda eval_sp_size: model.controlled_sample_from(
                rows(x_init, eval_sp_size), emb, head, t_start=0.6, num_steps=S, sample_M=M), rank=rank, world=2)
            assert torch.equal(part, whole[lo:lo + 4]), lo


def test_refusals(nets):
    from svdd_amd import ops
    model, emb, head, B, S, M = nets["tiny"]
    L = model.config.model.length
    x = _start_state(B, L, 3)
    clean = torch.zeros((B, L), dtype=torch.int64, device=DEV)
    cs = lambda xi=x, **kw: model.controlled_sample_from(xi, emb, head, num_steps=2, sample_M=2, **kw)     # noqa: E731
    rf = lambda xi=clean, rounds=1, t=0.3, **kw: model.refine(xi, emb, head, rounds, t, num_steps=2, sample_M=2, **kw)   # noqa: E731
    with knobs(model, rng_mode="philox"):
        with knobs(model, time_conditioning=True):
            for f in (cs, rf, lambda: model.decode_sample_from(x), lambda: model.renoise(clean, 0.3)):
                with pytest.raises(NotImplementedError):
                    f()
        for f in (lambda: cs(x.cpu()), lambda: rf(clean.cpu()), lambda: model.renoise(clean.cpu(), 0.3),
                  lambda: model.decode_sample_from(x.cpu()), lambda: rf(frozen=torch.ones(B, L)),
                  lambda: cs(torch.full_like(x, 5)), lambda: rf(torch.full_like(x, 5)), lambda: rf(rounds=70000),
                  lambda: rf(torch.full_like(x, 5).to(torch.uint8)), lambda: cs(torch.full_like(x, 5).to(torch.uint8)),
                  lambda: model.renoise(torch.full_like(x, 5).to(torch.uint8), 0.3)):
            with pytest.raises(ops.SvddError):
                f()
        for f in (lambda: cs(t_start=1e-5), lambda: cs(t_start=0.0), lambda: cs(t_start=1.5), lambda: rf(t=1e-5), lambda: rf(t=1.0001),
                  lambda: model.renoise(clean, 0.0), lambda: model.renoise(clean, 1.5), lambda: cs(x[:, :L - 1]), lambda: cs(x.float()),
                  lambda: rf(accept="maybe"), lambda: rf(rounds=-1), lambda: rf(frozen=torch.ones((B, L - 1), device=DEV)),
                  lambda: cs(x[:0])):
            with pytest.raises(ValueError):
                f()
    with knobs(model, rng_mode="replay", _shard=(0, 4, 8, 2)):
        for f in (cs, rf, lambda: model.renoise(clean, 0.3), lambda: model.decode_sample_from(x)):
            with pytest.raises(ops.SvddError, match="replay"):
                f()
    assert model._step_base == 0 and model._shard is None


def test_harness_controlled_decode_refine(nets):
    from svdd_amd.harness import BaseModel, batch_seed
    from svdd_amd.value_nets import RewardModel
    model, emb, head, B, S, M = nets["tiny"]
    h = BaseModel(emb, head, model, RewardModel(emb, head), 4, task="rna")
    with knobs(model, rng_mode="philox", philox_seed=8):
        model.config.sampling.steps, keep = 4, model.config.sampling.steps
        try:
            samples, value_preds, reward_preds, top_k, baseline = h.controlled_decode_refine(1, 2, rounds=2, t_renoise=0.5)
            assert model.philox_seed == 8
            with knobs(model, philox_seed=batch_seed(8, 0)):                  # the key the harness gives its first guided batch
                plain = model.controlled_sample(emb, head, eval_sp_size=4, sample_M=2)
                want, score, stats = model.refine(plain, emb, head, 2, 0.5, sample_M=2)
        finally:
            model.config.sampling.steps = keep
    assert len(samples) == 1 and torch.equal(samples[0], want) and h.refine_stats == [stats] and stats["steps_per_round"] == 2
    assert value_preds.shape == (4,) and baseline.shape == (4,) and torch.allclose(value_preds.reshape(-1), score, rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------------------------- the reference's recorded runs ----
def _replay_case(g, case, model, emb, head):
    """The engine in replay mode over a recorded two-round run: every re-masked state, every per-step state, both x_0 and the
    generator's end state -> (rows whose trajectory differs anywhere, the case's row count). Round 0's re-masked state involves no
    net and is asserted outright."""
    from svdd_amd import ops
    c = {k[len(case) + 1:]: v for k, v in g.items() if k.startswith(case + "_")}
    B, L = c["x0"].shape
    S, M, t0 = int(c["S"]), int(c["M"]), float(c["t_start"])
    x0, frozen = dev(c["x0"]).long(), dev(c["frozen"])
    finals, xts, stepped = [], [], []
    orig, orig_propose = model._noise_removal, ops.propose
    model._noise_removal = lambda *a, **k: finals.append(orig(*a, **k)) or finals[-1]

    def propose(logits, x, *a, **k):                       # the un-guided loop keeps no state trace: x of every step's draw
        stepped.append(x.detach().clone())
        return orig_propose(logits, x, *a, **k)
    try:
        with knobs(model, rng_mode="replay", state_trace=[]):
            torch.manual_seed(int(c["seed"]))
            if int(c["guided"]):
                x, _, stats = model.refine(x0, emb, head, 2, t0, num_steps=S, eps=float(c["eps"]), sample_M=M, frozen=frozen,
                                           accept="always")
                assert stats["accepted"] == [B, B]
                states = torch.stack(model.state_trace).cpu().numpy()
            else:
                ops.propose = propose
                x = x0
                for r in range(2):
                    xts.append(model.renoise(x, t0, frozen))
                    x = model.decode_sample_from(xts[-1], t_start=t0, num_steps=S, eps=float(c["eps"]))
                # per round: x before each of the S steps (propose's input), then x before the noise removal (state_trace)
                assert len(stepped) == 2 * S and len(model.state_trace) == 2
                states = torch.stack([t for r in range(2) for t in stepped[r * S:(r + 1) * S] + [model.state_trace[r]]]).cpu().numpy()
            nxt = torch.rand(2)
    finally:
        del model._noise_removal
        ops.propose = orig_propose
    assert np.array_equal(nxt.numpy(), c["next"]), "the generator's end state"
    fin = torch.stack(finals).cpu().numpy()
    assert fin.shape == (2, B, L) and np.array_equal(fin[1], x.cpu().numpy())
    assert states.shape == (2 * (S + 1), B, L)
    states = states.reshape(2, S + 1, B, L)
    if xts:                                                # renoise's own output is what each un-guided round started from
        assert np.array_equal(torch.stack(xts).cpu().numpy(), states[:, 0])
    # round 0's re-masked state: the mask rule on THIS host's move_chance, bit for bit, from the replayed torch.rand(B, L). The
    # scalar goes through torch's CPU exp / log1p, whose vectorised code may differ between CPU generations by an ulp (as for g30 /
    # g31, tests/elbo_ref.py): it is held to one ulp of exp of the recorded one, and a position of x_t may differ from the recorded
    # state only where its uniform lies between the two scalars - with equal scalars (the usual case) that is equality everywhere.
    mc_host, mc_rec = np.float32(model._move_chance(t0)), np.float32(c["move_chance"])
    assert abs(float(mc_host) - float(mc_rec)) <= 2.0 ** -24, (mc_host, mc_rec)
    torch.manual_seed(int(c["seed"]))
    u = torch.rand(B, L).numpy()
    assert np.array_equal(states[0, 0], RR.remask(c["x0"], u, mc_host, c["frozen"])[0]), "round 0's re-masked state (mask rule)"
    differs = states[0, 0] != c["xt"][0]
    assert np.all((u[differs] >= min(mc_host, mc_rec)) & (u[differs] < max(mc_host, mc_rec))), "round 0's re-masked state (recorded)"
    assert mc_host != mc_rec or not differs.any()
    bad = (fin != c["final"]).any(axis=(0, 2)) | (states != c["states"]).any(axis=(0, 1, 3)) | (states[:, 0] != c["xt"]).any(axis=(0, 2))
    return int(bad.sum()), B


@pytest.mark.parametrize("case", ["mc_t03", "mc_t10", "un_t03"])
def test_recorded_reference_run_tiny_nets(nets, case):
    """g32: every recorded state, both rounds' x_0 and the generator's end state. Cap on rows that leave the recorded trajectory at a
    near-tie of argmax (the nets run on other convolution code than the recording's): what the recorded run shows + 1: the CPU oracle
    port (oracle/svdd_oracle.py around the same nets) follows each recorded case with 0 rows off."""
    model, emb, head, *_ = nets["tiny"]
    bad, B = _replay_case(load_golden("g32_refine_tiny.npz"), case, model, emb, head)
    print(f"g32 {case}: rows off the recorded trajectory {bad} of {B}")
    assert bad <= 1


def test_recorded_reference_run_full_size_nets(nets):
    """g33: seed-44 full-size nets, L = 200, B = 3, t_start 0.3, 39 steps, M = 10, through the hand-written kernels; same cap."""
    model, emb, head, *_ = nets["full200"]
    g = load_golden("g33_refine_full.npz")
    for nm, mod in (("backbone", model.backbone), ("embedding", emb), ("head", head)):
        sums = np.array([float(p.double().sum()) for p in mod.state_dict().values()])
        assert np.allclose(sums, g["mc_t03_" + nm + "_param_sums"], rtol=0, atol=1e-6), nm
    bad, B = _replay_case(g, "mc_t03", model, emb, head)
    print(f"g33 mc_t03: rows off the recorded trajectory {bad} of {B}")
    assert bad <= 1
