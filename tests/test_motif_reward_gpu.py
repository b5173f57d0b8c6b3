"""-m gpu: the motif reward of SVDD-PM decoding. svdd_motif_reward is integer arithmetic up to its last two fp32
operations, so every output must EQUAL tests/motif_reward_ref.py's restatement, score bits and term.

  entry    svdd_motif_reward through the raw C entry in sentinel-guarded buffers (tests/kernel_harness.py): the lengths, widths, motif
           and row counts at which the kernel takes another path (one word and 64, L below some widths, one table stage and three,
           one row, one below / at / one above a row tile of 8, 32 and 64), the device-side count at 0, 1, n - 1 and n with the rows
           beyond it untouched, both strands and forward only, negative coefficients, caps and floors of 0, a term beyond 32 bits,
           base NULL / given / aliased with score, term only and score only, a token 4, two launches
  public   MotifReward.term for every chunking; GuidedReward's two doors
  decodes  SVDD-PM under a GuidedReward through the skipping loop against skip_unchanged off and against a host restatement of the
           loop, without and with a fused reward net as base; guidance raises the motif term; BaseModel.controlled_decode_motif; the
           --guide_* flags of the tweedie decode script
"""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from svdd_amd import _lib, motifs, ops
from tests import motif_reward_ref as RR
from tests.kernel_harness import DEV, _Buf, _st

pytestmark = pytest.mark.gpu
ROW_TILES = (8, 32, 64)                       # the tile sizes the kernel was measured at (it is built with one of them)
UNIT = 2.0 ** -10


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _reward(x, ms, c, both=True, count=None, base="null", outputs=("score", "term"), unit=UNIT, want_err=False):
    """One launch into guarded buffers -> (score f32 [n] | None, term i64 [n] | None, err). count: None (NULL) or an int on the
    device. base: "null", "given" (a separate buffer) or "alias" (the score buffer itself holds it). Exactly the rows below count are
    written; with "alias" the others keep their base."""
    n, L = x.shape
    M = len(ms.width)
    live = n if count is None else count
    tok = _dev(x.astype(np.uint8))
    score = _Buf(n) if "score" in outputs else None
    term = _Buf(2 * n, torch.int64) if "term" in outputs else None
    base_np = np.random.default_rng(n * 131 + L).standard_normal(n).astype(np.float32) * 3
    base_t = None
    if base == "given":
        base_t = _dev(base_np)
    elif base == "alias":
        score.body().copy_(_dev(base_np))
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    cnt = None if count is None else torch.tensor([count], dtype=torch.int32, device=DEV)
    args = [_dev(a) for a in (ms.pwm, ms.width, ms.threshold, c.hit_coef, c.hit_cap, c.margin_coef, c.margin_floor)]
    rc = _lib.lib().svdd_motif_reward(tok.data_ptr(), n, L, None if cnt is None else cnt.data_ptr(), args[0].data_ptr(),
                                      args[1].data_ptr(), args[2].data_ptr(), M, int(both), *[a.data_ptr() for a in args[3:]],
                                      score.ptr if base == "alias" else None if base_t is None else base_t.data_ptr(), unit,
                                      None if score is None else score.ptr, None if term is None else term.ptr, err.data_ptr(), _st())
    _lib.check(rc, "svdd_motif_reward")
    torch.cuda.synchronize()
    rows = torch.arange(n) < live
    out_s = out_t = None
    if score is not None:
        if base == "alias":
            score.untouched()                                              # the guards
            assert np.array_equal(score.cpu().numpy()[live:], base_np[live:]), "a row beyond count lost its base"
        else:
            score.assert_written_where("svdd_motif_reward score", rows)
        out_s = score.cpu().numpy().copy()[:live]
    if term is not None:
        term.assert_written_where("svdd_motif_reward term", rows.repeat_interleave(2))
        out_t = term.cpu().numpy().copy()[:live]
    return out_s, out_t, (int(err[0]) if want_err else None), (base_np if base != "null" else None)


def _check(x, ms, c, both=True, count=None, base="null", outputs=("score", "term"), unit=UNIT):
    got_s, got_t, _, base_np = _reward(x, ms, c, both, count, base, outputs, unit)
    live = x.shape[0] if count is None else count
    T = RR.term_ref(x[:live], ms, c.hit_coef, c.hit_cap, c.margin_coef, c.margin_floor, both)
    if got_t is not None:
        assert np.array_equal(got_t, T), ("term", x.shape, both, count)
    if got_s is not None:
        want = RR.score_ref(T, unit, None if base_np is None else base_np[:live])
        assert np.array_equal(got_s.view(np.int32), want.view(np.int32)), ("score bits", x.shape, both, count, base)
    return T


# ------------------------------------------------------------------------------------------------------ the entry ----
@pytest.mark.parametrize("L", [1, 10, 15, 16, 17, 33, 200, 1024])
def test_entry_equals_the_restatement_over_lengths(L):
    """Widths 1, 16, 17, 32 and five between, M = 9 (two table stages), 13 rows (a full group of 8 and a partial one); L = 1 and
    L = 10 lie below some widths (no window: the margin is -margin_floor)."""
    rng = np.random.default_rng(L)
    ms, c = RR.random_case(rng, (1, 16, 17, 32, 5, 8, 12, 20, 31))
    x = rng.integers(0, 4, (13, L))
    seen = set()
    for both, base in ((True, "null"), (False, "given")):
        T = _check(x, ms, c, both, base=base)
        seen.update(T.tolist())
    assert len(seen) > 1 or L == 1


@pytest.mark.parametrize("M", [1, 8, 9, 17])
def test_entry_equals_the_restatement_over_motif_counts(M):
    rng = np.random.default_rng(100 + M)
    ms, c = RR.random_case(rng, rng.integers(1, 33, M))
    x = rng.integers(0, 4, (9, 33))
    _check(x, ms, c, True)
    _check(x, ms, c, False, base="alias")


@pytest.mark.parametrize("tile", ROW_TILES)
def test_entry_over_row_counts_and_device_counts(tile):
    """n = 1, tile - 1, tile, tile + 1; at n = tile + 1 and 2 tile + 3 the device count at 0, 1, n - 1 and n: rows beyond it keep
    the sentinel (or, aliased, their base) and whole workgroups exit."""
    rng = np.random.default_rng(tile)
    ms, c = RR.random_case(rng, (6, 11, 19))
    for n in sorted({1, tile - 1, tile, tile + 1}):
        _check(rng.integers(0, 4, (n, 40)), ms, c)
    for n in (tile + 1, 2 * tile + 3):
        x = rng.integers(0, 4, (n, 40))
        for count in (0, 1, n - 1, n):
            _check(x, ms, c, count=count, base="given")
            _check(x, ms, c, both=False, count=count, base="alias", outputs=("score",))


def test_entry_coefficient_edges():
    """Hand-set coefficients: a penalty, a cap of 0 (the hits do not count), a cap that binds, a floor of 0 (no margin), a floor that
    binds, a negative margin coefficient; and a row that holds the consensus, whose margin saturates at 0."""
    rng = np.random.default_rng(7)
    ms, _ = RR.random_case(rng, (4, 4, 4, 9, 9, 9), frac=0.2)
    ms.threshold[3:] *= 3                                                  # the wide motifs: thresholds few windows reach
    x = rng.integers(0, 4, (12, 60))
    x[0, 10:19] = ms.pwm[3, :9].argmax(1)
    i32 = lambda *v: np.array(v, np.int32)                                 # noqa: E731
    c = SimpleNamespace(hit_coef=i32(-700, 900, 50, 0, 0, 3), hit_cap=i32(2, 0, 1, 5, 5, 1 << 20),
                        margin_coef=i32(0, 0, 0, 11, -13, 2), margin_floor=i32(0, 0, 0, 0, 150, (1 << 31) - 1))
    T = _check(x, ms, c)
    hits = np.stack([RR.term_ref(x, ms, i32(*(int(j == m) for j in range(6))), i32(*[1 << 20] * 6), i32(*[0] * 6), i32(*[0] * 6))
                     for m in range(6)], 1)                                # [n, M] plain hit counts from the restatement
    assert (hits[:, 0] > 2).any() and (hits[:, 1] > 0).any() and (hits[:, 2] > 1).any()      # the caps bind somewhere
    assert hits[0, 3] >= 1                                                 # the planted site: motif 3's margin is 0 in row 0
    assert len(set(T.tolist())) > 6
    _check(x, ms, c, both=False)


def test_entry_term_beyond_32_bits():
    """+-32767 in every entry of two width-32 motifs and margin_coef = 2^31 - 1: |T| reaches 2^31 x 2^21; the fp32 score is the
    rounded int64, times the unit."""
    rng = np.random.default_rng(8)
    pwm = np.where(rng.random((2, 32, 4)) < 0.5, 32767, -32767).astype(np.int16)
    pwm[:, np.arange(32), rng.integers(0, 4, 32)] = 32767                   # every column can score +32767
    ms =SimpleNamespace(width=np.array([32, 32], np.int32), pwm=pwm, threshold=np.array([32 * 32767, 1000], np.int32))
    big = (1 << 31) - 1
    c = SimpleNamespace(hit_coef=np.array([big, -big], np.int32), hit_cap=np.array([3, 3], np.int32),
                        margin_coef=np.array([big, -big], np.int32), margin_floor=np.array([1 << 22, 1 << 21], np.int32))
    x = rng.integers(0, 4, (10, 70))
    x[1, 5:37] = pwm[0].argmax(1)                                           # the all-maximum window: a hit at the threshold itself
    for unit in (UNIT, 1.0, 2.0 ** -40):
        T = _check(x, ms, c, unit=unit, base="given")
    assert np.abs(T).max() > 1 << 45 and len(set(T.tolist())) > 3
    assert T[1] != T[0]


@pytest.mark.parametrize("base", ["null", "given", "alias"])
def test_entry_optional_outputs_and_two_launches(base):
    rng = np.random.default_rng(9)
    ms, c = RR.random_case(rng, (3, 10, 18, 32, 7, 7, 7, 7, 25))
    x = rng.integers(0, 4, (41, 77))
    outs = [("score", "term"), ("score",)] + ([("term",)] if base != "alias" else [])
    for outputs in outs:
        _check(x, ms, c, base=base, outputs=outputs, count=37)
    a = _reward(x, ms, c, base=base)
    b = _reward(x, ms, c, base=base)
    assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32)) and np.array_equal(a[1], b[1])


def test_entry_flags_a_bad_token_and_reads_it_as_0():
    rng = np.random.default_rng(10)
    ms, c = RR.random_case(rng, (5, 16, 21))
    x = rng.integers(0, 4, (20, 50))
    assert _reward(x, ms, c, want_err=True)[2] == 0
    x[17, 49] = 4
    x[3, 0] = 255
    s, t, err, _ = _reward(x, ms, c, want_err=True)
    assert err == 1
    T = RR.term_ref(np.where(x > 3, 0, x), ms, c.hit_coef, c.hit_cap, c.margin_coef, c.margin_floor)
    assert np.array_equal(t, T) and np.array_equal(s.view(np.int32), RR.score_ref(T, UNIT).view(np.int32))
    assert _reward(x, ms, c, count=3, want_err=True)[2] == 0               # rows beyond the count are not read


# ----------------------------------------------------------------------------------------------------- the public ----
@pytest.fixture(scope="module")
def site():
    """One motif of width 10 with a clear consensus, p = 1e-4 threshold."""
    consensus = [0, 2, 3, 3, 1, 0, 0, 2, 1, 3]
    pfm = np.full((10, 4), 0.05)
    pfm[np.arange(10), consensus] = 0.85
    return motifs.MotifSet.from_pfms([pfm], names=["SITE"])


def test_term_is_independent_of_the_chunking():
    rng = np.random.default_rng(11)
    ms = motifs.MotifSet.from_pfms([rng.dirichlet([0.5] * 4, int(w)) for w in (6, 9, 14, 20, 32)], pvalue=1e-3)
    mr = motifs.MotifReward(ms, hit_weight=[1.0, -2.0, 0.5, 3.0, 1.0], margin_weight=[0.01, 0.0, 0.02, -0.005, 0.001], hit_cap=2)
    x = rng.integers(0, 4, (150, 64))
    T = RR.term_ref(x, ms, mr.hit_coef, mr.hit_cap, mr.margin_coef, mr.margin_floor)
    want = RR.score_ref(T, mr.unit)
    assert len(set(T.tolist())) > 20
    for rows in (None, 1, 7, 64, 149, 150, 1000):
        got, gi = mr.term(x if rows != 7 else torch.from_numpy(x).to(DEV), chunk_rows=rows, return_int=True)
        assert got.dtype == torch.float32 and got.device.type == "cuda"
        assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32)) and np.array_equal(gi.cpu().numpy(), T)
    bad = torch.from_numpy(x).to(DEV)
    bad[5, 5] = 4
    with pytest.raises(ops.SvddError, match="token > 3"):
        mr.term(bad)
    # GuidedReward without a net: both doors give the term on task 0
    gr = motifs.GuidedReward(None, mr)
    tok = torch.from_numpy(x.astype(np.uint8)).to(DEV)
    for out in (gr.forward_tokens(tok), gr(ops.transform_samples(tok)), gr(ops.transform_samples(tok, transposed=True))):
        assert out.shape == (150, 1, 1) and np.array_equal(out.reshape(-1).cpu().numpy().view(np.int32), want.view(np.int32))
    masked = tok.clone()
    masked[3, 7] = 4
    with pytest.raises(ValueError, match="MASK"):
        gr(ops.transform_samples(masked))


# ---------------------------------------------------------------------------------------------------- the decodes ----
B, M, S, SEED = 8, 4, 12, 5


@pytest.fixture(scope="module")
def nets():
    from svdd_amd import synthetic
    # L = 50, one stack of layers at hidden 128: the smallest backbone the one-launch kernel (which the skipping loop needs) takes
    model, emb, head, reward = synthetic.build("rna", DEV, hidden_dim=128, num_cnn_stacks=1)
    model.rng_mode, model.philox_seed = "philox", SEED
    return model, emb, head, reward


def _np_term(mr, tok):
    x = tok.cpu().numpy()
    return RR.score_ref(RR.term_ref(x, mr.mset, mr.hit_coef, mr.hit_cap, mr.margin_coef, mr.margin_floor, mr.both), mr.unit)


def _host_decode(model, base, mr):
    """The SVDD-PM loop restated on the host from ops.propose, ops.x0hat, the numpy term and ops.select: every candidate's x0-hat is
    scored, nothing is skipped -> (x0 int64 [B, L], the per-step scores fp32 [S, B, M])."""
    _, L, _, sched, x = model._decode_start(S, 1e-5, B)
    scores = []
    for i in range(S):
        logits = model._backbone_logits(x)
        cand, _, _ = ops.propose(logits, x, sched[i, 2], sched[i, 1], M, model._rng(i, M, B, L, logits))
        flat = cand.reshape(B * M, L)
        _, xh = ops.x0hat(model._backbone_logits(flat), flat, want_tokens=True, want_onehot=False)
        sc = _np_term(mr, xh)
        if base is not None:
            sc = (base.forward_tokens(xh).reshape(-1).float().cpu().numpy() + sc).astype(np.float32)     # one fp32 addition
        sc = torch.from_numpy(sc).to(DEV).view(B, M)
        scores.append(sc)
        mode, rng = model._select_args(i)
        x, _, _ = ops.select(sc, cand, mode=mode, rng=rng, want_soft=False)
    return model._noise_removal(x), torch.stack(scores)


def _decode(model, reward, skip):
    model.skip_unchanged, model.trace, model.skip_stats = skip, [], {}
    try:
        x0 = model.controlled_sample_tweedie(reward, num_steps=S, eval_sp_size=B, sample_M=M, options="True", task="rna")
        torch.cuda.synchronize()
        return x0, torch.stack([s for _, s in model.trace if s is not None]), dict(model.skip_stats)
    finally:
        model.skip_unchanged, model.trace, model.skip_stats = True, None, None


@pytest.mark.parametrize("with_net", [False, True])
def test_guided_decode_skipping_equals_plain_and_host(nets, site, with_net):
    """GuidedReward(None | the fused ConvGRU reward net, mr) through _tweedie_sample_skipping: the same tokens as with
    skip_unchanged off (the generic loop, through __call__) and as the host restatement, and the same per-step scores as the
    restatement's (base.forward_tokens plus the numpy term, added in fp32), bit for bit."""
    model, _, _, reward = nets
    mr = motifs.MotifReward(site, hit_weight=1.5, margin_weight=0.004)
    gr = motifs.GuidedReward(reward if with_net else None, mr)
    x_skip, sc_skip, stats = _decode(model, gr, True)
    assert stats.get("kind") == "pm" and 0 < stats["live_candidates"] <= stats["candidates"] == B * M * S     # the skipping loop ran
    x_plain, sc_plain, stats_plain = _decode(model, gr, False)
    assert "kind" not in stats_plain
    base = model.reward_callable(reward) if with_net else None
    assert base is None or hasattr(base, "forward_tokens")
    x_host, sc_host = _host_decode(model, base, mr)
    assert x_skip.dtype == torch.int64 and x_skip.shape == (B, 50) and int(x_skip.max()) <= 3
    assert torch.equal(x_skip, x_plain) and torch.equal(x_skip, x_host)
    assert torch.equal(sc_skip, sc_host)
    if not with_net:                                      # (with a net the generic loop goes through the net's one-hot door: its tokens are compared)
        assert torch.equal(sc_plain, sc_host)
    assert bool((sc_host.max(2).values != sc_host.min(2).values).any())     # the choice among a row's candidates mattered somewhere


def test_guidance_raises_the_motif_term(nets, site):
    """A positive margin weight on SITE (width 10): the mean term of the guided batch is strictly greater than that of the un-guided
    decode of the same seed (no tolerance). Measured on MI355X: guided -6.92138671875, un-guided -10.87646484375."""
    model, _, _, _ = nets
    mr = motifs.MotifReward(site, margin_weight=0.01)
    x_g, _, stats = _decode(model, motifs.GuidedReward(None, mr), True)
    assert stats.get("kind") == "pm"
    x_u = model.decode_sample(num_steps=S, eval_sp_size=B)
    guided, unguided = float(mr.term(x_g).double().mean()), float(mr.term(x_u).double().mean())
    print(f"MOTIF_TERM guided {guided!r} unguided {unguided!r}")
    assert unguided < 0.0                                                  # not saturated: no un-guided row holds the site
    assert guided > unguided


def test_controlled_decode_motif_fills_motif_terms(nets, site):
    from svdd_amd.harness import BaseModel
    model, emb, head, reward = nets
    steps = model.config.sampling.steps
    model.config.sampling.steps = S
    try:
        bm = BaseModel(emb, head, model, reward, B, task="rna", val_batch_num=0).to(DEV).eval()
        mr = motifs.MotifReward(site, hit_weight=2.0, margin_weight=0.01)
        samples, value_preds, reward_preds, selected, baseline = bm.controlled_decode_motif(2, 2, mr)
    finally:
        model.config.sampling.steps = steps
    assert len(samples) == 2 * B and reward_preds.shape[0] == 2 * B and baseline.shape[0] == 2 * B
    assert len(bm.motif_terms) == 2 and all(t.shape == (B,) and t.dtype == torch.float32 for t in bm.motif_terms)
    x = torch.stack(list(samples))
    assert np.array_equal(torch.cat(bm.motif_terms).cpu().numpy().view(np.int32), _np_term(mr, x).view(np.int32))
    plain = torch.cat([bm._reward(x[:B]), bm._reward(x[B:])]).reshape(-1)  # the predictions are the plain reward model's, batch by batch
    assert reward_preds.shape == plain.shape and torch.allclose(reward_preds, plain, rtol=0, atol=1e-5)
    assert model.philox_seed == SEED


def test_cli_guided_tweedie_decode(tmp_path, capsys):
    """--method tweedie with the --guide_* flags: the decode runs under the GuidedReward, writes the usual npz and prints the term."""
    from svdd_amd import cli
    fixture = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "motifs_tiny.meme")
    args = cli.build_parser("tweedie").parse_args(["--task", "rna", "--batch_size", "8", "--sample_M", "2", "--rng", "philox",
                                                   "--out_dir", str(tmp_path), "--guide_motifs", fixture,
                                                   "--guide_weights", "MT0004.1=+2,MT0002.1=-1", "--guide_margin", "MT0005.1=0.01"])
    path, out = cli.run(args)
    with np.load(path) as f:
        assert f["decoding"].shape[0] == 8 and f["baseline"].shape[0] == 8
    assert len(out[0]) == 8 and path.endswith("rna-MRL_tw.npz")
    assert "motif term of the guided designs: mean" in capsys.readouterr().out
