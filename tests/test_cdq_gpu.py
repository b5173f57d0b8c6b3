"""-m gpu: the value function's training data, MC and CD-Q rollouts on the device (ABI 17).

  kernel    svdd_value_target against the numpy restatement tests/cdq_ref.py in sentinel-guarded buffers: tokens, one-hot and the
            MEAN target bit for bit; LOGMEANEXP special values exact, finite rows against float64 under a bar taken from the fp32
            restatement of the same formula
  fixtures  the reference's own _sample(cdq=True) / _sample() runs and eval-mode value targets (tests/golden/make_golden_cdq.py),
            replayed: g34 through the PyTorch modules, g35 through the hand-written kernels
  engine    value_targets against its own pieces, every knob, batch splits, weights changed between calls, train-mode nets, the
            harness's training forward, refusals
"""
import contextlib
import copy

import numpy as np
import pytest
import torch

from tests import cdq_ref as C
from tests import e2e_parity
from tests.conftest import load_golden
from tests.kernel_harness import DEV, _Buf, _st

pytestmark = pytest.mark.gpu
MASK = 4
LME_FACTOR = 8                     # bar of a finite LOGMEANEXP row = LME_FACTOR x max |fp32 restatement - float64| over its case table
FP32_EPS = 2.0 ** -23


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


# ------------------------------------------------------------------------------------------------ the kernel ----
PLANTS = [lambda M: np.r_[np.nan, np.zeros(M - 1)], lambda M: np.r_[np.zeros(M - 1), np.nan], lambda M: np.r_[np.inf, np.ones(M - 1)],
          lambda M: np.r_[-np.inf, np.ones(M - 1)], lambda M: np.r_[np.inf, -np.inf, np.zeros(M - 2)] if M > 1 else np.array([np.inf]),
          lambda M: np.r_[1e8, 1.0, -1e8, np.zeros(M - 3)] if M > 2 else np.full(M, 1e8),      # fl(1e8 + 1) = 1e8: a 1-ulp cancellation
          lambda M: np.r_[1.0, -1e8, 1e8, np.zeros(M - 3)] if M > 2 else np.full(M, -1e8),
          lambda M: np.full(M, 0.1), lambda M: np.full(M, -3.4e38), lambda M: np.full(M, -np.inf), lambda M: np.full(M, np.inf),
          lambda M: np.full(M, 1e-41)]                                                          # all equal; overflow; denormals


def _scores(B, M, rng, shift=0, scale=1.0):
    s = (rng.standard_normal((B, M)) * scale).astype(np.float32)
    for b in range(min(B, len(PLANTS))):
        s[b] = PLANTS[(b + shift) % len(PLANTS)](M).astype(np.float32)
    return s


def _launch(cand, scores=None, reduce="mean", alpha=1.0, want_onehot=True, misalign=0):
    """One svdd_value_target launch through the raw C entry, every output in a guarded sentinel buffer -> dict of numpy outputs
    (None where the buffer was not passed). misalign: byte offset of the cand / x_next rows' base."""
    from svdd_amd import _lib, ops
    L_ = _lib.lib()
    B, M, L = cand.shape
    raw = torch.zeros(cand.size + 8, dtype=torch.uint8, device=DEV)
    raw[misalign:misalign + cand.size] = torch.from_numpy(cand.reshape(-1)).to(DEV)
    sc = None if scores is None else dev(np.asarray(scores, np.float32))
    xn = _Buf(B * L + 8, torch.uint8)
    oh = _Buf(B * L * 4) if want_onehot else None
    tg = _Buf(B) if scores is not None else None
    rc = L_.svdd_value_target(None if sc is None else sc.data_ptr(), raw.data_ptr() + misalign, B, L, M, ops.TARGET_REDUCE[reduce],
                              float(alpha), xn.ptr + misalign, None if oh is None else oh.ptr, None if tg is None else tg.ptr, _st())
    _lib.check(rc, "svdd_value_target")
    torch.cuda.synchronize()
    mask = torch.zeros(B * L + 8, dtype=torch.bool)
    mask[misalign:misalign + B * L] = True
    xn.assert_written_where("x_next", mask)
    out = dict(x_next=xn.cpu().numpy()[misalign:misalign + B * L].reshape(B, L), onehot_next=None, target=None)
    if oh is not None:
        oh.assert_written("onehot_next")
        out["onehot_next"] = oh.cpu().numpy().reshape(B, L, 4)
    if tg is not None:
        tg.assert_written("target")
        out["target"] = tg.cpu().numpy()
    return out


def _same(got, ref, what):
    assert np.array_equal(got["x_next"], ref["x_next"]), (what, "x_next")
    if got["onehot_next"] is not None:
        assert got["onehot_next"].tobytes() == ref["onehot_next"].tobytes(), (what, "onehot_next")
    if got["target"] is not None:
        bad = np.flatnonzero(got["target"].view(np.uint32) != ref["target"].view(np.uint32))
        bad = [b for b in bad if not (np.isnan(got["target"][b]) and np.isnan(ref["target"][b]))]       # any NaN is a NaN
        assert not bad, (what, "target", bad[:5], got["target"][bad[:5]], ref["target"][bad[:5]])


def _mean_case(B, L, M, rng):
    cand = rng.integers(0, 5, (B, M, L)).astype(np.uint8)                     # MASK tokens included: their one-hot rows are zero
    s = _scores(B, M, rng, shift=L)
    ref = C.boundary(cand, s)
    _same(_launch(cand, s), ref, "mean")
    got = _launch(cand, s, want_onehot=False)
    assert got["onehot_next"] is None
    _same(got, ref, "mean, no one-hot")
    got = _launch(cand)                                                       # tokens only: step 0 of a rollout
    assert got["target"] is None
    _same(got, ref, "tokens only")
    assert np.array_equal(ref["onehot_next"].sum(-1), (cand[:, -1] != MASK).astype(np.float32))


@pytest.mark.parametrize("B", [1, 3, 257])
@pytest.mark.parametrize("L", [1, 3, 4, 5, 63, 64, 65, 200, 257])
def test_value_target_kernel_matches_the_restatement(L, B):
    """Every row shape (word and byte path, tails, more rows than a workgroup's four waves) at M = 10: the last draw, its one-hot and
    the sequential fp32 mean (planted NaN, +-inf, the 1e8 + 1 - 1e8 cancellation, all-equal, overflowing and denormal rows), bit for
    bit; with and without the one-hot; tokens only."""
    _mean_case(B, L, 10, np.random.default_rng(1000 * L + B))


@pytest.mark.parametrize("B", [1, 3, 257])
@pytest.mark.parametrize("L", [5, 200])
@pytest.mark.parametrize("M", [1, 2, 64, 65, 1024])
def test_value_target_kernel_every_draw_count(M, L, B):
    _mean_case(B, L, M, np.random.default_rng(7 * M + 1000 * L + B))


def test_value_target_mean_is_sequential_in_ascending_order():
    """Planted rows whose sequential fp32 sum differs from a pairwise / reversed / float64 one, and IEEE special values."""
    rng = np.random.default_rng(5)
    for M in (3, 10, 64):
        s = _scores(24, M, rng)
        cand = rng.integers(0, 4, (24, M, 7)).astype(np.uint8)
        got = _launch(cand, s)["target"]
        ref = C.seq_mean_f32(s)
        _same(dict(x_next=C.x_next(cand), onehot_next=None, target=got), dict(x_next=C.x_next(cand), target=ref), M)
        assert np.isnan(got[0]) and np.isnan(got[1]) and got[2] == np.inf and got[3] == -np.inf and np.isnan(got[4])
        assert got[5] == 0.0 and got[6] == 0.0                                # 1e8 + 1 - 1e8 and 1 - 1e8 + 1e8: both lose the 1
        assert got[9] == -np.inf and got[10] == np.inf
    s = np.array([[1e8, -1e8, 1.0]], np.float32)                              # the same three numbers in an order that keeps the 1
    assert _launch(np.zeros((1, 3, 4), np.uint8), s)["target"][0] == np.float32(1.0) / np.float32(3.0)
    # large random rows: a float64 mean differs from the sequential fp32 one somewhere, the kernel follows the latter
    s = (rng.standard_normal((64, 1024)) * 10).astype(np.float32)
    got = _launch(np.zeros((64, 1024, 4), np.uint8), s)["target"]
    assert got.tobytes() == C.seq_mean_f32(s).tobytes() and got.tobytes() != s.astype(np.float64).mean(1).astype(np.float32).tobytes()


@pytest.mark.parametrize("L", [64, 200])
def test_value_target_rows_at_an_odd_address_take_the_byte_path(L):
    """A multiple-of-4 length in token buffers that are not 4-byte aligned: same results as the aligned launch."""
    rng = np.random.default_rng(L)
    cand = rng.integers(0, 5, (5, 3, L)).astype(np.uint8)
    s = _scores(5, 3, rng)
    a = _launch(cand, s)
    for mis in (1, 2, 3):
        for oh in (True, False):
            b = _launch(cand, s, misalign=mis, want_onehot=oh)
            _same(b, a, ("misaligned", mis, oh))


@pytest.mark.parametrize("alpha", [0.1, 1.0, 10.0])
def test_value_target_logmeanexp(alpha):
    """Special values exact (NaN, +inf, all -inf, M = 1 gives the score itself); finite rows within LME_FACTOR x the error of the fp32
    numpy restatement of the same formula against the float64 one, per case table (floored at 2 ulp of the largest target, as
    tests/grad_ref.bar). Prints `ERR <case> <kernel error> bar <bar>` (profiles/value_target_kernel.txt)."""
    rng = np.random.default_rng(int(alpha * 10))
    one = np.zeros((1, 1, 4), np.uint8)
    for v in (0.37, -2.5e4, 0.0, 1e-41, -np.inf, np.inf):
        assert _launch(one, np.array([[v]], np.float32), "logmeanexp", alpha)["target"][0] == np.float32(v), v
    assert np.isnan(_launch(one, np.array([[np.nan]], np.float32), "logmeanexp", alpha)["target"][0])
    for M in (2, 10, 65, 1024):
        for scale in (0.01, 1.0, 100.0):
            B = 64
            s = (rng.standard_normal((B, M)) * scale + rng.standard_normal((B, 1)) * scale).astype(np.float32)
            s[0, 0], s[1, -1], s[2, 0], s[3] = np.nan, np.inf, -np.inf, -np.inf
            s[4, 0], s[4, 1] = np.nan, np.inf
            s[5] = 0.25 * scale                                               # all equal: exp(0) summed, log(1) = 0
            got = _launch(np.zeros((B, M, 4), np.uint8), s, "logmeanexp", alpha)["target"]
            r64, r32 = C.logmeanexp_f64(s, alpha), C.logmeanexp_f32(s, alpha)
            assert np.isnan(got[0]) and got[1] == np.inf and got[3] == -np.inf and np.isnan(got[4]) and np.isfinite(got[2])
            assert np.isnan(r64[0]) and r64[1] == np.inf and r64[3] == -np.inf and np.isnan(r64[4])
            fin = np.isfinite(r64)
            assert fin.sum() == B - 4 and np.isfinite(got[fin]).all()
            bar = max(LME_FACTOR * float(np.abs(r32[fin].astype(np.float64) - r64[fin]).max()), 2 * FP32_EPS * float(np.abs(r64[fin]).max()))
            err = float(np.abs(got[fin].astype(np.float64) - r64[fin]).max())
            print(f"ERR value_target_logmeanexp alpha={alpha} M={M} scale={scale} {err:.3e} bar {bar:.1e} (factor {LME_FACTOR})")
            assert err <= bar, (alpha, M, scale, err, bar)
            assert abs(float(got[5]) - 0.25 * scale) <= 2 * FP32_EPS * max(0.25 * scale, alpha)


def test_ops_value_target_and_refusals():
    from svdd_amd import _lib, ops
    rng = np.random.default_rng(11)
    cand, s = rng.integers(0, 5, (6, 4, 12)).astype(np.uint8), rng.standard_normal((6, 4)).astype(np.float32)
    ref = C.boundary(cand, s)
    slab, y, states = torch.zeros((2, 6, 12, 4), device=DEV), torch.zeros((2, 6), device=DEV), torch.zeros((2, 6, 12), dtype=torch.uint8, device=DEV)
    xn, oh, tg = ops.value_target(dev(s), dev(cand), x_next=states[1], onehot_next=slab[1], target=y[1])
    assert xn.data_ptr() == states[1].data_ptr() and tg.data_ptr() == y[1].data_ptr()
    _same(dict(x_next=states[1].cpu().numpy(), onehot_next=slab[1].cpu().numpy(), target=y[1].cpu().numpy()), ref, "slab slices")
    assert not states[0].any() and not slab[0].any() and not y[0].any()
    xn, oh, tg = ops.value_target(None, dev(cand))
    assert oh is None and tg is None and np.array_equal(xn.cpu().numpy(), ref["x_next"])
    xn, oh, tg = ops.value_target(dev(s), dev(cand), "logmeanexp", 0.5)
    assert np.allclose(tg.cpu().numpy(), C.logmeanexp_f64(s, 0.5), rtol=0, atol=1e-5)
    with pytest.raises(ValueError):
        ops.value_target(dev(s), dev(cand), "median")
    for f in (lambda: ops.value_target(dev(s), dev(cand), "logmeanexp", 0.0), lambda: ops.value_target(torch.from_numpy(s), dev(cand)),
              lambda: ops.value_target(dev(s), torch.from_numpy(cand)), lambda: ops.value_target(None, dev(cand), target=y[1]),
              lambda: ops.value_target(dev(s)[:, :3], dev(cand)), lambda: ops.value_target(dev(s), dev(cand), x_next=states[1, :5])):
        with pytest.raises(ops.SvddError):
            f()
    # the raw entry on live pointers: the refusals come before the launch
    L_, c, x = _lib.lib(), dev(cand), torch.zeros((6, 12), dtype=torch.uint8, device=DEV)
    sd, t = dev(s), torch.zeros(6, device=DEV)
    call = lambda *a: L_.svdd_value_target(*a, _st())                                       # noqa: E731
    ok = (sd.data_ptr(), c.data_ptr(), 6, 12, 4, 0, 1.0, x.data_ptr(), None, t.data_ptr())
    assert call(*ok) == _lib.OK
    bad = {"cand null": ok[:1] + (None,) + ok[2:], "x_next null": ok[:7] + (None,) + ok[8:], "M > MAX_M": ok[:4] + (1025,) + ok[5:],
           "reduce": ok[:5] + (7,) + ok[6:], "alpha": ok[:5] + (1, -1.0) + ok[7:], "scores alone": ok[:9] + (None,),
           "target alone": (None,) + ok[1:], "x_next is cand": ok[:7] + (c.data_ptr(),) + ok[8:], "B = 0": ok[:2] + (0,) + ok[3:]}
    for what, a in bad.items():
        assert call(*a) == _lib.E_ARG, what
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the engine ----
@pytest.fixture(scope="module")
def nets():
    """name -> (model, embedding, head, reward, B, S): the reference's tiny nets (PyTorch modules; the value net doubles as the
    reward model, as in g34), the full-size nets at L = 50 and at L = 200 (hand-written kernels)."""
    from svdd_amd import synthetic
    from svdd_amd.value_nets import RewardModel
    tiny = e2e_parity.tiny_engine(load_golden("nets_tiny.npz"), 50, 8, DEV)
    out = {"tiny": tiny + (RewardModel(tiny[1], tiny[2]), 8, 8)}
    out["full50"] = synthetic.build("rna", DEV) + (8, 6)
    out["full200"] = synthetic.build("dna", DEV) + (4, 5)
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


def _u8(t):
    return t.to(torch.uint8).cpu().numpy()


def _replay_fixture(g, model, emb, head, reward):
    """The engine in replay mode at the recorded seeds: _sample(cdq=True) against every recorded draw, mid, final and the generator's
    end state; value_targets("cdq") and ("mc") against the recorded states and targets. -> rows off the recorded trajectory (cdq, mc)."""
    S, draws = int(g["S"]), int(g["draws"])
    _, _, B, L = g["all_mid"].shape
    with knobs(model, rng_mode="replay"):
        torch.manual_seed(int(g["seed"]))
        x0, mid, all_mid = model._sample(num_steps=S, eval_sp_size=B, cdq=True)
        nxt = torch.rand(2)
        assert np.array_equal(nxt.numpy(), g["next"]), "the generator's end state (_sample cdq)"
        assert x0.dtype == torch.int64 and len(mid) == S - 1 and len(all_mid) == S and all(len(a) == draws for a in all_mid)
        assert all(m is a[-1] for m, a in zip(mid, all_mid)) and all(t.dtype == torch.int64 and t.shape == (B, L) for a in all_mid for t in a)
        am = np.stack([np.stack([_u8(t) for t in a]) for a in all_mid])
        off = (am != g["all_mid"]).any(axis=(0, 1, 3)) | (_u8(x0) != g["final"]).any(axis=1)
        torch.manual_seed(int(g["seed"]))
        vt = model.value_targets(emb, head, reward, mode="cdq", draws=draws, num_steps=S, eval_sp_size=B)
        assert np.array_equal(torch.rand(2).numpy(), g["next"]), "the generator's end state (value_targets cdq)"
        states, y = vt.states.cpu().numpy(), vt.y.cpu().numpy().reshape(S, B)
        assert np.array_equal(states[:-1], am[:-1, -1]) and np.array_equal(states[-1], _u8(x0)) and torch.equal(vt.x0, x0)
        assert np.array_equal(vt.onehot.cpu().numpy(), C.onehot(states).reshape(S * B, L, 4))
        want = np.concatenate([g["y_cdq"], g["reward"][None]])
        err = np.abs(y - want)[:, ~off]
        print(f"cdq: rows off {int(off.sum())} of {B}; max |y - recorded| on the others {err.max():.2e} (targets), "
              f"{np.abs(y[-1] - g['reward'])[~off].max():.2e} (reward)")
        assert err.max() <= 1e-4
        # the pairing is visible at this tolerance: the recorded targets shifted by one step are far from y
        assert np.abs(y[1:S - 1] - g["y_cdq"][:S - 2])[:, ~off].mean() > 5e-4
        torch.manual_seed(int(g["mc_seed"]))
        mc = model.value_targets(emb, head, reward, mode="mc", num_steps=S, eval_sp_size=B)
        assert np.array_equal(torch.rand(2).numpy(), g["mc_next"]), "the generator's end state (value_targets mc)"
        ms, my = mc.states.cpu().numpy(), mc.y.cpu().numpy().reshape(S, B)
        off_mc = (ms[:-1] != g["mc_mid"]).any(axis=(0, 2)) | (ms[-1] != g["mc_final"]).any(axis=1)
        assert np.array_equal(my, np.broadcast_to(my[-1], (S, B)))
        assert np.abs(my[-1] - g["mc_reward"])[~off_mc].max() <= 1e-4
        torch.manual_seed(int(g["mc_seed"]))
        px0, pmid = model._sample(num_steps=S, eval_sp_size=B)                # the path that was there before: same rollout
        assert torch.equal(px0, mc.x0) and np.array_equal(np.stack([_u8(t) for t in pmid]), ms[:-1])
    return int(off.sum()), int(off_mc.sum())


def test_recorded_reference_run_tiny_nets(nets):
    """g34 through the PyTorch modules on the device. Cap: at most 1 row may leave the recorded trajectory at a near-tie of an argmax
    (the condition of g32 / g33; the CPU restatement follows the recordings with 0 rows off, tests/test_cdq_cpu.py)."""
    model, emb, head, reward, *_ = nets["tiny"]
    off, off_mc = _replay_fixture(load_golden("g34_cdq_tiny.npz"), model, emb, head, reward)
    print(f"g34: rows off the recorded trajectory {off} (cdq) {off_mc} (mc) of 8")
    assert off <= 1 and off_mc <= 1


def test_recorded_reference_run_full_size_nets(nets):
    """g35: seed-44 full-size nets and reward model, L = 200, B = 3, 32 steps, through the hand-written kernels; same cap."""
    model, emb, head, reward, *_ = nets["full200"]
    g = load_golden("g35_cdq_full.npz")
    for nm, mod in (("backbone", model.backbone), ("embedding", emb), ("head", head), ("reward_embedding", reward.embedding),
                    ("reward_head", reward.head)):
        sums = np.array([float(p.double().sum()) for p in mod.state_dict().values()])
        assert np.allclose(sums, g[nm + "_param_sums"], rtol=0, atol=1e-6), nm
    from svdd_amd.fused import FusedValueNet
    assert isinstance(model.reward_callable(reward), FusedValueNet)
    off, off_mc = _replay_fixture(g, model, emb, head, reward)
    print(f"g35: rows off the recorded trajectory {off} (cdq) {off_mc} (mc) of 3")
    assert off <= 1 and off_mc <= 1


def _vt(model, emb, head, reward, B, S, seed=5, **kw):
    with knobs(model, rng_mode="philox", philox_seed=seed):
        return model.value_targets(emb, head, reward, **{**dict(mode="cdq", draws=4, num_steps=S, eval_sp_size=B), **kw})


def _same_vt(a, b):
    return (torch.equal(a.states, b.states) and torch.equal(a.y.view(torch.int32), b.y.view(torch.int32)) and torch.equal(a.x0, b.x0)
            and (a.onehot is None or b.onehot is None or torch.equal(a.onehot, b.onehot)))


@pytest.mark.parametrize("name", ["tiny", "full50", "full200"])
@pytest.mark.parametrize("reduce", ["mean", "logmeanexp"])
def test_value_targets_is_its_pieces(nets, name, reduce):
    """value_targets("cdq") against the same thing assembled from _sample(cdq=True)'s lists, per-draw value calls and cdq_ref: tokens
    equal; y bit for bit ("mean") given the scores the call itself used (model.trace), which agree with one value call per draw to
    the project's score tolerance; the last block is the reward of x_0."""
    from svdd_amd import ops
    model, emb, head, reward, B, S = nets[name]
    M, L = 4, model.config.model.length
    with knobs(model, trace=[]):
        vt = _vt(model, emb, head, reward, B, S, reduce=reduce, alpha=0.3)
        trace = model.trace
    assert vt.states.shape == (S, B, L) and vt.states.dtype == torch.uint8 and vt.onehot.shape == (S * B, L, 4) and vt.y.shape == (S * B,)
    assert vt.x0.dtype == torch.int64 and len(trace) == S + 1 and trace[0][1] is None
    with knobs(model, rng_mode="philox", philox_seed=5, cdq_draws=M), torch.no_grad():
        x0, mid, all_mid = model._sample(num_steps=S, eval_sp_size=B, cdq=True)
        fn = model.value_callable(emb, head)
        per_draw = np.stack([np.stack([fn(ops.transform_samples(c.to(torch.uint8))).reshape(B).float().cpu().numpy() for c in a])
                             for a in all_mid])                                # [S, M, B]
        r = model.reward_callable(reward)(ops.transform_samples(x0.to(torch.uint8), transposed=True)).reshape(B).float().cpu().numpy()
    used = np.stack([t[1].cpu().numpy().T for t in trace[1:S]])                # [S - 1, M, B]: what svdd_value_target reduced
    assert np.abs(used - per_draw[1:]).max() <= 1e-4
    red = C.seq_mean_f32 if reduce == "mean" else (lambda s: C.logmeanexp_f32(s, 0.3))
    values = np.concatenate([per_draw[:1], used])
    states, y = C.assemble_cdq(np.stack([np.stack([_u8(c) for c in a]) for a in all_mid]), values, _u8(x0), r, reduce=red)
    assert np.array_equal(vt.states.cpu().numpy(), states) and torch.equal(vt.x0, x0)
    assert np.array_equal(vt.onehot.cpu().numpy(), C.onehot(states).reshape(S * B, L, 4))
    got = vt.y.cpu().numpy()
    if reduce == "mean":
        assert got.tobytes() == y.tobytes()
    else:
        assert np.abs(got - y).max() <= 1e-5 and np.all(got[:(S - 1) * B] >= C.seq_mean_f32(np.moveaxis(used, 1, -1)).reshape(-1) - 1e-6)
    assert np.array_equal(got[(S - 1) * B:], r)
    assert _vt(model, emb, head, reward, B, S, reduce=reduce, alpha=0.3, want_onehot=False).onehot is None
    mc = _vt(model, emb, head, reward, B, S, mode="mc")
    with knobs(model, rng_mode="philox", philox_seed=5):
        px0, pmid = model._sample(num_steps=S, eval_sp_size=B)
    assert torch.equal(mc.x0, px0) and torch.equal(mc.states[:-1], torch.stack(pmid).to(torch.uint8)) and torch.equal(mc.states[-1], px0.to(torch.uint8))
    assert np.array_equal(mc.onehot.cpu().numpy(), C.onehot(mc.states.cpu().numpy()).reshape(S * B, L, 4))
    assert torch.equal(mc.y.view(S, B), mc.y[:B].expand(S, B))


@pytest.mark.parametrize("name", ["tiny", "full50", "full200"])
def test_value_targets_does_not_depend_on_the_engine_knobs(nets, name):
    model, emb, head, reward, B, S = nets[name]
    for mode in ("cdq", "mc"):
        base = _vt(model, emb, head, reward, B, S, mode=mode)
        for kw in (dict(skip_unchanged=False), dict(logits_cache="on"), dict(logits_cache="off"), dict(incremental_backbone="on"),
                   dict(incremental_backbone="off"), dict(dedup_prior=False), dict(skip_unchanged=False, dedup_prior=False, logits_cache="off")):
            with knobs(model, **kw):
                assert _same_vt(_vt(model, emb, head, reward, B, S, mode=mode), base), (mode, kw)
    assert not torch.equal(_vt(model, emb, head, reward, B, S, seed=6).states, base.states)


@pytest.mark.parametrize("name", ["full50", "full200"])
def test_value_targets_rows_do_not_depend_on_how_the_batch_is_split(nets, name):
    """Philox mode: rows lo .. lo + n of a whole-batch call = the call on n rows at row_offset = lo (tokens and targets, bit for bit:
    the hand-written kernels' output for a row does not depend on the batch around it)."""
    model, emb, head, reward, B, S = nets[name]
    for mode in ("cdq", "mc"):
        whole = _vt(model, emb, head, reward, B, S, mode=mode)
        for lo, n in ((0, 1), (1, B - 1)):
            with knobs(model, row_offset=lo):
                part = _vt(model, emb, head, reward, n, S, mode=mode)
            assert torch.equal(part.states, whole.states[:, lo:lo + n]), (mode, lo)
            assert torch.equal(part.y.view(S, n).view(torch.int32), whole.y.view(S, B)[:, lo:lo + n].contiguous().view(torch.int32)), (mode, lo)


def _trainable(emb, head):
    emb, head = copy.deepcopy(emb), copy.deepcopy(head)
    for p in list(emb.parameters()) + list(head.parameters()):
        p.requires_grad_(True)
    return emb, head


def test_weights_changed_in_place_between_two_calls(nets):
    """One SGD step on embedding and head (the train-mode forward also moves the BatchNorm running statistics): the next call's
    targets are those of a freshly constructed Diffusion on copies of the updated nets, and differ from the first call's."""
    from svdd_amd.diffusion import Diffusion
    from svdd_amd.fused import FusedValueNet
    model, emb, head, reward, B, S = nets["full50"]
    emb, head = _trainable(emb, head)
    first = _vt(model, emb, head, reward, B, S)
    assert isinstance(model.value_callable(emb, head), FusedValueNet)
    bn = [m for m in emb.modules() if isinstance(m, torch.nn.BatchNorm1d)]
    rm = [m.running_mean.clone() for m in bn]
    opt = torch.optim.SGD(list(emb.parameters()) + list(head.parameters()), lr=0.05)
    emb.train(), head.train()
    torch.manual_seed(3)
    loss = ((head(emb(first.onehot)).view(-1) - first.y - 1.0) ** 2).mean()
    loss.backward()
    opt.step()
    emb.eval(), head.eval()
    assert bn and any(not torch.equal(a, m.running_mean) for a, m in zip(rm, bn))
    second = _vt(model, emb, head, reward, B, S)
    fresh = Diffusion(model.config, backbone=copy.deepcopy(model.backbone)).to(DEV).eval()
    third = _vt(fresh, copy.deepcopy(emb), copy.deepcopy(head), copy.deepcopy(reward), B, S)
    assert _same_vt(second, third)
    assert torch.equal(second.states, first.states)                           # the rollout does not involve the value net
    n = (S - 1) * B
    assert not torch.equal(second.y[:n], first.y[:n]) and torch.equal(second.y[n:], first.y[n:])
    assert (second.y[:n] - first.y[:n]).abs().max() > 1e-4


def test_train_mode_nets_give_eval_mode_targets_and_come_back_in_train_mode(nets):
    for name in ("tiny", "full50"):
        model, emb, head, reward, B, S = nets[name]
        emb, head = _trainable(emb, head)
        ref = _vt(model, emb, head, reward, B, S)
        emb.train(), head.train()
        assert any(isinstance(m, torch.nn.Dropout) and m.p == 0.1 for m in emb.modules())
        frozen_one = next(m for m in emb.modules() if isinstance(m, torch.nn.BatchNorm1d))
        frozen_one.eval()                                                     # a caller's mixed modes survive the call too
        a = _vt(model, emb, head, reward, B, S)
        b = _vt(model, emb, head, reward, B, S)
        assert _same_vt(a, b) and _same_vt(a, ref)
        assert emb.training and head.training and not frozen_one.training
        assert all(m.training for m in emb.modules() if m is not frozen_one) and all(m.training for m in head.modules())


@pytest.mark.parametrize("cdq,alpha", [(False, None), (True, None), (True, 0.5)])
def test_harness_training_forward(nets, cdq, alpha):
    """BaseModel.forward() in training mode = loss_fct(head(embedding(vt.onehot)).view(-1), vt.y) for the value_targets of the same
    seed; backward fills the value net's gradients and nobody else's."""
    from svdd_amd.harness import BaseModel
    model, emb, head, reward, B, S = nets["full50"]
    emb, head = _trainable(emb, head)
    steps = model.config.sampling.steps
    model.config.sampling.steps = S
    try:
        h = BaseModel(emb, head, model, reward, B, task="rna", cdq=cdq, cdq_alpha=alpha)
        h.cdq_draws = 4
        kw = dict(mode="cdq" if cdq else "mc", reduce="mean" if alpha is None else "logmeanexp", alpha=1.0 if alpha is None else alpha)
        vt = _vt(model, emb, head, reward, B, S, **kw)
        h.train()
        assert not model.training and not reward.training and emb.training
        with knobs(model, rng_mode="philox", philox_seed=5):
            torch.manual_seed(9)
            loss = h()
        assert _same_vt(h.last_targets, vt) and emb.training and head.training
        torch.manual_seed(9)                                                  # the same dropout masks
        want = torch.nn.functional.mse_loss(head(emb(vt.onehot)).view(-1), vt.y)
        assert loss.shape == () and loss.requires_grad and torch.allclose(loss, want, rtol=1e-5, atol=0)
        loss.backward()
        pe, ph = _trainable(emb, head)                                        # which parameters a forward reaches at all (some are
        ph(pe(vt.onehot[:2])).sum().backward()                                # registered and never applied, as in the reference)
        reached = [[n for n, p in m.named_parameters() if p.grad is not None] for m in (pe, ph)]
        filled = [[n for n, p in m.named_parameters() if p.grad is not None] for m in (emb, head)]
        assert filled == reached and len(reached[0]) > 10 and reached[1]
        grads = [p.grad for m in (emb, head) for p in m.parameters() if p.grad is not None]
        assert all(bool(torch.isfinite(g).all()) for g in grads) and any(float(g.abs().max()) > 0 for g in grads)
        assert all(p.grad is None for m in (model, reward) for p in m.parameters())
        h.eval()
        x, y = vt.onehot[:B], vt.y[:B]
        assert torch.allclose(h(x0=x, y=y), torch.nn.functional.mse_loss(head(emb(x)).view(-1), y), rtol=1e-6, atol=0)
    finally:
        model.config.sampling.steps = steps


def test_refusals(nets):
    from svdd_amd import ops
    from svdd_amd.harness import BaseModel
    from svdd_amd.value_nets import ConvHead, RewardModel
    model, emb, head, reward, B, S = nets["tiny"]
    vt = lambda e=emb, h=head, r=reward, **kw: _vt(model, e, h, r, B, 2, **kw)                     # noqa: E731
    two = ConvHead(2, 8).to(DEV).eval()
    for f in (lambda: vt(h=two), lambda: vt(r=RewardModel(emb, two)), lambda: vt(h=two, mode="mc")):
        with pytest.raises(NotImplementedError):
            f()
    for f in (lambda: vt(mode="td"), lambda: vt(reduce="median"), lambda: vt(alpha=0.0), lambda: vt(alpha=-1.0),
              lambda: vt(alpha=float("nan")), lambda: vt(alpha=float("inf"), reduce="logmeanexp"), lambda: vt(draws=0),
              lambda: vt(draws=1025), lambda: vt(draws=2.5)):
        with pytest.raises(ValueError):
            f()
    for f in (lambda: vt(e=copy.deepcopy(emb).cpu()), lambda: vt(h=copy.deepcopy(head).cpu()),
              lambda: vt(r=copy.deepcopy(reward).cpu()), lambda: vt(r=copy.deepcopy(reward).cpu(), mode="mc")):
        with pytest.raises(ops.SvddError):
            f()
    with knobs(model, rng_mode="philox", cdq_draws=0):
        with pytest.raises(ValueError):
            model._sample(num_steps=2, eval_sp_size=2, cdq=True)
    h = BaseModel(emb, head, model, reward, B, task="rna", n_tasks=2).train()
    with pytest.raises(NotImplementedError):
        h()
    h.eval()
    assert emb.training is False and model.rng_mode == "replay"


def test_train_value_cli(tmp_path):
    """train_value.py's implementation, in-process: a few AdamW iterations of BaseModel.forward, the loss printed per iteration, and a
    checkpoint in the layout the decode scripts' --load_checkpoint_path reads."""
    from svdd_amd import cli, synthetic
    from svdd_amd.value_nets import load_reference_state_dict
    out = str(tmp_path / "value.pt")
    for extra in ([], ["--cdq"], ["--cdq_alpha", "0.5"]):
        path, losses = cli.main_train(["--task", "rna", "--batch_size", "4", "--steps", "4", "--iters", "2", "--lr", "1e-3", "--out", out] + extra)
        assert path == out and len(losses) == 2 and all(np.isfinite(v) for v in losses)
    sd = torch.load(out, map_location="cpu")["model_state_dict"]
    _, emb, head, _ = synthetic.build("rna", DEV)
    before = [p.detach().clone() for p in emb.parameters()]
    load_reference_state_dict(emb, {k[len("embedding."):]: v for k, v in sd.items() if k.startswith("embedding.")})
    load_reference_state_dict(head, {k[len("head."):]: v for k, v in sd.items() if k.startswith("head.")})
    assert any(not torch.equal(a, b) for a, b in zip(before, emb.parameters()))       # the optimiser moved the weights
