"""-m gpu: in-silico mutagenesis and ISM-driven directed evolution on the device.

  kernels   svdd_ism_mutants, svdd_ism_fold, svdd_evolve_apply against the host restatement tests/ism_ref.py in sentinel-guarded
            buffers, exactly: every shape path, dead rows, a bad token, ties, NaN, +-inf, an all-NaN row, every chunking, both stop
            modes, launches after the stop
  engine    Diffusion.ism_scores against forward_tokens on every mutant, bit for bit (windowed tower at L = 200 / 105, whole
            sequences at L = 33; fp32 and f16x3; one position per chunk against one chunk); Diffusion.evolve against evolve_ref driven
            by the same scores, exactly (windowed route, and the opaque route with the tiny value net); the harness entries
  fixtures  g36 / g37: the reference's own nets on every mutant, one at a time, on the CPU (tests/golden/make_golden_ism.py),
            within the project's soft-value bar of 1e-4
"""
import contextlib

import numpy as np
import pytest
import torch

from tests import e2e_parity
from tests import ism_ref as R
from tests.conftest import load_golden
from tests.kernel_harness import DEV, _Buf, _st

pytestmark = pytest.mark.gpu
SOFT_BAR = 1e-4                    # README: "soft values within 1e-4"


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.float32 else np.ascontiguousarray(a)


def _same_bits(got, want, what):
    """Equal bit for bit, except that any NaN equals any NaN."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = _bits(got) != _bits(want)
    if got.dtype == np.float32:
        bad &= ~(np.isnan(got) & np.isnan(want))
    assert not bad.any(), (what, np.argwhere(bad)[:5].tolist(), got[bad][:5], want[bad][:5])


# ------------------------------------------------------------------------------------------------ svdd_ism_mutants ----
def _positions(L, P):
    if P == L:
        return list(range(L))
    return sorted({0, L - 1} | {int(v) for v in np.linspace(0, L - 1, P).round()})[:P - 1] + [L - 1] if P > 1 else [0]


def _mutants(x, positions, live=None, want_onehot=True, misalign=0):
    """One svdd_ism_mutants launch through the raw C entry, outputs in guarded sentinel buffers -> (cand, onehot | None, err)."""
    from svdd_amd import _lib
    B, L = x.shape
    P = len(positions)
    n = B * 3 * P
    raw = torch.zeros(x.size + 8, dtype=torch.uint8, device=DEV)
    raw[misalign:misalign + x.size] = dev(x.reshape(-1))
    pos = dev(np.asarray(positions, np.int32))
    lv = None if live is None else dev(np.asarray(live, np.uint8))
    cand, oh, err = _Buf(n * L + 8, torch.uint8), (_Buf(n * L * 4) if want_onehot else None), torch.zeros(1, dtype=torch.int32, device=DEV)
    rc = _lib.lib().svdd_ism_mutants(raw.data_ptr() + misalign, pos.data_ptr(), None if lv is None else lv.data_ptr(), B, L, P,
                                     cand.ptr + misalign, None if oh is None else oh.ptr, err.data_ptr(), _st())
    _lib.check(rc, "svdd_ism_mutants")
    torch.cuda.synchronize()
    mask = torch.zeros(n * L + 8, dtype=torch.bool)
    mask[misalign:misalign + n * L] = True
    cand.assert_written_where("cand", mask)
    out = cand.cpu().numpy()[misalign:misalign + n * L].reshape(B, 3 * P, L)
    if oh is not None:
        oh.assert_written("onehot")
    return out, (None if oh is None else oh.cpu().numpy().reshape(n, L, 4)), int(err[0])


@pytest.mark.parametrize("B,L,P", [(1, 1, 1), (3, 7, 7), (2, 105, 105), (3, 200, 200), (2, 208, 5)])
def test_ism_mutants_kernel_matches_the_restatement(B, L, P):
    """Tokens and one-hot exact, guards intact; word path (L % 4 == 0) and byte path, more mutants than a workgroup's four waves,
    positions 0 and L - 1; with and without the one-hot; a misaligned base takes the byte path with the same result."""
    rng = np.random.default_rng(100 * L + B)
    x = rng.integers(0, 4, (B, L)).astype(np.uint8)
    pos = _positions(L, P)
    assert len(pos) == P and pos[0] == 0 and pos[-1] == L - 1 and all(b > a for a, b in zip(pos, pos[1:]))
    want = R.mutants_ref(x, pos)
    cand, oh, err = _mutants(x, pos)
    assert err == 0 and np.array_equal(cand, want) and oh.tobytes() == R.onehot_ref(want).reshape(-1, L, 4).tobytes()
    assert (cand != x[:, None, :]).sum(-1).tolist() == [[1] * (3 * P)] * B                # exactly one changed position each
    cand, oh, err = _mutants(x, pos, want_onehot=False)
    assert oh is None and err == 0 and np.array_equal(cand, want)
    cand, oh, err = _mutants(x, pos, misalign=1)
    assert err == 0 and np.array_equal(cand, want) and oh.tobytes() == R.onehot_ref(want).reshape(-1, L, 4).tobytes()


@pytest.mark.parametrize("L", [7, 200])
def test_ism_mutants_dead_rows_and_bad_tokens(L):
    from svdd_amd import fused
    rng = np.random.default_rng(L)
    x = rng.integers(0, 4, (3, L)).astype(np.uint8)
    pos = list(range(L))
    live = [1, 0, 1]
    want = R.mutants_ref(x, pos, live)
    cand, oh, err = _mutants(x, pos, live)
    assert err == 0 and np.array_equal(cand, want) and oh.tobytes() == R.onehot_ref(want).reshape(-1, L, 4).tobytes()
    assert (cand[1] == x[1]).all() and (cand[0] != x[0]).sum() == 3 * L
    # svdd_candidate_windows on these buffers: a dead row's copies are flagged 0 (the compaction drops them), a mutant never is
    flags = torch.empty(3 * 3 * L, dtype=torch.int32, device=DEV)
    win = fused.candidate_windows(dev(cand), dev(x), flags=flags).cpu().numpy().reshape(3, 3 * L, 2)
    flags = flags.cpu().numpy().reshape(3, 3 * L)
    assert (flags[1] == 0).all() and (flags[[0, 2]] >= 1).all() and (win[1] == 0).all()
    p = np.repeat(pos, 3)
    assert (win[0, :, 0] <= p).all() and (win[0, :, 1] > p).all() and (win[0] % 16 == 0).all()
    # a token 4 in a parent: err is set, the token is copied through, its one-hot row is zero, the position offers copies
    xb = x.copy()
    xb[2, L // 2] = 4
    want = R.mutants_ref(xb, pos)
    cand, oh, err = _mutants(xb, pos)
    assert err == 1 and np.array_equal(cand, want) and oh.tobytes() == R.onehot_ref(want).reshape(-1, L, 4).tobytes()
    assert (cand[2, :, L // 2] == 4).all() and (oh.reshape(3, 3 * L, L, 4)[2, :, L // 2] == 0).all()


def test_ops_ism_mutants_and_refusals():
    from svdd_amd import ops
    x = np.random.default_rng(3).integers(0, 4, (2, 12)).astype(np.uint8)
    pos = torch.tensor([0, 5, 11], dtype=torch.int32, device=DEV)
    cand, oh = ops.ism_mutants(dev(x), pos)
    assert np.array_equal(cand.cpu().numpy(), R.mutants_ref(x, [0, 5, 11])) and oh.shape == (18, 12, 4)
    xb = x.copy()
    xb[0, 0] = 4
    with pytest.raises(ops.SvddError, match="token > 3"):
        ops.ism_mutants(dev(xb), pos)
    with pytest.raises(ops.SvddError, match="outside"):
        ops.ism_mutants(dev(x), torch.tensor([0, 12], dtype=torch.int32, device=DEV))      # flagged on the device, nothing out of bounds
    for f in (lambda: ops.ism_mutants(torch.from_numpy(x), pos), lambda: ops.ism_mutants(dev(x), pos.cpu()),
              lambda: ops.ism_mutants(dev(x), pos, cand=torch.empty((2, 9, 11), dtype=torch.uint8, device=DEV)),
              lambda: ops.ism_mutants(dev(x), pos.long())):
        with pytest.raises(ops.SvddError):
            f()


# ------------------------------------------------------------------------------------------------ svdd_ism_fold ----
def _synthetic_scores(B, P, rng):
    """[B, 3P]: small integers (many exact ties), planted NaN, +-inf; row 1 all NaN, row 2 all -inf, row 3 ends in +inf twice."""
    s = rng.integers(-3, 4, (B, 3 * P)).astype(np.float32)
    s[0, ::5] = np.nan
    s[0, 1] = np.inf
    if B > 1:
        s[1] = np.nan
    if B > 2:
        s[2] = -np.inf
    if B > 3:
        s[3, -2:] = np.inf
        s[3, 0] = -np.inf
    return s


def _fold(s, ps, x, pos, chunk, live=None, with_ism=True, with_best=True, slot_route=False):
    from svdd_amd import _lib
    B, L = x.shape
    P = len(pos)
    xd, posd, psd = dev(x), dev(np.asarray(pos, np.int32)), dev(ps)
    lv = None if live is None else dev(np.asarray(live, np.uint8))
    ism = _Buf(B * P * 4) if with_ism else None
    bs, bp, ba = (_Buf(B), _Buf(B, torch.int32), _Buf(B, torch.int32)) if with_best else (None, None, None)
    ptr = lambda b: None if b is None else b.ptr                                           # noqa: E731
    for p0 in range(0, P, chunk):
        pc = min(chunk, P - p0)
        sc = np.ascontiguousarray(s[:, 3 * p0:3 * (p0 + pc)])
        slot = None
        if slot_route:                                   # the compacted form: only the live rows' scores, in a shuffled order
            keep = np.flatnonzero(np.repeat(np.ones(B, bool) if live is None else np.asarray(live, bool), 3 * pc))
            order = np.random.default_rng(p0).permutation(len(keep))
            slot_np = np.full(B * 3 * pc, -1, np.int32)
            slot_np[keep[order]] = np.arange(len(keep), dtype=np.int32)
            sc = np.concatenate([sc.reshape(-1)[keep[order]], np.full(3, 777.0, np.float32)])  # rows past the count: never read
            slot = dev(slot_np)
        scd = dev(sc)
        rc = _lib.lib().svdd_ism_fold(scd.data_ptr(), None if slot is None else slot.data_ptr(), psd.data_ptr(), xd.data_ptr(),
                                      posd.data_ptr(), None if lv is None else lv.data_ptr(), B, L, P, p0, pc, ptr(ism), ptr(bs), ptr(bp),
                                      ptr(ba), _st())
        _lib.check(rc, "svdd_ism_fold")
    torch.cuda.synchronize()
    for b in (ism, bs, bp, ba):
        if b is not None:
            b.assert_written("fold output")
    return (None if ism is None else ism.cpu().numpy().reshape(B, P, 4),
            None if bs is None else (bs.cpu().numpy(), bp.cpu().numpy(), ba.cpu().numpy()))


@pytest.mark.parametrize("B,L,P", [(1, 4, 1), (5, 30, 7), (6, 200, 200), (3, 9, 65)])
def test_ism_fold_kernel_matches_the_restatement_in_every_chunking(B, L, P):
    """The table and the running best against fold_ref, exactly (first mutant wins a tie, a NaN and -inf never win, the all-NaN
    row keeps (-inf, -1, -1)); chunks of 1, 3 and all positions give identical bits; the compacted (slot) form of the same scores
    and a dead row likewise; either output alone."""
    rng = np.random.default_rng(B * 1000 + P)
    L = max(L, P)
    x = rng.integers(0, 4, (B, L)).astype(np.uint8)
    pos = sorted(rng.choice(L, P, replace=False).tolist())
    s, ps = _synthetic_scores(B, P, rng), rng.standard_normal(B).astype(np.float32)
    for live in (None, [b % 3 != 1 for b in range(B)]):
        want_ism, want_best = np.empty((B, P, 4), np.float32), R.new_best(B)
        R.fold_ref(s, ps, x, pos, 0, P, want_ism, want_best, live)
        if live is None and B > 2:
            assert want_best[1][1] == -1 and want_best[1][2] == -1 and want_best[0][2] == -np.inf
        for chunk in (1, 3, P):
            for slot_route in (False, True):
                ism, best = _fold(s, ps, x, pos, chunk, live, slot_route=slot_route)
                if slot_route and live is not None:      # a dead row's mutants are copies with the parent's score
                    dead = ~np.asarray(live, bool)
                    w = want_ism.copy()
                    w[dead] = ps[dead, None, None]
                    _same_bits(ism, w, ("ism", chunk, "slot"))
                else:
                    _same_bits(ism, want_ism, ("ism", chunk, slot_route))
                for g, w, nm in zip(best, want_best, ("best_score", "best_pos", "best_allele")):
                    _same_bits(g, w, (nm, chunk, slot_route, live))
        ism, best = _fold(s, ps, x, pos, 3, live, with_best=False)
        assert best is None
        _same_bits(ism, want_ism, "ism alone")
        ism, best = _fold(s, ps, x, pos, 3, live, with_ism=False)
        assert ism is None and all(_bits(g).tobytes() == _bits(w).tobytes() for g, w in zip(best, want_best))


# ------------------------------------------------------------------------------------------------ svdd_evolve_apply ----
class _State:
    """The in-place state of svdd_evolve_apply in guarded buffers, mirrored by numpy arrays that apply_ref updates."""

    def __init__(self, x, score, stop):
        B, L = x.shape
        self.B, self.L, self.stop = B, L, stop
        self.np = dict(x=x.copy(), cur=score.copy(), live=np.ones(B, np.uint8) if stop == "row" else None, x_best=x.copy(),
                       score_best=score.copy())
        m0 = R.NEG_INF
        for v in score:
            if v > m0:
                m0 = v
        self.state = {"best_so_far": m0, "stopped": False}
        self.buf = dict(x=_Buf(B * L, torch.uint8), cur=_Buf(B), live=_Buf(B, torch.uint8), bsf=_Buf(1), stopped=_Buf(1, torch.int32),
                        x_best=_Buf(B * L, torch.uint8), score_best=_Buf(B))
        for k, v in (("x", x), ("cur", score), ("live", np.ones(B, np.uint8)), ("bsf", np.array([m0], np.float32)),
                     ("stopped", np.zeros(1, np.int32)), ("x_best", x), ("score_best", score)):
            self.buf[k].body().copy_(dev(np.ascontiguousarray(v).reshape(-1)))

    def launch(self, best):
        from svdd_amd import _lib
        B = self.B
        bs, bp, ba = (dev(a) for a in best)
        tr = (_Buf(B, torch.int32), _Buf(B, torch.int32), _Buf(B), _Buf(B, torch.uint8))
        b = self.buf
        rc = _lib.lib().svdd_evolve_apply(bs.data_ptr(), bp.data_ptr(), ba.data_ptr(), B, self.L, {"global": 0, "row": 1}[self.stop],
                                          b["x"].ptr, b["cur"].ptr, b["live"].ptr if self.stop == "row" else None, b["bsf"].ptr,
                                          b["stopped"].ptr, b["x_best"].ptr, b["score_best"].ptr, *[t.ptr for t in tr], _st())
        _lib.check(rc, "svdd_evolve_apply")
        torch.cuda.synchronize()
        return tr

    def snapshot(self):
        for v in self.buf.values():
            v.untouched()                                # asserts the guards
        return {k: v.bits().cpu().numpy().copy() for k, v in self.buf.items()}

    def check(self, what):
        n, b = self.np, self.buf
        assert np.array_equal(b["x"].cpu().numpy().reshape(self.B, self.L), n["x"]), (what, "x")
        assert np.array_equal(b["x_best"].cpu().numpy().reshape(self.B, self.L), n["x_best"]), (what, "x_best")
        _same_bits(b["cur"].cpu().numpy(), n["cur"], (what, "score_cur"))
        _same_bits(b["score_best"].cpu().numpy(), n["score_best"], (what, "score_best"))
        _same_bits(b["bsf"].cpu().numpy(), np.array([self.state["best_so_far"]], np.float32), (what, "best_so_far"))
        assert int(b["stopped"].cpu()[0]) == int(self.state["stopped"]), (what, "stopped")
        if self.stop == "row":
            assert np.array_equal(b["live"].cpu().numpy(), n["live"]), (what, "live")


@pytest.mark.parametrize("stop", ["global", "row"])
@pytest.mark.parametrize("B,L", [(1, 1), (5, 7), (37, 200), (1100, 12)])
def test_evolve_apply_kernel_matches_the_restatement(B, L, stop):
    """Iterations of synthetic picks (ties with the row's score, NaN, +-inf, rows without a pick, picks at positions 0 and L - 1)
    through the kernel and apply_ref: every state buffer and the trace equal after every launch; a launch after `stopped` is set
    changes nothing (all buffers compared before and after, trace buffers untouched). B = 1100: more rows than the one workgroup
    has threads."""
    rng = np.random.default_rng(B * 10 + L + (stop == "row"))
    x = rng.integers(0, 4, (B, L)).astype(np.uint8)
    score = rng.integers(-2, 3, B).astype(np.float32)
    st = _State(x, score, stop)
    stopped_at = None
    for it in range(12):
        rising = it < 4                                  # the first iterations keep the batch maximum rising; from the 7th on no
        hi = 3 if rising else 2 if it < 6 else 1         # pick beats its row's score (ties and losses only): both modes stop there
        bs = (st.np["cur"] + rng.integers(-1, hi, B)).astype(np.float32)
        if rising and B > 1:
            bs[rng.integers(0, B)] = st.state["best_so_far"] + 1
        bp = rng.integers(0, L, B).astype(np.int32)
        ba = rng.integers(0, 4, B).astype(np.int32)
        bp[0] = (0, L - 1)[it % 2]
        if B > 4:
            bs[1], bs[2] = np.nan, -np.inf
            bp[3], ba[3], bs[3] = -1, -1, -np.inf        # a row without a pick
            bs[4] = np.inf if it == 2 else bs[4]
            bs[3] = -np.inf
        best = (bs, bp, ba)
        before = st.snapshot()
        tr = st.launch(best)
        want = R.apply_ref(best, stop, st.np["x"], st.np["cur"], st.np["live"], st.state, st.np["x_best"], st.np["score_best"])
        if want is None:                                 # already stopped: nothing is written, not even the trace
            after = st.snapshot()
            assert all(np.array_equal(before[k], after[k]) for k in before), it
            for t in tr:
                t.assert_untouched("trace after the stop")
            continue
        for t, w, nm in zip(tr, want, ("position", "allele", "score", "taken")):
            t.assert_written(nm)
            _same_bits(t.cpu().numpy(), w, (it, nm))
        st.check(it)
        if st.state["stopped"] and stopped_at is None:
            stopped_at = it
    assert stopped_at is not None and stopped_at < 11, "the case never reached (and re-entered) the stopped state"


# ------------------------------------------------------------------------------------------------ the engine ----
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


@pytest.fixture(scope="module")
def nets():
    """"full": the full-size seeded nets with every convolution and norm of the value net and the reward model re-drawn
    (net_ref.distinct_layers: no two layers of a tower equal); "plain": the seed-44 nets of g37 as they are; "tiny": the
    reference's 8-channel value net (PyTorch modules: the opaque route)."""
    from svdd_amd import synthetic
    from tests.net_ref import distinct_layers
    full = synthetic.build("dna", DEV)
    distinct_layers(full[1], seed=1)
    distinct_layers(full[3].embedding, seed=2)
    return {"full": full, "plain": synthetic.build("dna", DEV), "tiny": e2e_parity.tiny_engine(load_golden("nets_tiny.npz"), 50, 8, DEV)}


def _x(B, L, seed):
    return np.random.default_rng(seed).integers(0, 4, (B, L)).astype(np.uint8)


def _table_from_forward_tokens(fn, x, pos):
    """The [B, P, 4] table assembled on the host from fn.forward_tokens on every mutant's tokens (and on the parents)."""
    B, L = x.shape
    score = lambda t: fn.forward_tokens(dev(t)).reshape(len(t), -1)[:, 0].float().cpu().numpy()      # noqa: E731
    return R.ism_ref(x, pos, score), score(x)


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
@pytest.mark.parametrize("L", [200, 105, 33])
def test_ism_scores_equal_forward_tokens_bit_for_bit(nets, L, precision):
    """B = 3, all positions: every entry is fn.forward_tokens on that mutant's tokens, bit for bit (torch.equal), the parent-base
    entries the parent's own score; one position per chunk gives the bits of one chunk. L = 200 and 105 take the windowed tower
    (one 16-aligned row window per mutant, the rest copied from the parent's tower output), L = 33 whole sequences."""
    from svdd_amd.fused import FusedValueNet
    model, emb, head, _ = nets["full"]
    x = _x(3, L, L)
    with knobs(model, precision=precision):
        fn = model.value_callable(emb, head)
        assert isinstance(fn, FusedValueNet) and fn.precision == precision
        assert (model._ism_route(emb, head, None, L)[1] is fn) == (L > 104)
        ism = model.ism_scores(dev(x), emb, head)
        want, parent = _table_from_forward_tokens(fn, x, list(range(L)))
        one = model.ism_scores(dev(x).long(), emb, head, chunk_rows=9)
        sub = model.ism_scores(dev(x), emb, head, positions=[0, L // 2, L - 1], compare="subtract")
        fc = model.ism_scores(dev(x), emb, head, positions=[0, L // 2, L - 1], compare="log2FC")
    assert ism.dtype == torch.float32 and ism.shape == (3, L, 4) and not torch.isnan(ism).any()
    assert torch.equal(ism.cpu(), torch.from_numpy(want))
    own = ism.cpu().numpy()[np.arange(3)[:, None], np.arange(L)[None, :], x]
    assert own.tobytes() == np.broadcast_to(parent[:, None], (3, L)).astype(np.float32).tobytes()
    assert torch.equal(one, ism)
    # a mutant's score differs from its parent's nearly everywhere: the table is not the parent's score repeated
    assert float((ism.cpu() != torch.from_numpy(parent)[:, None, None]).float().mean()) > 0.7
    pick = ism[:, [0, L // 2, L - 1]]
    ref = torch.from_numpy(parent).to(DEV)[:, None, None]
    assert torch.equal(sub, pick - ref) and torch.equal(torch.nan_to_num(fc), torch.nan_to_num(torch.log2(pick / ref)))


def test_ism_scores_reward_layout_and_the_harness(nets):
    """reward_model given: the [n, 4, L]-layout reward net (fused: the windowed route) scores; BaseModel.ism_predict is that call."""
    from svdd_amd.fused import FusedValueNet
    from svdd_amd.harness import BaseModel
    model, emb, head, reward = nets["full"]
    x = _x(2, 200, 9)
    fn = model.reward_callable(reward)
    assert isinstance(fn, FusedValueNet)
    pos = [0, 17, 18, 100, 199]
    ism = model.ism_scores(dev(x), emb, head, reward_model=reward, positions=pos)
    want, _ = _table_from_forward_tokens(fn, x, pos)
    assert torch.equal(ism.cpu(), torch.from_numpy(want))
    assert not torch.equal(ism, model.ism_scores(dev(x), emb, head, positions=pos))           # the value net is another net
    h = BaseModel(emb, head, model, reward, 2)
    assert torch.equal(h.ism_predict(dev(x), positions=pos), ism)
    xb, sb, tr = h.evolve(dev(x), max_iter=1, positions=pos)
    xw, sw, tw = R.evolve_ref(x, pos, lambda t: fn.forward_tokens(dev(t)).reshape(-1).cpu().numpy(), 1, "global")
    assert np.array_equal(xb.cpu().numpy(), xw) and sb.cpu().numpy().tobytes() == sw.tobytes() and tr["iters"] == tw["iters"] == 1


def _check_evolve(got, want):
    (xb, sb, tr), (xw, sw, tw) = got, want
    assert xb.dtype == torch.int64 and np.array_equal(xb.cpu().numpy(), xw)
    _same_bits(sb.cpu().numpy(), sw, "score_best")
    assert tr["iters"] == tw["iters"]
    for k in ("position", "allele", "taken", "score"):
        _same_bits(tr[k].cpu().numpy(), tw[k], k)


@pytest.mark.parametrize("stop", ["global", "row"])
@pytest.mark.parametrize("positions,max_iter", [(None, 4), ([3, 100, 101], 12)])
def test_evolve_equals_the_restatement_windowed_route(nets, stop, positions, max_iter):
    """L = 200, B = 3: x_best, score_best and the whole trace equal evolve_ref driven by forward_tokens scores, exactly. All
    positions for 4 iterations; three positions for up to 12, where rows run out of improving moves (stop = "row": dead rows, whose
    mutants the windowed route drops; stop = "global": the stalling iteration in the trace)."""
    model, emb, head, _ = nets["full"]
    x = _x(3, 200, 21)
    fn = model.value_callable(emb, head)
    assert model._ism_route(emb, head, None, 200)[1] is fn
    score = lambda t: fn.forward_tokens(dev(t)).reshape(-1).float().cpu().numpy()             # noqa: E731
    pos = list(range(200)) if positions is None else positions
    want = R.evolve_ref(x, pos, score, max_iter, stop)
    got = model.evolve(dev(x), emb, head, max_iter=max_iter, positions=positions, stop=stop)
    _check_evolve(got, want)
    print(f"evolve {stop} P={len(pos)}: iters {want[2]['iters']}, taken per iteration {want[2]['taken'].sum(1).tolist()}")
    if positions is not None:
        assert want[2]["iters"] < max_iter and want[2]["taken"][-1].sum() == 0                # it did stop on its own
        _check_evolve(model.evolve(dev(x), emb, head, max_iter=max_iter, positions=positions, stop=stop, chunk_rows=9), want)
    x0, s0, t0 = model.evolve(dev(x), emb, head, max_iter=0, stop=stop)
    assert np.array_equal(x0.cpu().numpy(), x) and t0["iters"] == 0 and t0["score"].shape == (1, 3) and t0["position"].shape == (0, 3)
    assert s0.cpu().numpy().tobytes() == score(x).tobytes()


@pytest.mark.parametrize("stop", ["global", "row"])
def test_evolve_equals_the_restatement_opaque_route(nets, stop):
    """The tiny 8-channel value net (PyTorch modules) at L = 50: the opaque fn(transform_samples(cand)) route, one chunk per
    iteration, against evolve_ref driven by the same call on the same batch."""
    from svdd_amd import ops
    model, emb, head = nets["tiny"]
    x = _x(3, 50, 5)
    fn = model.value_callable(emb, head)
    assert not hasattr(fn, "forward_tokens") and model._ism_route(emb, head, None, 50)[1] is None
    with torch.no_grad():
        score = lambda t: fn(ops.transform_samples(dev(t))).reshape(len(t), -1)[:, 0].float().cpu().numpy()   # noqa: E731
        want = R.evolve_ref(x, list(range(50)), score, 4, stop)
        _check_evolve(model.evolve(dev(x), emb, head, max_iter=4, stop=stop), want)
        ism = model.ism_scores(dev(x), emb, head)
        assert torch.equal(ism.cpu(), torch.from_numpy(R.ism_ref(x, list(range(50)), score)))


# ------------------------------------------------------------------------------------------------ the fixtures ----
def _fixture(g, model, emb, head):
    x, pos = g["x"], g["positions"].tolist()
    ism = model.ism_scores(dev(x), emb, head, positions=pos).cpu().numpy()
    assert ism.shape == g["ism"].shape
    own = ism[np.arange(len(x))[:, None], np.arange(len(pos))[None, :], x[:, pos]]
    err, perr = float(np.abs(ism - g["ism"]).max()), float(np.abs(own - g["parent"][:, None]).max())
    spread = float(np.abs(g["ism"] - g["parent"][:, None, None]).mean())
    return err, perr, spread


def test_recorded_reference_table_tiny_nets(nets):
    """g36: the reference's tiny value net on every mutant, one at a time, on the CPU; the engine's table (PyTorch modules on the
    device) within the soft-value bar."""
    model, emb, head = nets["tiny"]
    err, perr, spread = _fixture(load_golden("g36_ism_tiny.npz"), model, emb, head)
    print(f"ERR ism_g36 {err:.3e} (parents {perr:.3e}) bar {SOFT_BAR:.0e}; mean |mutant - parent| recorded {spread:.3e}")
    assert err <= SOFT_BAR and perr <= SOFT_BAR


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_recorded_reference_table_full_size_nets(nets, precision):
    """g37: the seed-44 full-size value net, L = 200, B = 2, all positions, through the windowed tower; same bar."""
    model, emb, head, _ = nets["plain"]
    g = load_golden("g37_ism_full.npz")
    for nm, mod in (("embedding", emb), ("head", head)):
        sums = np.array([float(p.double().sum()) for p in mod.state_dict().values()])
        assert np.allclose(sums, g[nm + "_param_sums"], rtol=0, atol=1e-6), nm
    with knobs(model, precision=precision):
        assert model._ism_route(emb, head, None, 200)[1] is not None
        err, perr, spread = _fixture(g, model, emb, head)
    print(f"ERR ism_g37 {precision} {err:.3e} (parents {perr:.3e}) bar {SOFT_BAR:.0e}; mean |mutant - parent| recorded {spread:.3e}")
    assert err <= SOFT_BAR and perr <= SOFT_BAR
