"""-m gpu: pattern scanning and pattern-driven directed evolution on the device.

  kernels   svdd_pattern_mutants, svdd_pattern_fold, svdd_pattern_apply against the host restatement tests/pattern_ref.py in
            sentinel-guarded buffers, exactly: word and byte paths, a second lane loop, patterns across word borders and across
            255 | 256, mixed widths, dead rows, bad tokens, ties across a chunk border, NaN, an all-NaN row, the compacted form, both
            stop modes, more rows than the workgroup has threads, launches after the stop
  engine    Diffusion.pattern_scores against forward_tokens on every mutant, bit for bit (windowed tower at L = 200 / 105 / 208,
            whole mutants at L = 50 / 104, fused and plain nets; fp32 and f16x3; one, two and all positions per chunk); Diffusion.evolve_patterns against
            evolve_patterns_ref driven by the same scores, exactly; motifs.consensus_patterns -> evolve_patterns -> scan_rows
  fixtures  g42 / g43: the reference's own nets on every mutant, one at a time, on the CPU (tests/golden/make_golden_pattern.py),
            within the project's soft-value bar of 1e-4
"""
import contextlib
import os

import numpy as np
import pytest
import torch

from tests import e2e_parity
from tests import pattern_ref as R
from tests.conftest import load_golden
from tests.kernel_harness import DEV, _Buf, _st

pytestmark = pytest.mark.gpu
SOFT_BAR = 1e-4                    # README: "soft values within 1e-4"
HERE = os.path.dirname(os.path.abspath(__file__))


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


def pack(patterns):
    """-> (u8 [K, 32] with a byte no pattern holds past each width, i32 [K]) on the device: the padding is never read."""
    pat = np.full((len(patterns), 32), 0xEE, np.uint8)
    for k, p in enumerate(patterns):
        pat[k, :len(p)] = p
    return dev(pat), dev(np.array([len(p) for p in patterns], np.int32))


# ------------------------------------------------------------------------------------------------ svdd_pattern_mutants ----
def _mutants(x, positions, patterns, live=None, want_onehot=True, misalign=0):
    """One svdd_pattern_mutants launch through the raw C entry, outputs in guarded sentinel buffers -> (cand, onehot | None, err)."""
    from svdd_amd import _lib
    B, L = x.shape
    P, K = len(positions), len(patterns)
    n = B * P * K
    raw = torch.zeros(x.size + 8, dtype=torch.uint8, device=DEV)
    raw[misalign:misalign + x.size] = dev(x.reshape(-1))
    pos = dev(np.asarray(positions, np.int32))
    pat, widths = pack(patterns)
    lv = None if live is None else dev(np.asarray(live, np.uint8))
    cand, oh, err = _Buf(n * L + 8, torch.uint8), (_Buf(n * L * 4) if want_onehot else None), torch.zeros(1, dtype=torch.int32, device=DEV)
    rc = _lib.lib().svdd_pattern_mutants(raw.data_ptr() + misalign, pos.data_ptr(), pat.data_ptr(), widths.data_ptr(),
                                         None if lv is None else lv.data_ptr(), B, L, P, K, cand.ptr + misalign,
                                         None if oh is None else oh.ptr, err.data_ptr(), _st())
    _lib.check(rc, "svdd_pattern_mutants")
    torch.cuda.synchronize()
    mask = torch.zeros(n * L + 8, dtype=torch.bool)
    mask[misalign:misalign + n * L] = True
    cand.assert_written_where("cand", mask)
    out = cand.cpu().numpy()[misalign:misalign + n * L].reshape(B, P * K, L)
    if oh is not None:
        oh.assert_written("onehot")
    return out, (None if oh is None else oh.cpu().numpy().reshape(n, L, 4)), int(err[0])


WIDTHS = (1, 3, 4, 5, 6, 32)       # 3 at start 3 lies in two words, 6 at start 3 in three, 32 at an odd start in nine


def _starts(L, w):
    """0, L - w, starts that put a pattern across a word border, and 254 (across 255 | 256) where they fit."""
    return sorted(p for p in {0, 1, 3, 7, 254, L - w} if 0 <= p and p + w <= L)


def _check_mutants(x, positions, patterns, live=None, want_err=0):
    want = R.mutants_ref(x, positions, patterns, live)
    L = x.shape[1]
    for kw in (dict(), dict(want_onehot=False), dict(misalign=1)):
        cand, oh, err = _mutants(x, positions, patterns, live, **kw)
        assert err == want_err and np.array_equal(cand, want), (kw, positions, [len(p) for p in patterns])
        if oh is not None:
            assert oh.tobytes() == R.onehot_ref(want).reshape(-1, L, 4).tobytes(), kw
    return want


@pytest.mark.parametrize("L", [1, 3, 4, 50, 200, 260])
def test_pattern_mutants_kernel_matches_the_restatement(L):
    """Tokens and one-hot exact, guards intact. L = 3 and 50 take the byte path, a misaligned base forces it at every L (the same
    result); L = 260 makes a lane loop a second time. Every width alone (K = 1) at 0, L - w and across word borders, then all
    widths that fit together (K = 5 at L >= 50: mixed widths, the pattern index running fastest); with and without the one-hot."""
    rng = np.random.default_rng(L)
    B = 3
    x = rng.integers(0, 4, (B, L)).astype(np.uint8)
    fit = [w for w in WIDTHS if w <= L]
    for w in fit:
        pat = [rng.integers(0, 4, w).astype(np.uint8)]
        pos = _starts(L, w)
        assert pos[0] == 0 and pos[-1] == L - w
        want = _check_mutants(x, pos, pat)
        assert ((want != x[:, None, :]).sum(-1) <= w).all()
    mixed = [rng.integers(0, 4, w).astype(np.uint8) for w in (fit if len(fit) < 5 else [1, 32, 5, 3, 6])]
    wmax = max(len(p) for p in mixed)
    want = _check_mutants(x, _starts(L, wmax), mixed)
    if L == 260:                                         # the widest pattern at 228 covers 255 | 256; 3 and 6 at 254 cross it as well
        assert _starts(L, wmax) == [0, 1, 3, 7, 228] and _starts(L, 3)[-2] == 254 and _starts(L, 6)[-1] == 254
    # a pattern that is already there gives an exact copy, and svdd_candidate_windows flags it 0
    if L >= 4:
        from svdd_amd import fused
        p0 = L // 2 - 1
        own = [x[1, p0:p0 + min(3, L)].copy(), rng.integers(0, 4, 1).astype(np.uint8)]
        want = _check_mutants(x, [0, p0], own)
        copies = (want == x[:, None]).all(-1).reshape(-1)
        assert copies[1 * 4 + 2] and not copies.all()
        flags = torch.empty(B * 4, dtype=torch.int32, device=DEV)
        fused.candidate_windows(dev(want), dev(x), flags=flags)
        assert np.array_equal(flags.cpu().numpy() == 0, copies)


@pytest.mark.parametrize("L", [7, 200, 260])
def test_pattern_mutants_dead_rows_bad_tokens_and_windows_that_leave_the_row(L):
    rng = np.random.default_rng(L + 1)
    x = rng.integers(0, 4, (3, L)).astype(np.uint8)
    pats = [rng.integers(0, 4, w).astype(np.uint8) for w in (1, 5, 3)]
    pos = _starts(L, 5)
    want = _check_mutants(x, pos, pats, live=[1, 0, 1])
    assert (want[1] == x[1]).all() and (want[0] != x[0]).any()
    # a MASK token anywhere in a parent (here: far from every window): err, and every mutant of THAT row is an exact copy
    xb = x.copy()
    xb[2, L - 1] = 4
    want = _check_mutants(xb, pos[:2], pats, want_err=1)
    assert (want[2] == xb[2]).all() and (want[2, :, L - 1] == 4).all() and (want[0] != xb[0]).any()
    # a window that leaves the row (the widest pattern at L - 3), a negative start: err, copies, nothing out of bounds
    want = _check_mutants(x, [0, L - 3], pats, want_err=1)
    assert (want[:, 3 + 1] == x).all() and (want[:, 3 + 2] != x).any()
    want = _check_mutants(x, [-2, 0], pats, want_err=1)
    assert (want[:, :3] == x[:, None]).all()
    # a pattern token 4: err, copies for that pattern alone
    bad = [pats[0], np.array([0, 4, 1], np.uint8)]
    want = _check_mutants(x, pos, bad, want_err=1)
    assert (want[:, 1::2] == x[:, None]).all() and (want[:, 0::2] != x[:, None]).any()


def test_ops_pattern_mutants_and_refusals():
    from svdd_amd import ops
    x = np.random.default_rng(3).integers(0, 4, (2, 12)).astype(np.uint8)
    pats = [np.array([1, 2, 3, 0, 1], np.uint8), np.array([2], np.uint8)]
    pos = torch.tensor([0, 5, 7], dtype=torch.int32, device=DEV)
    pat, widths = pack(pats)
    cand, oh = ops.pattern_mutants(dev(x), pos, pat, widths)
    assert np.array_equal(cand.cpu().numpy(), R.mutants_ref(x, [0, 5, 7], pats)) and oh.shape == (12, 12, 4)
    xb = x.copy()
    xb[0, 11] = 4
    with pytest.raises(ops.SvddError, match="token > 3"):
        ops.pattern_mutants(dev(xb), pos, pat, widths)
    bad, _ = pack([np.array([1, 4, 3, 0, 1], np.uint8), np.array([2], np.uint8)])              # a pattern token 4 forced through ops
    with pytest.raises(ops.SvddError, match="token > 3"):
        ops.pattern_mutants(dev(x), pos, bad, widths)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    cand, _ = ops.pattern_mutants(dev(x), pos, bad, widths, want_onehot=False, err=err)
    assert int(err[0]) == 1 and (cand.cpu().numpy()[:, 0::2] == x[:, None]).all() and (cand.cpu().numpy()[:, 1::2] != x[:, None]).any()
    with pytest.raises(ops.SvddError, match="outside"):
        ops.pattern_mutants(dev(x), torch.tensor([0, 8], dtype=torch.int32, device=DEV), pat, widths)   # 8 + 5 > 12: flagged on the device
    for f in (lambda: ops.pattern_mutants(torch.from_numpy(x), pos, pat, widths), lambda: ops.pattern_mutants(dev(x), pos.cpu(), pat, widths),
              lambda: ops.pattern_mutants(dev(x), pos, pat[:, :16].contiguous(), widths), lambda: ops.pattern_mutants(dev(x), pos, pat, widths.long()),
              lambda: ops.pattern_mutants(dev(x), pos, pat, widths, cand=torch.empty((2, 6, 11), dtype=torch.uint8, device=DEV))):
        with pytest.raises(ops.SvddError):
            f()


# ------------------------------------------------------------------------------------------------ svdd_pattern_fold ----
def _fold_scores(B, P, K, chunk, rng):
    """[B, P K]: small integers (many exact ties). Row 0: the maximum planted on both sides of the first chunk border (the earlier
    one must win) and a NaN in what would be the winning place in front of them; row 1 all NaN; row 2 all -inf; row 3: NaN at
    both ends, +inf twice."""
    s = rng.integers(-3, 4, (B, P * K)).astype(np.float32)
    border = min(chunk, P - 1) * K
    s[0, [max(border - 1, 0), border]] = 7.0
    s[0, 0] = np.nan if border > 1 else s[0, 0]
    if B > 1:
        s[1] = np.nan
    if B > 2:
        s[2] = -np.inf
    if B > 3:
        s[3, [0, -1]] = np.nan
        s[3, [P * K // 2, P * K - 2]] = np.inf
    return s


def _fold(s, ps, P, K, chunk, live=None, with_table=True, with_best=True, slot_route=False):
    from svdd_amd import _lib
    B = len(ps)
    psd = dev(ps)
    lv = None if live is None else dev(np.asarray(live, np.uint8))
    table = _Buf(B * P * K) if with_table else None
    bs, bp, bk = (_Buf(B), _Buf(B, torch.int32), _Buf(B, torch.int32)) if with_best else (None, None, None)
    ptr = lambda b: None if b is None else b.ptr                                           # noqa: E731
    for p0 in range(0, P, chunk):
        pc = min(chunk, P - p0)
        sc = np.ascontiguousarray(s[:, K * p0:K * (p0 + pc)])
        slot = None
        if slot_route:                                   # the compacted form: every third entry is a copy (slot -1), the rest shuffled
            keep = np.flatnonzero(np.arange(B * pc * K) % 3 != 1)
            order = np.random.default_rng(p0).permutation(len(keep))
            slot_np = np.full(B * pc * K, -1, np.int32)
            slot_np[keep[order]] = np.arange(len(keep), dtype=np.int32)
            sc = np.concatenate([sc.reshape(-1)[keep[order]], np.full(3, 777.0, np.float32)])  # rows past the count: never read
            slot = dev(slot_np)
        scd = dev(sc)
        rc = _lib.lib().svdd_pattern_fold(scd.data_ptr(), None if slot is None else slot.data_ptr(), psd.data_ptr(),
                                          None if lv is None else lv.data_ptr(), B, P, K, p0, pc, ptr(table), ptr(bs), ptr(bp), ptr(bk), _st())
        _lib.check(rc, "svdd_pattern_fold")
    torch.cuda.synchronize()
    for b in (table, bs, bp, bk):
        if b is not None:
            b.assert_written("fold output")
    return (None if table is None else table.cpu().numpy().reshape(B, P, K),
            None if bs is None else (bs.cpu().numpy(), bp.cpu().numpy(), bk.cpu().numpy()))


def _fold_want(s, ps, P, K, live):
    """fold_ref in one chunk."""
    table, best = np.empty((len(ps), P, K), np.float32), R.new_best(len(ps))
    R.fold_ref(s, ps, K, 0, P, table, best, live)
    return table, best


@pytest.mark.parametrize("K", [1, 5])
@pytest.mark.parametrize("P", [1, 64, 65, 130])
def test_pattern_fold_kernel_matches_the_restatement_in_every_chunking(P, K):
    """The table and the running best against fold_ref, exactly: the first (position, pattern) wins a tie, the running best of the
    earlier chunks wins a tie across the chunk border, a NaN and -inf never win, the all-NaN row keeps (-inf, -1, -1). One chunk,
    two chunks and chunks of 7 positions give identical bits (P K > 64: lanes loop); the compacted (slot) form with -1 entries;
    a dead row; either output alone."""
    rng = np.random.default_rng(P * 10 + K)
    B = 6
    half = (P + 1) // 2
    s, ps = _fold_scores(B, P, K, half, rng), rng.integers(-2, 9, B).astype(np.float32)
    ps[5] = 9.0                                          # above every finite score: in the slot form row 5's first copy wins
    for live in (None, [b % 3 != 1 for b in range(B)]):
        want_t, want_b = _fold_want(s, ps, P, K, live)
        if live is None:
            assert want_b[1][1] == -1 and want_b[2][1] == -1 and want_b[0][2] == -np.inf and want_b[1][2] == -1
            if P > 1:
                assert want_b[0][0] == 7.0 and want_b[1][0] * K + want_b[2][0] == min(half, P - 1) * K - 1   # the earlier of the two
        for chunk in sorted({P, half, min(P, 7)}):
            table, best = _fold(s, ps, P, K, chunk, live)
            _same_bits(table, want_t, ("table", chunk))
            for g, w, nm in zip(best, want_b, ("best_score", "best_pos", "best_pattern")):
                _same_bits(g, w, (nm, chunk, live))
            # the compacted form: the copies' entries are the parent's score (the reference folds the dense scores with them put in)
            sd = s.copy()
            for p0 in range(0, P, chunk):
                pc = min(chunk, P - p0)
                local = (np.arange(B * pc * K) % 3 == 1).reshape(B, pc * K)
                blk = sd[:, K * p0:K * (p0 + pc)]
                blk[local] = np.broadcast_to(ps[:, None], blk.shape)[local]
            wt, wb = _fold_want(sd, ps, P, K, live)
            table, best = _fold(s, ps, P, K, chunk, live, slot_route=True)
            _same_bits(table, wt, ("table", chunk, "slot"))
            for g, w, nm in zip(best, wb, ("best_score", "best_pos", "best_pattern")):
                _same_bits(g, w, (nm, chunk, "slot", live))
            if live is None and P * K > 3:
                assert wb[0][5] == 9.0                   # a copy's score (the parent's) is a legitimate winner
        table, best = _fold(s, ps, P, K, half, live, with_best=False)
        assert best is None
        _same_bits(table, want_t, "table alone")
        table, best = _fold(s, ps, P, K, half, live, with_table=False)
        assert table is None and all(_bits(g).tobytes() == _bits(w).tobytes() for g, w in zip(best, want_b))


# ------------------------------------------------------------------------------------------------ svdd_pattern_apply ----
class _State:
    """The in-place state of svdd_pattern_apply in guarded buffers, mirrored by numpy arrays that apply_ref updates."""

    def __init__(self, x, score, stop, positions, patterns):
        B, L = x.shape
        self.B, self.L, self.stop, self.positions, self.patterns = B, L, stop, positions, patterns
        self.pos_dev = dev(np.asarray(positions, np.int32))
        self.pat_dev, self.widths_dev = pack(patterns)
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
        bs, bp, bk = (dev(a) for a in best)
        tr = (_Buf(B, torch.int32), _Buf(B, torch.int32), _Buf(B), _Buf(B, torch.uint8))
        b = self.buf
        rc = _lib.lib().svdd_pattern_apply(bs.data_ptr(), bp.data_ptr(), bk.data_ptr(), self.pos_dev.data_ptr(), self.pat_dev.data_ptr(),
                                           self.widths_dev.data_ptr(), B, self.L, len(self.positions), len(self.patterns),
                                           {"global": 0, "row": 1}[self.stop], b["x"].ptr, b["cur"].ptr,
                                           b["live"].ptr if self.stop == "row" else None, b["bsf"].ptr, b["stopped"].ptr, b["x_best"].ptr,
                                           b["score_best"].ptr, *[t.ptr for t in tr], _st())
        _lib.check(rc, "svdd_pattern_apply")
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
@pytest.mark.parametrize("B,L", [(1, 9), (17, 37), (1025, 12), (3, 264)])
def test_pattern_apply_kernel_matches_one_step_of_the_restatement(B, L, stop):
    """Iterations of synthetic picks (ties with the row's score, NaN, +-inf, rows without a pick, picks that do not fit, picks of
    5 and 6 bytes across one and two word borders, at 0 and at L - w) through the kernel and apply_ref: every state buffer and
    the trace equal after every launch; x_best keeps the first occurrence of a row's maximum; a launch after `stopped` is set
    changes nothing (all buffers compared before and after, trace buffers untouched). B = 1025: a thread strides over rows;
    L = 37 and 9: the byte path; L = 264: a lane loops."""
    rng = np.random.default_rng(B * 10 + L + (stop == "row"))
    x = rng.integers(0, 4, (B, L)).astype(np.uint8)
    score = rng.integers(-2, 3, B).astype(np.float32)
    patterns = [rng.integers(0, 4, w).astype(np.uint8) for w in (5, 1, 6, 3)]
    positions = sorted({0, 1, 3, L - 6, L - 5, L - 3, L - 1} - {-1, -2})       # the last starts fit only the shorter patterns
    P, K = len(positions), len(patterns)
    st = _State(x, score, stop, positions, patterns)
    stopped_at = None
    for it in range(12):
        rising = it < 4                                  # the first iterations keep the batch maximum rising; from the 7th on no
        hi = 3 if rising else 2 if it < 6 else 1         # pick beats its row's score (ties and losses only): both modes stop there
        bs = (st.np["cur"] + rng.integers(-1, hi, B)).astype(np.float32)
        bp = rng.integers(0, P, B).astype(np.int32)
        bk = rng.integers(0, K, B).astype(np.int32)
        bp[0], bk[0] = ((0, 2), (positions.index(L - 6), 2), (2, 0), (positions.index(L - 5), 0))[it % 4]    # 6 at 0 / L - 6, 5 at 3 / L - 5
        if rising:
            bs[0 if B < 5 else rng.integers(5, B)] = st.state["best_so_far"] + 1
        if B > 4:
            bs[1], bs[2] = np.nan, -np.inf
            bp[3], bk[3], bs[3] = -1, -1, -np.inf        # a row without a pick
            bp[4], bk[4] = P - 1, 2                      # 6 bytes at L - 1: the pick does not fit, it is not valid
        best = (bs, bp, bk)
        before = st.snapshot()
        tr = st.launch(best)
        want = R.apply_ref(best, positions, patterns, stop, st.np["x"], st.np["cur"], st.np["live"], st.state, st.np["x_best"],
                           st.np["score_best"])
        if want is None:                                 # already stopped: nothing is written, not even the trace
            after = st.snapshot()
            assert all(np.array_equal(before[k], after[k]) for k in before), it
            for t in tr:
                t.assert_untouched("trace after the stop")
            continue
        for t, w, nm in zip(tr, want, ("position", "pattern", "score", "taken")):
            t.assert_written(nm)
            _same_bits(t.cpu().numpy(), w, (it, nm))
        st.check(it)
        if B > 4 and it == 0:
            assert want[0][4] == -1 and want[3][4] == 0 and want[3].sum() > 0
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
    """"full": the full-size seeded nets with every convolution and norm of the value net re-drawn (net_ref.distinct_layers: no two
    layers of a tower equal); "plain": the seed-44 nets of g43 as they are; "tiny": the reference's 8-channel value net (PyTorch
    modules: the whole-mutant route)."""
    from svdd_amd import synthetic
    from tests.net_ref import distinct_layers
    full = synthetic.build("dna", DEV)
    distinct_layers(full[1], seed=1)
    return {"full": full, "plain": synthetic.build("dna", DEV), "tiny": e2e_parity.tiny_engine(load_golden("nets_tiny.npz"), 50, 8, DEV)}


def _x(B, L, seed):
    return np.random.default_rng(seed).integers(0, 4, (B, L)).astype(np.uint8)


def _brute_table(score, x, pos, patterns):
    """[B, P, K] from `score` on EVERY mutant's tokens, the copies included, and the parents' scores."""
    B, L = x.shape
    m = R.mutants_ref(x, pos, patterns)
    return score(m.reshape(-1, L)).reshape(B, len(pos), len(patterns)), score(x)


def _case(L, seed):
    """B = 2; patterns of widths 1, 7 and 32, the last a slice of row 0 (at its second position: that mutant is a copy);
    positions with 0 and L - 32 among them."""
    x = _x(2, L, seed)
    rng = np.random.default_rng(seed + 1)
    pos = sorted({0, 5, 16, 33, L // 2, L - 40, L - 32})
    patterns = [rng.integers(0, 4, 1).astype(np.uint8), rng.integers(0, 4, 7).astype(np.uint8), x[0, pos[1]:pos[1] + 32].copy()]
    return x, pos, patterns


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
@pytest.mark.parametrize("L", [200, 105, 208])
def test_pattern_scores_equal_forward_tokens_bit_for_bit_windowed(nets, L, precision):
    """Every entry is fn.forward_tokens on that mutant's tokens in the same precision, bit for bit (torch.equal) — the copy's entry
    too, which the engine does not compute; Pc = 1, Pc = 2 and all positions per chunk give the same bits. L = 105 and 208 are
    the ends of the windowed range."""
    from svdd_amd.fused import FusedValueNet
    model, emb, head, _ = nets["full"]
    x, pos, patterns = _case(L, L)
    with knobs(model, precision=precision):
        fn = model.value_callable(emb, head)
        assert isinstance(fn, FusedValueNet) and fn.precision == precision and model._ism_route(emb, head, None, L)[1] is fn
        score = lambda t: fn.forward_tokens(dev(t)).reshape(len(t), -1)[:, 0].float().cpu().numpy()      # noqa: E731
        table = model.pattern_scores(dev(x), patterns, emb, head, positions=pos)
        want, parent = _brute_table(score, x, pos, patterns)
        one = model.pattern_scores(dev(x).long(), [p.tolist() for p in patterns], emb, head, positions=pos, chunk_rows=6)
        two = model.pattern_scores(dev(x), patterns, emb, head, positions=torch.tensor(pos), chunk_rows=12)
        sub = model.pattern_scores(dev(x), patterns, emb, head, positions=pos[:2], compare="subtract")
        # one and two candidates per parent and pass (K = 1 / K = 2 with one position per chunk): the windowed tower at M = 1 and M = 2
        m1 = model.pattern_scores(dev(x), patterns[1:2], emb, head, positions=pos, chunk_rows=2)
        m2 = model.pattern_scores(dev(x), patterns[1:], emb, head, positions=pos, chunk_rows=4)
    assert torch.equal(m1, table[:, :, 1:2]) and torch.equal(m2, table[:, :, 1:])
    assert table.dtype == torch.float32 and table.shape == (2, len(pos), 3) and not torch.isnan(table).any()
    assert torch.equal(table.cpu(), torch.from_numpy(want))
    assert table.cpu().numpy()[0, 1, 2].tobytes() == parent[0].tobytes()                      # the copy: the parent's score, same bits
    assert torch.equal(one, table) and torch.equal(two, table)
    assert float((table.cpu() != torch.from_numpy(parent)[:, None, None]).float().mean()) > 0.9
    assert torch.equal(sub, table[:, :2] - torch.from_numpy(parent).to(DEV)[:, None, None])


def test_pattern_scores_whole_mutant_route_and_strings(nets):
    """The tiny 8-channel value net (PyTorch modules) at L = 50: the fn(transform_samples(cand)) route against the same call on the
    same batches of mutants, exactly: all positions in one chunk, Pc = 1, Pc = 2 with a ragged last chunk (5 positions), and all
    42 starts in chunks of 4 (ragged); the copy's entry is the parent's score from the parents' own batch. Patterns given as strings
    are the same patterns."""
    from svdd_amd import ops
    model, emb, head = nets["tiny"]
    x = _x(3, 50, 5)
    pos = [0, 3, 17, 30, 41]
    patterns = [np.array([2], np.uint8), np.array([1, 0, 3, 3], np.uint8), x[1, 17:26].copy()]
    fn = model.value_callable(emb, head)
    assert not hasattr(fn, "forward_tokens") and model._ism_route(emb, head, None, 50)[1] is None
    with torch.no_grad():
        score = lambda t: fn(ops.transform_samples(dev(t))).reshape(len(t), -1)[:, 0].float().cpu().numpy()   # noqa: E731
        want, parent = _brute_table(score, x, pos, patterns)
        want[1, 2, 2] = parent[1]                        # the copy: the engine's entry is the parent's, from the parents' batch
        table = model.pattern_scores(dev(x), patterns, emb, head, positions=pos)
        assert torch.equal(table.cpu(), torch.from_numpy(want))
        as_text = ["".join("ACGT"[t] for t in p) for p in patterns]
        assert torch.equal(model.pattern_scores(dev(x), as_text, emb, head, positions=pos), table)
        assert torch.equal(table.cpu(), torch.from_numpy(R.table_ref(x, pos, patterns, score, whole_batch=True)))
        for chunk_rows, pc in ((9, 1), (18, 2), (26, 2)):                                  # B K = 9 rows per position
            got = model.pattern_scores(dev(x), patterns, emb, head, positions=pos, chunk_rows=chunk_rows)
            assert torch.equal(got.cpu(), torch.from_numpy(R.table_ref(x, pos, patterns, score, whole_batch=True, chunk=pc))), chunk_rows
            assert got[1, 2, 2].cpu().numpy().tobytes() == parent[1].tobytes()            # the copy, in a chunk with p0 > 0
        every = list(range(50 - 9 + 1))                                                    # positions None: 0 .. L - w_max
        full = model.pattern_scores(dev(x), patterns, emb, head)
        assert full.shape == (3, 42, 3) and torch.equal(full.cpu(), torch.from_numpy(R.table_ref(x, every, patterns, score, whole_batch=True)))
        full4 = model.pattern_scores(dev(x), patterns, emb, head, chunk_rows=36)           # 10 chunks of 4 positions and one of 2
        assert torch.equal(full4.cpu(), torch.from_numpy(R.table_ref(x, every, patterns, score, whole_batch=True, chunk=4)))


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
@pytest.mark.parametrize("L", [50, 104])
def test_pattern_scores_forward_tokens_route_in_every_chunking(nets, L, precision):
    """The fused net at L <= 104 takes the whole-mutant route through forward_tokens, whose bits do not depend on the batch: the
    table equals forward_tokens on every mutant bit for bit, and Pc = 1, Pc = 2 (ragged: 7 positions) and one chunk give the
    same bits; evolve_patterns with one position per chunk equals evolve_patterns_ref exactly."""
    from svdd_amd.fused import FusedValueNet
    model, emb, head, _ = nets["full"]
    x = _x(2, L, L + 3)
    rng = np.random.default_rng(L + 4)
    pos = sorted({0, 2, 5, 11, L - 40, L - 33, L - 32})                    # starts in 0 .. L - 32
    patterns = [rng.integers(0, 4, 1).astype(np.uint8), rng.integers(0, 4, 7).astype(np.uint8), x[0, pos[1]:pos[1] + 32].copy()]
    assert len(pos) == 7
    with knobs(model, precision=precision):
        fn = model.value_callable(emb, head)
        assert isinstance(fn, FusedValueNet) and model._ism_route(emb, head, None, L)[1] is None
        score = lambda t: fn.forward_tokens(dev(t)).reshape(len(t), -1)[:, 0].float().cpu().numpy()      # noqa: E731
        table = model.pattern_scores(dev(x), patterns, emb, head, positions=pos)
        want, parent = _brute_table(score, x, pos, patterns)
        one = model.pattern_scores(dev(x), patterns, emb, head, positions=pos, chunk_rows=6)
        two = model.pattern_scores(dev(x), patterns, emb, head, positions=pos, chunk_rows=12)
        short = [p[:6] for p in patterns]
        ev_want = R.evolve_patterns_ref(score, x, short, pos[::2], 3, "row")
        ev_one = model.evolve_patterns(dev(x), short, emb, head, max_iter=3, positions=pos[::2], stop="row", chunk_rows=6)
        ev_two = model.evolve_patterns(dev(x), short, emb, head, max_iter=3, positions=pos[::2], stop="global", chunk_rows=12)
        ev_want_two = R.evolve_patterns_ref(score, x, short, pos[::2], 3, "global")
    assert torch.equal(table.cpu(), torch.from_numpy(want)) and table.cpu().numpy()[0, 1, 2].tobytes() == parent[0].tobytes()
    assert torch.equal(one, table) and torch.equal(two, table)
    _check_evolve(ev_one, ev_want)
    _check_evolve(ev_two, ev_want_two)
    assert ev_want[2]["taken"][0].any()


def _check_evolve(got, want):
    (xb, sb, tr), (xw, sw, tw) = got, want
    assert xb.dtype == torch.int64 and np.array_equal(xb.cpu().numpy(), xw)
    _same_bits(sb.cpu().numpy(), sw, "score_best")
    assert tr["iters"] == tw["iters"]
    for k in ("position", "pattern", "taken", "score"):
        _same_bits(tr[k].cpu().numpy(), tw[k], k)


def _noop_picks(x, patterns, trace):
    """Replays the trace on the host -> the (iteration, row) pairs whose pick was a pattern already in place."""
    x = x.copy()
    out = []
    for it in range(trace["iters"]):
        for b in range(len(x)):
            p, k = int(trace["position"][it, b]), int(trace["pattern"][it, b])
            if p < 0:
                continue
            if np.array_equal(x[b, p:p + len(patterns[k])], patterns[k]):
                out.append((it, b))
            if trace["taken"][it, b]:
                x[b, p:p + len(patterns[k])] = patterns[k]
    return out


@pytest.mark.parametrize("stop", ["global", "row"])
def test_evolve_patterns_equals_the_restatement_windowed_route(nets, stop):
    """L = 200, B = 3, three patterns at four starts: x_best, score_best and the whole trace equal evolve_patterns_ref driven by
    forward_tokens scores, exactly; three iterations or more, among them a pick that is a no-op (a pattern already in place: not
    computed, the row's own score). One position per chunk gives the same run. max_iter = 0 returns the input."""
    model, emb, head, _ = nets["full"]
    x = _x(3, 200, 25)                                   # "global": four iterations, row 0's third pick a no-op that is taken
    rng = np.random.default_rng(26)
    patterns = [rng.integers(0, 4, w).astype(np.uint8) for w in (6, 11, 20)]
    pos = [10, 60, 110, 160]
    fn = model.value_callable(emb, head)
    assert model._ism_route(emb, head, None, 200)[1] is fn
    score = lambda t: fn.forward_tokens(dev(t)).reshape(-1).float().cpu().numpy()             # noqa: E731
    want = R.evolve_patterns_ref(score, x, patterns, pos, 8, stop)
    got = model.evolve_patterns(dev(x), patterns, emb, head, max_iter=8, positions=pos, stop=stop)
    noop = _noop_picks(x, patterns, want[2])
    print(f"evolve_patterns {stop}: iters {want[2]['iters']}, taken per iteration {want[2]['taken'].sum(1).tolist()}, no-op picks {noop}")
    _check_evolve(got, want)
    assert want[2]["iters"] >= 3 and noop, "the case must run three iterations and meet a no-op pick"
    _check_evolve(model.evolve_patterns(dev(x), patterns, emb, head, max_iter=8, positions=pos, stop=stop, chunk_rows=9), want)
    x0, s0, t0 = model.evolve_patterns(dev(x), patterns, emb, head, max_iter=0, stop=stop)
    assert np.array_equal(x0.cpu().numpy(), x) and t0["iters"] == 0 and t0["score"].shape == (1, 3) and t0["pattern"].shape == (0, 3)
    assert s0.cpu().numpy().tobytes() == score(x).tobytes()


@pytest.mark.parametrize("stop", ["global", "row"])
def test_evolve_patterns_whole_mutant_route(nets, stop):
    """The tiny value net at L = 50 against evolve_patterns_ref around the same call on the same batches (whole_batch: the copies
    go through the net with the rest and their answers are dropped, as in the engine): one chunk per iteration, one position per
    chunk, and three positions per chunk with a ragged last one."""
    from svdd_amd import ops
    model, emb, head = nets["tiny"]
    x = _x(3, 50, 7)
    rng = np.random.default_rng(8)
    patterns = [rng.integers(0, 4, w).astype(np.uint8) for w in (2, 5, 9)]
    pos = [0, 12, 25, 41]
    fn = model.value_callable(emb, head)
    with torch.no_grad():
        score = lambda t: fn(ops.transform_samples(dev(t))).reshape(len(t), -1)[:, 0].float().cpu().numpy()   # noqa: E731
        want = R.evolve_patterns_ref(score, x, patterns, pos, 5, stop, whole_batch=True)
        _check_evolve(model.evolve_patterns(dev(x), patterns, emb, head, max_iter=5, positions=pos, stop=stop), want)
        assert want[2]["iters"] >= 1 and want[2]["taken"][0].any()
        for chunk_rows, pc in ((9, 1), (27, 3)):                                           # B K = 9 rows per position, 4 positions
            want = R.evolve_patterns_ref(score, x, patterns, pos, 5, stop, whole_batch=True, chunk=pc)
            _check_evolve(model.evolve_patterns(dev(x), patterns, emb, head, max_iter=5, positions=pos, stop=stop, chunk_rows=chunk_rows), want)


def test_harness_entries_and_the_reward_layout(nets):
    """reward_model given: the [n, 4, L]-layout reward net (fused: the windowed route) scores; BaseModel.pattern_scan and
    evolve_patterns are those calls."""
    from svdd_amd.fused import FusedValueNet
    from svdd_amd.harness import BaseModel
    model, emb, head, reward = nets["full"]
    x, pos, patterns = _case(200, 9)
    fn = model.reward_callable(reward)
    assert isinstance(fn, FusedValueNet)
    score = lambda t: fn.forward_tokens(dev(t)).reshape(len(t), -1)[:, 0].float().cpu().numpy()          # noqa: E731
    table = model.pattern_scores(dev(x), patterns, emb, head, reward_model=reward, positions=pos)
    assert torch.equal(table.cpu(), torch.from_numpy(_brute_table(score, x, pos, patterns)[0]))
    assert not torch.equal(table, model.pattern_scores(dev(x), patterns, emb, head, positions=pos))      # the value net is another net
    h = BaseModel(emb, head, model, reward, 2)
    assert torch.equal(h.pattern_scan(dev(x), patterns, positions=pos), table)
    xb, sb, tr = h.evolve_patterns(dev(x), patterns, max_iter=2, positions=pos, stop="row")
    xw, sw, tw = R.evolve_patterns_ref(score, x, patterns, pos, 2, "row")
    assert np.array_equal(xb.cpu().numpy(), xw) and sb.cpu().numpy().tobytes() == sw.tobytes() and tr["iters"] == tw["iters"]


def test_consensus_patterns_evolve_and_the_motif_scan_agree(nets):
    """motifs.consensus_patterns -> evolve_patterns -> motifs.scan_rows: a row that took a pick has that motif's best window at
    the trace's start position with the motif's maximal score (checked for every motif `reachable` marks true)."""
    from svdd_amd import motifs
    model, emb, head, _ = nets["full"]
    mset = motifs.load_meme(os.path.join(HERE, "golden", "motifs_tiny.meme"))
    patterns = motifs.consensus_patterns(mset)
    x = _x(4, 200, 31)
    xb, sb, tr = model.evolve_patterns(dev(x), patterns, emb, head, max_iter=1, stop="row")
    assert tr["iters"] == 1
    _, best_score, best_start, _ = motifs.scan_rows(xb, mset)
    checked = 0
    for b in range(4):
        if not int(tr["taken"][0, b]):
            assert np.array_equal(xb[b].cpu().numpy(), x[b])
            continue
        p, k = int(tr["position"][0, b]), int(tr["pattern"][0, b])
        assert np.array_equal(xb[b, p:p + len(patterns[k])].cpu().numpy(), patterns[k]) and float(sb[b]) == float(tr["score"][1, b])
        if not mset.reachable[k]:
            continue
        assert int(best_score[b, k]) == int(mset.max_score[k]) and int(best_start[b, k]) == p, (b, k, p)
        checked += 1
    print(f"consensus -> evolve -> scan: picks {tr['pattern'][0].tolist()} at {tr['position'][0].tolist()}, {checked} rows checked")
    assert checked > 0


# ------------------------------------------------------------------------------------------------ the fixtures ----
def _fixture(g, model, emb, head):
    x, pos = g["x"], g["positions"].tolist()
    patterns = [g["patterns"][k, :w] for k, w in enumerate(g["widths"].tolist())]
    table = model.pattern_scores(dev(x), patterns, emb, head, positions=pos).cpu().numpy()
    assert table.shape == g["table"].shape
    parent = table[0, int(g["copy_at"]), -1]                                                   # the copy: row 0's own score
    err, perr = float(np.abs(table - g["table"]).max()), float(abs(parent - g["parent"][0]))
    spread = float(np.abs(g["table"] - g["parent"][:, None, None]).mean())
    return err, perr, spread


def test_recorded_reference_table_tiny_nets(nets):
    """g42: the reference's tiny value net on every mutant, one at a time, on the CPU; the engine's table (PyTorch modules on the
    device) within the soft-value bar."""
    model, emb, head = nets["tiny"]
    err, perr, spread = _fixture(load_golden("g42_pattern_tiny.npz"), model, emb, head)
    print(f"ERR pattern_g42 {err:.3e} (parent {perr:.3e}) bar {SOFT_BAR:.0e}; mean |mutant - parent| recorded {spread:.3e}")
    assert err <= SOFT_BAR and perr <= SOFT_BAR


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_recorded_reference_table_full_size_nets(nets, precision):
    """g43: the seed-44 full-size value net, L = 200, B = 2, 24 starts, three patterns, through the windowed tower; same bar."""
    model, emb, head, _ = nets["plain"]
    g = load_golden("g43_pattern_full.npz")
    for nm, mod in (("embedding", emb), ("head", head)):
        sums = np.array([float(p.double().sum()) for p in mod.state_dict().values()])
        assert np.allclose(sums, g[nm + "_param_sums"], rtol=0, atol=1e-6), nm
    with knobs(model, precision=precision):
        assert model._ism_route(emb, head, None, 200)[1] is not None
        err, perr, spread = _fixture(g, model, emb, head)
    print(f"ERR pattern_g43 {precision} {err:.3e} (parent {perr:.3e}) bar {SOFT_BAR:.0e}; mean |mutant - parent| recorded {spread:.3e}")
    assert err <= SOFT_BAR and perr <= SOFT_BAR


@pytest.mark.parametrize("net, precision, L, ism_rows, pattern_rows", [
    ("full", "f32", 105, 360, 389), ("full", "f16x3", 105, 360, 389),        # the shortest windowed length
    ("full", "f32", 33, 130, 125), ("full", "f16x3", 33, 130, 125),          # the fused net's forward_tokens route
    ("tiny", "f32", 33, 130, 125)])                                           # PyTorch modules: the opaque callable
def test_width_one_patterns_equal_ism_bit_for_bit(nets, net, precision, L, ism_rows, pattern_rows):
    """The two kinds meet in one driver: the four width-1 patterns A, C, G, T at every position are ism_scores' table [B, L, 4],
    bit for bit, on every route (both sides are pinned to forward_tokens / the opaque call by the tests above: no tolerance). The
    pattern whose base is already there is a copy that the pattern side does not compute; the ISM side has no copies. Each call
    runs in at least two chunks with a ragged last one, of different sizes for the two calls (B = 3: 9 and 12 rows per position)."""
    from svdd_amd.fused import FusedValueNet
    model, emb, head = nets[net][:3]
    x = _x(3, L, L + 7)
    chunks = [rows // per for rows, per in ((ism_rows, 9), (pattern_rows, 12))]
    assert chunks[0] != chunks[1] and all(pc < L and L % pc for pc in chunks)
    with knobs(model, precision=precision), torch.no_grad():
        fn = model.value_callable(emb, head)
        if net == "tiny":
            assert not hasattr(fn, "forward_tokens") and model._ism_route(emb, head, None, L)[1] is None
        else:
            assert isinstance(fn, FusedValueNet) and fn.precision == precision
            assert (model._ism_route(emb, head, None, L)[1] is fn) == (L > 104)
        ism = model.ism_scores(dev(x), emb, head, chunk_rows=ism_rows)
        table = model.pattern_scores(dev(x), ["A", "C", "G", "T"], emb, head, positions=None, chunk_rows=pattern_rows)
    assert ism.shape == table.shape == (3, L, 4) and not torch.isnan(ism).any()
    assert torch.equal(table, ism)
