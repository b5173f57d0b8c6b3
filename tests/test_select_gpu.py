"""-m gpu: diverse library selection. Everything here is an exact integer and must EQUAL tests/select_ref.py.

  svdd_within       through the raw C entry in sentinel-guarded buffers (tests/kernel_harness.py), each output once NULL and once
                    given: every word edge of the row with dirty padding bits, tile / workgroup / segment edges on both sides,
                    radius 0, 1 and L - 1, one and both strands, every kind of device count, seeded `first`
  svdd_greedy_pick  on RANDOM bit matrices and `first` vectors (not derived from distances): word and lane edges of the settled
                    set, a count that starts above 0, k reached before / inside / never, cap reached exactly
  public            quality.select_diverse on the shared case table for every block_rows, library_quality,
                    BaseModel.select_library and --select
"""
import functools
import math

import numpy as np
import pytest
import torch

from svdd_amd import _lib
from tests import select_ref as S
from tests.conftest import load_golden
from tests.kernel_harness import DEV, SENT32, _Buf, _st

pytestmark = pytest.mark.gpu
MAX = S.INT32_MAX


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _i32(init):
    """A guarded int32 buffer holding `init`."""
    init = np.asarray(init).reshape(-1)
    b = _Buf(init.size, torch.int32)
    b.body().copy_(_dev(init.astype(np.int64).astype(np.uint32).view(np.int32)))          # uint32 words and negative ints alike
    return b


def _packed(x, dirty):
    """svdd_pack_tokens' rule (select_ref.pack_ref) in a guarded buffer; dirty: random bits in the padding of the last word."""
    p = S.pack_ref(x)
    L = x.shape[1]
    if dirty and L % 16:
        junk = np.random.default_rng(L).integers(0, 1 << 32, p.shape[0], dtype=np.uint64).astype(np.uint32)
        p[:, -1] |= junk & ~np.uint32((1 << (2 * (L % 16))) - 1)
    return _i32(p)


def _family_rows(n, L, seed):
    """Rows near each other: radius 0 and 1 have hits, L - 1 has misses where L allows any."""
    return S.planted(n, L, 3, min(2, L), seed, copy_share=0.3, rc_share=0.3)[0]


# ---------------------------------------------------------------------------------------------------- svdd_within ----
SIZES = [(1, 1), (63, 65), (64, 64), (65, 63), (257, 257), (1, 257), (257, 1)]


@pytest.mark.parametrize("L", [1, 15, 16, 17, 33, 200, 1024])
def test_within_equals_the_reference(L):
    lib = _lib.lib()
    n_case = 0
    for si, (B, N) in enumerate(SIZES):
        xq, xdb = _family_rows(B, L, 10 + si), _family_rows(N, L, 10 + si)[::-1].copy()   # the same founders on both sides
        q, db = _packed(xq, True), _packed(xdb, True)
        q_rc = _packed(S.revcomp(xq).astype(np.uint8), True)
        D = {rc: S.distance_matrix(xq, xdb, rc) for rc in (False, True)}
        counts = [None, 0, max(1, N - 20), N + 9] if N > 1 else [None, 0, 5]       # N - 20: in the middle of a tile
        for ri, radius in enumerate(sorted({0, min(1, L - 1), L - 1})):
            for ci, count in enumerate(counts):
                rc = bool((si + ri + ci) % 2)
                extra = (si + ci) % 2                                          # words of mask beyond ceil(N / 32)
                mw = (N + 31) // 32 + extra
                first0 = np.full(B, MAX, np.int64)
                first0[::3] = SENT32                                           # any earlier value: here the sentinel itself
                first0[1::5] = 0                                               # below every answer: stays
                want_first, want_mask = S.within_of(D[rc], radius, count, first0, mw)
                cnt = None if count is None else _i32(np.array([count]))
                for outputs in ("both", "first", "mask"):
                    first = _i32(first0) if outputs != "mask" else None
                    mask = _Buf(B * mw, torch.int32) if outputs != "first" else None
                    code = lib.svdd_within(q.ptr, q_rc.ptr if rc else None, db.ptr, None if cnt is None else cnt.ptr, B, N, L, radius,
                                           None if first is None else first.ptr, None if mask is None else mask.ptr, mw, _st())
                    _lib.check(code, "svdd_within")
                    torch.cuda.synchronize()
                    q.untouched(), db.untouched(), q_rc.untouched(), cnt is None or cnt.untouched()       # the guards
                    what = (L, B, N, radius, count, rc, outputs)
                    if first is not None:
                        first.untouched()
                        assert np.array_equal(first.cpu().numpy(), want_first), what
                    if mask is not None:
                        mask.assert_written(f"svdd_within mask {what}")      # every word, the ones beyond the count too
                        assert np.array_equal(mask.cpu().numpy().view(np.uint32).reshape(B, mw), want_mask), what
                    n_case += 1
        if L > 1 and N > 1 and B > 1:                                          # the data has hits and misses at the small radii
            hits = D[False] <= min(1, L - 1)
            assert hits.any() and (L < 15 or not hits.all())
    assert n_case >= 60


def test_within_many_segments():
    """A database long enough for several segments per workgroup column: the mask words of every segment, `first` across
    segments by atomic min, and a device count that ends in the middle of one segment and leaves the later ones empty."""
    lib = _lib.lib()
    B, N, L = 260, 40000, 16
    rng = np.random.default_rng(0)
    xq, xdb = rng.integers(0, 4, (B, L)).astype(np.uint8), rng.integers(0, 4, (N, L)).astype(np.uint8)
    xdb[rng.integers(0, N, 1500)] = xq[rng.integers(0, B, 1500)]                # exact copies of the queries
    q, db = _packed(xq, False), _packed(xdb, False)
    # distances on the packed words with numpy: 2-bit fields that differ
    pq, pdb = S.pack_ref(xq)[:, 0], S.pack_ref(xdb)[:, 0]
    v = pq[:, None] ^ pdb[None, :]
    v = (v | (v >> np.uint32(1))) & np.uint32(0x55555555)
    D = np.zeros(v.shape, np.int16)
    for s in range(0, 32, 2):
        D += ((v >> np.uint32(s)) & np.uint32(1)).astype(np.int16)
    mw = (N + 31) // 32
    for count in (None, 17777):
        want_first, want_mask = S.within_of(D, 3, count, None, mw)
        cnt = None if count is None else _i32(np.array([count]))
        first, mask = _i32(np.full(B, MAX)), _Buf(B * mw, torch.int32)
        _lib.check(lib.svdd_within(q.ptr, None, db.ptr, None if cnt is None else cnt.ptr, B, N, L, 3, first.ptr, mask.ptr, mw, _st()),
                   "svdd_within")
        torch.cuda.synchronize()
        first.untouched()
        mask.assert_written("svdd_within mask")
        assert np.array_equal(first.cpu().numpy(), want_first)
        assert np.array_equal(mask.cpu().numpy().view(np.uint32).reshape(B, mw), want_mask)
        assert (want_first != MAX).sum() > B // 2


# ----------------------------------------------------------------------------------------------- svdd_greedy_pick ----
def _bit_matrix(T, density, rng, symmetric=True):
    close = rng.random((T, T)) < density
    if symmetric:
        close = np.triu(close, 1)
        close = close | close.T
        close[np.arange(T), np.arange(T)] = rng.random(T) < 0.5                # the diagonal does no harm either way
    return close


def _mask_words(close, mw, rng):
    T = close.shape[0]
    bits = np.zeros((T, 32 * mw), bool)
    bits[:, :T] = close
    bits[:, T:] = rng.random((T, 32 * mw - T)) < 0.5                           # junk in the padding bits and the extra words
    return (bits.reshape(T, mw, 32).astype(np.uint32) << np.arange(32, dtype=np.uint32)).sum(2, dtype=np.uint32)


def _run_pick(close, first, k, count0, cap, L, base, rng, extra_words=0):
    """One launch in guarded buffers against greedy_pick_ref -> the number of picks made."""
    T, W = close.shape[0], (L + 15) // 16
    mw = (T + 31) // 32 + extra_words
    rows = rng.integers(0, 1 << 32, (T, W), dtype=np.uint64).astype(np.uint32)
    mask, rowb = _i32(_mask_words(close, mw, rng)), _i32(rows)
    firstb = None if first is None else _i32(first)
    count, reps, ranks, rep_pick = _i32(np.array([count0])), _Buf(cap * W, torch.int32), _Buf(cap, torch.int32), _Buf(T, torch.int32)
    code = _lib.lib().svdd_greedy_pick(mask.ptr, mw, None if firstb is None else firstb.ptr, rowb.ptr, T, L, base, k, count.ptr,
                                       reps.ptr, ranks.ptr, cap, rep_pick.ptr, _st())
    _lib.check(code, "svdd_greedy_pick")
    torch.cuda.synchronize()
    mask.untouched(), rowb.untouched(), count.untouched(), firstb is None or firstb.untouched()
    want, picks, count1 = S.greedy_pick_ref(close, first, k, count0, cap)
    what = (T, k, count0, cap, L)
    rep_pick.assert_written(f"rep_pick {what}")
    assert np.array_equal(rep_pick.cpu().numpy(), want), what
    assert int(count.cpu()[0]) == count1 == count0 + len(picks) <= cap, what
    new = np.zeros(cap, bool)
    new[count0:count1] = True                                                 # appended: nothing before, nothing beyond, guards intact
    ranks.assert_written_where(f"picked_rank {what}", _dev(new))
    reps.assert_written_where(f"reps {what}", _dev(np.repeat(new, W)))
    assert np.array_equal(ranks.cpu().numpy()[count0:count1], base + np.asarray(picks, np.int64)), what
    assert np.array_equal(reps.cpu().numpy().view(np.uint32).reshape(cap, W)[count0:count1], rows[picks].reshape(-1, W)), what
    return len(picks)


@pytest.mark.parametrize("T", [1, 31, 32, 33, 64, 65, 1000])
def test_greedy_pick_equals_the_reference(T):
    rng = np.random.default_rng(T)
    made = []
    for density in (0.0, 2.0 / T, 0.3):
        close = _bit_matrix(T, density, rng)
        free = S.greedy_pick_ref(close, None, T, 0, T)[2]                     # picks of the block on its own
        for count0 in (0, 5):
            first = np.full(T, MAX, np.int64)
            if count0:
                has = rng.random(T) < 0.3
                first[has] = rng.integers(0, count0, has.sum())
            own = S.greedy_pick_ref(close, first, T + count0, count0, T + count0)[2] - count0
            #    k reached before the block,  inside it,                        never;      cap exactly reached (k beyond it)
            for k, cap in ((max(count0, 1), T + 8), (count0 + (own + 1) // 2, T + 8), (count0 + T + 3, count0 + T + 3),
                           (count0 + T + 3, max(1, count0 + own))):
                if k < 1 or (count0 == 0 and k == 0):
                    continue
                made.append(_run_pick(close, first if count0 else None, k, count0, cap, 33, 1000 * count0, rng,
                                      extra_words=int(density > 0.1)))
        assert free >= 1
    assert max(made) >= 1 and (T == 1 or min(made) < max(made))


def test_greedy_pick_other_shapes():
    """A matrix that is not symmetric (only the bits j > i of a picked row may matter), rows of one word and of 64 words, the second
    register of the settled set (T > 2048), and a count the state cannot hold (nothing is written)."""
    rng = np.random.default_rng(1)
    close = _bit_matrix(200, 0.05, rng, symmetric=False)
    assert _run_pick(close, None, 500, 0, 200, 16, 7, rng) > 1
    assert _run_pick(np.triu(close, 1), None, 500, 3, 300, 1024, 0, rng) > 1
    big = _bit_matrix(2500, 0.002, rng)
    first = np.full(2500, MAX, np.int64)
    first[rng.random(2500) < 0.2] = 1
    assert _run_pick(big, first, 5000, 2, 2600, 200, 1 << 20, rng) > 64
    T, W = 40, 3
    mask, rows = _i32(_mask_words(close[:T, :T], 2, rng)), _i32(np.zeros((T, W), np.uint32))
    for bad in (-1, 11):
        count, reps, ranks, rep_pick = _i32(np.array([bad])), _Buf(10 * W, torch.int32), _Buf(10, torch.int32), _Buf(T, torch.int32)
        _lib.check(_lib.lib().svdd_greedy_pick(mask.ptr, 2, None, rows.ptr, T, 33, 0, 5, count.ptr, reps.ptr, ranks.ptr, 10, rep_pick.ptr,
                                               _st()), "svdd_greedy_pick")
        torch.cuda.synchronize()
        reps.assert_untouched("reps"), ranks.assert_untouched("picked_rank"), rep_pick.assert_untouched("rep_pick")
        assert int(count.cpu()[0]) == bad


# ------------------------------------------------------------------------------------------------------- the public ----
@functools.lru_cache(maxsize=None)
def _ref(name, rc, with_scores=True):
    x, scores, min_dist = S.case(name)[:3] if name in S.CASES else S.degenerate(name)
    return S.select_ref(x, scores if with_scores else None, None, min_dist, rc)


def _same(got, want, what):
    assert got.picked.dtype == got.rep.dtype == torch.int64 and got.rep_dist.dtype == torch.int32, what
    for g, w, n in zip(got, want, got._fields):
        assert np.array_equal(g.cpu().numpy(), w), (what, n)


@pytest.mark.parametrize("rc", [False, True])
@pytest.mark.parametrize("name", list(S.CASES))
def test_select_diverse_equals_the_reference(name, rc):
    from svdd_amd import quality
    x, scores, min_dist, T = S.case(name)
    N = x.shape[0]
    full = _ref(name, rc)
    xd, sd = _dev(x), _dev(scores)
    for block_rows in (1, 7, 64, 1024, T, None):
        _same(quality.select_diverse(xd, sd, None, min_dist, rc, block_rows), full, (name, rc, block_rows))
    runs = {}
    for k in (1, 3, N + 5):
        runs[k] = quality.select_diverse(x, scores, k, min_dist, rc, T)       # host data: checked there, moved by the wrapper
        _same(runs[k], S.prefix_of(*full, k), (name, rc, k))
    # the prefix property between two real runs
    three = S.prefix_of(*[t.cpu().numpy() for t in runs[N + 5]], 3)
    _same(runs[3], three, (name, rc, "prefix"))
    _same(quality.select_diverse(xd.long(), None, None, min_dist, rc, T), _ref(name, rc, False), (name, rc, "given order"))


def test_select_diverse_orders_by_a_stable_descending_sort():
    from svdd_amd import quality
    x, _, min_dist, T = S.case("odd")
    N = x.shape[0]
    rng = np.random.default_rng(3)
    scores = rng.integers(-2, 3, N).astype(np.float32)                        # five values: ties everywhere, -0.0 and 0.0 among them
    scores[rng.random(N) < 0.1] = -0.0
    scores[rng.random(N) < 0.05] = np.inf
    scores[rng.random(N) < 0.05] = -np.inf
    for dtype in (np.float32, np.float64):
        s = scores.astype(dtype)
        for k in (None, 4):
            _same(quality.select_diverse(x, torch.from_numpy(s), k, min_dist, True, T), S.select_ref(x, s, k, min_dist, True), (dtype, k))
    _same(quality.select_diverse(_dev(x), scores, None, 1, False), S.select_ref(x, scores, None, 1, False), "dedup")


@pytest.mark.parametrize("name", S.DEGENERATE)
def test_select_diverse_degenerate_cases(name):
    from svdd_amd import quality
    x, scores, min_dist = S.degenerate(name)
    for rc in (False, True):
        for k in (None, 1, 2):
            for block_rows in (None, 1, 3):
                want = S.select_ref(x, scores, k, min_dist, rc)
                _same(quality.select_diverse(x, scores, k, min_dist, rc, block_rows), want, (name, rc, k, block_rows))
    if name == "equal":
        assert len(S.select_ref(x, scores, None, min_dist, False)[0]) == 1


def test_a_token_above_3_raises():
    from svdd_amd import ops, quality
    bad = _dev(S.case("word")[0]).clone()
    bad[4, 4] = 4                                                             # on the device the kernel's err word speaks
    with pytest.raises(ops.SvddError, match="token > 3"):
        quality.select_diverse(bad, min_dist=2)


def _library_ref(x, scores, k, min_dist, rc):
    picked, rep, _ = S.select_ref(x, scores, None, min_dist, rc)
    N, P = x.shape[0], len(picked)
    n = min(k, P)
    s = scores.astype(np.float64)
    number = np.empty(N, np.int64)
    number[picked] = np.arange(P)
    rep_no = number[rep]
    return {"library_size": n, "library_score_mean": math.fsum(s[picked[:n]].tolist()) / n,
            "library_score_min": float(s[picked[:n]].min()),
            "topk_score_mean": math.fsum(np.sort(s)[::-1][:n].tolist()) / n, "families": P,
            "largest_family_fraction": int(np.bincount(rep_no, minlength=P).max()) / N,
            "library_family_coverage": int((rep_no < n).sum()) / N}


def test_library_quality_equals_the_reference():
    from svdd_amd import quality
    x, scores, min_dist, _ = S.case("gosai")
    for rc, k in ((False, 5), (True, 5), (True, 10 ** 6)):
        got, want = quality.library_quality(x, scores, k, min_dist, rc), _library_ref(x, scores, k, min_dist, rc)
        assert list(got) == list(want)
        assert got == want, (got, want)                                       # the means are correctly rounded sums: exact too
        assert got["families"] > 5 and got["library_size"] == min(k, got["families"])
        assert got["topk_score_mean"] >= got["library_score_mean"] and 0 < got["library_family_coverage"] <= 1
    assert quality.library_quality(x, scores, 10 ** 6, min_dist)["library_family_coverage"] == 1.0


def test_harness_select_library_and_cli(tmp_path):
    from svdd_amd import cli
    from svdd_amd.harness import BaseModel
    from svdd_amd.value_nets import RewardModel
    from tests import e2e_parity
    model, emb, head = e2e_parity.tiny_engine(load_golden("nets_tiny.npz"), 50, 4, DEV)
    reward = RewardModel(emb, head).to(DEV).eval()
    model.rng_mode, model.philox_seed = "philox", 9
    hm = BaseModel(emb, head, model, reward, batch_size=4, task="dna")
    samples = hm.controlled_decode(gen_batch_num=2, sample_M=2)[0]
    x = torch.cat(samples)
    x = torch.cat([x, x[:3], 3 - x[5:6].flip(1)])                             # near copies: three duplicates and a reverse complement
    scores = torch.cat([hm._reward(x[i:i + 4].long()) for i in range(0, x.shape[0], 4)]).reshape(-1).float().cpu().numpy()
    for rc, families in ((False, 9), (True, 8)):
        tokens, sc, idx, report = hm.select_library(x, 5, 30, revcomp=rc)
        want = S.select_ref(x.cpu().numpy(), scores, 5, 30, rc)[0]
        assert np.array_equal(idx.cpu().numpy(), want) and torch.equal(tokens, x[idx])
        assert np.array_equal(sc.cpu().numpy(), scores[want])
        assert report == _library_ref(x.cpu().numpy(), scores, 5, 30, rc) and report["families"] <= families
    listed = hm.select_library(list(x.split(4)), 5, 30)                        # `samples` as in evaluate_nll
    assert torch.equal(listed[2], hm.select_library(x, 5, 30)[2])
    args = ["--task", "rna", "--batch_size", "4", "--sample_M", "2", "--val_batch_num", "2", "--rng", "philox"]
    path, out = cli.main("mc", args + ["--out_dir", str(tmp_path / "on"), "--select", "3", "--select_min_dist", "2", "--select_revcomp"])
    z = np.load(path)
    keys = ["library_size", "library_score_mean", "library_score_min", "library_topk_score_mean", "library_families",
            "library_largest_family_fraction", "library_family_coverage"]
    assert sorted(z.files) == sorted(["baseline", "decoding", "selected", "selected_idx", "selected_scores"] + keys)
    xs, decoding = torch.cat(out[0]).cpu().numpy(), z["decoding"].reshape(-1)
    assert np.array_equal(z["selected_scores"], decoding[z["selected_idx"]])
    assert np.array_equal(z["selected_idx"], S.select_ref(xs, decoding, 3, 2, True)[0])
    assert np.array_equal(z["selected"], xs[z["selected_idx"]]) and int(z["library_size"]) == len(z["selected_idx"]) == 3
    plain, _ = cli.main("mc", args + ["--out_dir", str(tmp_path / "off")])
    assert sorted(np.load(plain).files) == ["baseline", "decoding"]           # without the flags the file is what it was
    with pytest.raises(SystemExit):
        cli.main("mc", args + ["--select_min_dist", "2"])                     # refused without --select
