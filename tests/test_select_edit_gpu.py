"""-m gpu: diverse library selection under a minimum edit distance. Everything here is an exact integer and must
EQUAL tests/select_edit_ref.py (tests/edit_ref.py's Wagner-Fischer table; at L >= 64 as recorded in tests/golden).

  svdd_edit_within  through the raw C entry in sentinel-guarded buffers (tests/kernel_harness.py), each output once NULL and once
                    given: every class of plane words and every edge of a plane word and of a packed word with dirty padding bits,
                    tile / workgroup edges on both sides, radius 0, 1, about L / 8 and L - 1, one and both strands, every kind of
                    device count, seeded `first`, extra mask words; many segments; at 257 x 257 rows of 1024 against svdd_edit_nn
  svdd_edit_pairs   raw, in guarded buffers: equal and unequal lengths, idx with -1, repeats and rows that do not exist, cap 0, mid
                    and max, both strands
  public            quality.select_diverse_edit on the shared case table for every block_rows, edit_distance,
                    library_quality_edit, BaseModel.select_library_edit and --select_metric
"""
import math

import numpy as np
import pytest
import torch

from svdd_amd import _lib
from tests import select_edit_ref as E
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


def _packed(x, dirty=True):
    """svdd_pack_tokens' rule (select_ref.pack_ref) in a guarded buffer; dirty: random bits in the padding of the last word."""
    p = S.pack_ref(x)
    L = x.shape[1]
    if dirty and L % 16:
        junk = np.random.default_rng(L).integers(0, 1 << 32, p.shape[0], dtype=np.uint64).astype(np.uint32)
        p[:, -1] |= junk & ~np.uint32((1 << (2 * (L % 16))) - 1)
    return _i32(p)


def _bits(mask, N):
    """mask u32 [B, mw] -> bool [B, N]."""
    return ((mask[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(mask.shape[0], -1)[:, :N].astype(bool)


# ----------------------------------------------------------------------------------------------- svdd_edit_within ----
@pytest.mark.parametrize("L", E.KERNEL_LS)
def test_edit_within_equals_the_reference(L):
    lib = _lib.lib()
    if L >= 16:
        assert E.kernel_case_is_not_vacuous(L) == [True] * 4, L                # on the reference alone
    n_case = 0
    for si, (B, N) in enumerate(E.kernel_sizes(L)):
        xq, xdb, D = E.kernel_case(L, si)
        q, db = _packed(xq), _packed(xdb)
        counts = [None, 0, max(1, N - 20), N + 9] if N > 1 else [None, 0, 5]       # N - 20: in the middle of a tile
        for ri, radius in enumerate(sorted({0, min(1, L - 1), E.mid_radius(L), L - 1})):
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
                    code = lib.svdd_edit_within(q.ptr, db.ptr, None if cnt is None else cnt.ptr, B, N, L, radius, int(rc),
                                                None if first is None else first.ptr, None if mask is None else mask.ptr, mw, _st())
                    _lib.check(code, "svdd_edit_within")
                    torch.cuda.synchronize()
                    q.untouched(), db.untouched(), cnt is None or cnt.untouched()                         # the guards
                    what = (L, B, N, radius, count, rc, outputs)
                    if first is not None:
                        first.untouched()
                        assert np.array_equal(first.cpu().numpy(), want_first), what
                    if mask is not None:
                        mask.assert_written(f"svdd_edit_within mask {what}")  # every word, the ones beyond the count too
                        assert np.array_equal(mask.cpu().numpy().view(np.uint32).reshape(B, mw), want_mask), what
                    n_case += 1
    assert n_case >= (18 if L == 1 else 60 if L <= 65 else 42)


def test_edit_within_many_segments():
    """A database long enough for several segments per workgroup column: the mask words of every segment, `first` across
    segments by atomic min, and a device count that ends in the middle of one segment and leaves the later ones empty."""
    lib = _lib.lib()
    xq, xdb, hits = E.segment_case()
    B, N, L = E.SEG_B, E.SEG_N, E.SEG_L
    D = np.where(hits, 0, L).astype(np.int8)                                  # all within_of needs: within the radius or not
    q, db = _packed(xq, False), _packed(xdb, False)
    mw = (N + 31) // 32
    for count in (None, 8888):
        want_first, want_mask = S.within_of(D, 0, count, None, mw)
        cnt = None if count is None else _i32(np.array([count]))
        first, mask = _i32(np.full(B, MAX)), _Buf(B * mw, torch.int32)
        _lib.check(lib.svdd_edit_within(q.ptr, db.ptr, None if cnt is None else cnt.ptr, B, N, L, E.SEG_RADIUS, 0, first.ptr, mask.ptr,
                                        mw, _st()), "svdd_edit_within")
        torch.cuda.synchronize()
        first.untouched()
        mask.assert_written("svdd_edit_within mask")
        assert np.array_equal(first.cpu().numpy(), want_first)
        assert np.array_equal(mask.cpu().numpy().view(np.uint32).reshape(B, mw), want_mask)
        assert (want_first != MAX).sum() > B // 2


def test_edit_within_at_1024_agrees_with_edit_nn():
    """A size the numpy table cannot reach, as a supplement to the reference: 257 x 257 planted rows of 1024. The number of mask
    bits is the number of pairs svdd_edit_nn's histogram counts within the radius, and the two-strand mask is the one-strand
    masks of the queries and of their reverse complements, OR-ed."""
    from svdd_amd import ops
    x = E.planted_indel(257, 1024, 4, 16, 3)[0]
    radius, mw = 20, 9
    q, q_rc = ops.pack_tokens(_dev(x)), ops.pack_tokens(_dev(S.revcomp(x).astype(np.uint8)))
    masks = {}
    for name, (rows, both) in {"fwd": (q, False), "rev": (q_rc, False), "both": (q, True)}.items():
        masks[name] = torch.empty((257, mw), dtype=torch.int32, device=DEV)
        ops.edit_within(rows, q, 1024, radius, both_strands=both, mask=masks[name])
        hist = torch.zeros(radius + 2, dtype=torch.int64, device=DEV)
        ops.edit_nn(rows, q, 1024, 1024, radius, hist=hist)
        bits = _bits(masks[name].cpu().numpy().view(np.uint32), 257)
        if name != "both":
            assert int(bits.sum()) == int(hist[:radius + 1].sum()) > 257, name
    assert torch.equal(masks["both"], masks["fwd"] | masks["rev"]) and not torch.equal(masks["both"], masks["fwd"])


def test_edit_within_records_under_its_own_profile_slot():
    """Slot 15 (SVDD_SLOT_EDIT_WITHIN, appended: the earlier numbers stay): one span per call, nothing in the slots of svdd_within
    (13) and svdd_greedy_pick (14)."""
    from svdd_amd import ops
    q = ops.pack_tokens(_dev(E.case("word")[0]))
    first = torch.full((q.shape[0],), ops.FIRST_INIT, dtype=torch.int32, device=DEV)
    try:
        torch.cuda.synchronize()
        for k in range(16):
            _lib.profile_collect(k)
        _lib.profile_enable(True)
        ops.edit_within(q, q, 16, 2, both_strands=True, first=first)
        _lib.profile_enable(False)
        torch.cuda.synchronize()
        got = [_lib.profile_collect(k) for k in range(16)]
    finally:
        _lib.profile_enable(False)
    assert [n for _, n in got] == [0] * 15 + [1] and got[15][0] > 0.0, got


# ------------------------------------------------------------------------------------------------ svdd_edit_pairs ----
def _pair_rows(B, N, Lq, Ld, seed):
    """db: N random rows; query i: row idx[i] of db cut or padded to Lq, with a few edits and, for a share, on the other strand."""
    rng = np.random.default_rng(seed)
    xdb = rng.integers(0, 4, (N, Ld))
    src = rng.integers(0, N, B)
    xq = np.empty((B, Lq), np.int64)
    for i in range(B):
        seq = xdb[src[i]].tolist()
        for _ in range(int(rng.integers(0, 6))):
            pos = int(rng.integers(len(seq)))
            if rng.random() < 0.5:
                seq.insert(pos, int(rng.integers(4)))
            elif len(seq) > 1:
                del seq[pos]
        row = np.asarray(seq[:Lq] + rng.integers(0, 4, max(0, Lq - len(seq))).tolist(), np.int64)
        xq[i] = 3 - row[::-1] if rng.random() < 0.3 else row
    return xq.astype(np.uint8), xdb.astype(np.uint8), src


@pytest.mark.parametrize("Lq,Ld", [(1, 1), (33, 33), (33, 40), (200, 197), (1024, 1000)])
def test_edit_pairs_equals_the_reference(Lq, Ld):
    lib = _lib.lib()
    N = 5
    xq, xdb, src = _pair_rows(257, N, Lq, Ld, Lq)
    idx = src.copy()
    idx[3::7] = (idx[3::7] + 1) % N                                            # not the row it was made from
    idx[2::11] = -1
    idx[5::13] = [N, N + 5, 2 ** 31 - 1, -7][:len(idx[5::13])] + [N] * max(0, len(idx[5::13]) - 4)      # rows that do not exist
    real = (idx >= 0) & (idx < N)
    d = {rc: np.full(257, -1, np.int64) for rc in (False, True)}
    for j in range(N):                                                        # 257 pairs, not 257 x 5
        rows = np.nonzero(real & (idx == j))[0]
        for rc in (False, True):
            d[rc][rows] = E.distance_matrix(xq[rows], xdb[j:j + 1], rc)[:, 0]
    assert (d[True] < d[False]).any() or Lq == 1
    db = _packed(xdb)
    mid = abs(Lq - Ld) + max(Lq, Ld) // 8                                      # the difference of the lengths is paid by every pair
    for B in (1, 65, 257):
        q, ix = _packed(xq[:B]), _i32(idx[:B])
        for cap in sorted({0, mid, max(Lq, Ld)}):
            for rc in (False, True):
                want = np.where(real[:B] & (d[rc][:B] <= cap), d[rc][:B], -1)
                dist = _Buf(B, torch.int32)
                _lib.check(lib.svdd_edit_pairs(q.ptr, db.ptr, ix.ptr, B, N, Lq, Ld, cap, int(rc), dist.ptr, _st()), "svdd_edit_pairs")
                torch.cuda.synchronize()
                q.untouched(), db.untouched(), ix.untouched()
                dist.assert_written(f"svdd_edit_pairs dist {(Lq, Ld, B, cap, rc)}")
                assert np.array_equal(dist.cpu().numpy(), want), (Lq, Ld, B, cap, rc)
                if B == 257 and cap == mid and Lq > 1:
                    assert (want >= 0).any() and (want[real] == -1).any()      # the cap bites, and not everywhere


# ------------------------------------------------------------------------------------------------------- the public ----
def _ref(name, rc, with_scores=True):
    x, scores, min_dist = E.case(name)[:3] if name in E.CASES else S.degenerate(name)
    return E.select_of(E.case_distances(name, rc), scores if with_scores else None, None, min_dist)


def _same(got, want, what):
    assert got.picked.dtype == got.rep.dtype == torch.int64 and got.rep_dist.dtype == torch.int32, what
    for g, w, n in zip(got, want, got._fields):
        assert np.array_equal(g.cpu().numpy(), w), (what, n)


@pytest.mark.parametrize("rc", [False, True])
@pytest.mark.parametrize("name", list(E.CASES))
def test_select_diverse_edit_equals_the_reference(name, rc):
    from svdd_amd import quality
    x, scores, min_dist, T = E.case(name)
    N = x.shape[0]
    full = _ref(name, rc)
    xd, sd = _dev(x), _dev(scores)
    for block_rows in (1, 7, T, 1024, None):
        _same(quality.select_diverse_edit(xd, sd, None, min_dist, rc, block_rows), full, (name, rc, block_rows))
    runs = {}
    for k in (1, 3, N + 5):
        runs[k] = quality.select_diverse_edit(x, scores, k, min_dist, rc, T)  # host data: checked there, moved by the wrapper
        _same(runs[k], S.prefix_of(*full, k), (name, rc, k))
    three = S.prefix_of(*[t.cpu().numpy() for t in runs[N + 5]], 3)           # the prefix property between two real runs
    _same(runs[3], three, (name, rc, "prefix"))
    _same(quality.select_diverse_edit(xd.long(), None, None, min_dist, rc, T), _ref(name, rc, False), (name, rc, "given order"))


def test_select_diverse_edit_orders_by_a_stable_descending_sort():
    from svdd_amd import quality
    x, _, min_dist, T = E.case("odd")
    N = x.shape[0]
    rng = np.random.default_rng(3)
    scores = rng.integers(-2, 3, N).astype(np.float32)                        # five values: ties everywhere, -0.0 and 0.0 among them
    scores[rng.random(N) < 0.1] = -0.0
    scores[rng.random(N) < 0.05] = np.inf
    scores[rng.random(N) < 0.05] = -np.inf
    D = E.case_distances("odd", True)
    for dtype in (np.float32, np.float64):
        s = scores.astype(dtype)
        for k in (None, 4):
            _same(quality.select_diverse_edit(x, torch.from_numpy(s), k, min_dist, True, T), E.select_of(D, s, k, min_dist), (dtype, k))


@pytest.mark.parametrize("name", S.DEGENERATE)
def test_select_diverse_edit_degenerate_cases(name):
    from svdd_amd import quality
    x, scores, min_dist = S.degenerate(name)
    for rc in (False, True):
        D = E.case_distances(name, rc)
        for k in (None, 1, 2):
            for block_rows in (None, 1, 3):
                want = E.select_of(D, scores, k, min_dist)
                _same(quality.select_diverse_edit(x, scores, k, min_dist, rc, block_rows), want, (name, rc, k, block_rows))
    if name == "equal":
        assert len(E.select_of(E.case_distances(name, False), scores, None, min_dist)[0]) == 1


def test_min_dist_1_is_the_hamming_selection():
    """Distance 0 means equal rows under either metric: two different kernels, one answer."""
    from svdd_amd import quality
    for name in ("odd", "gosai"):
        x, scores = E.case(name)[:2]
        for rc in (False, True):
            a, b = quality.select_diverse_edit(x, scores, None, 1, rc), quality.select_diverse(x, scores, None, 1, rc)
            for g, w in zip(a, b):
                assert torch.equal(g, w), (name, rc)
            assert 1 < a.picked.numel() < x.shape[0]                          # the planted copies are there to be removed


def test_a_token_above_3_raises():
    from svdd_amd import ops, quality
    bad = _dev(E.case("word")[0]).clone()
    bad[4, 4] = 4                                                             # on the device the kernel's err word speaks
    with pytest.raises(ops.SvddError, match="token > 3"):
        quality.select_diverse_edit(bad, min_dist=2)
    with pytest.raises(ops.SvddError, match="token > 3"):
        quality.edit_distance(bad, bad)


def test_edit_distance_equals_the_diagonal_of_the_table():
    from svdd_amd import quality
    rng = np.random.default_rng(5)
    for name in ("odd", "gosai"):
        x = E.case(name)[0]
        perm = rng.permutation(x.shape[0])
        for rc in (False, True):
            want = E.case_distances(name, rc)[np.arange(x.shape[0]), perm]
            got = quality.edit_distance(_dev(x), x[perm], revcomp=rc)
            assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want), (name, rc)
            cap = int(np.median(want))
            assert np.array_equal(quality.edit_distance(x, _dev(x[perm]), cap, rc).cpu().numpy(), np.where(want <= cap, want, -1))
    a, b = rng.integers(0, 4, (40, 70)), rng.integers(0, 4, (40, 61))          # lengths may differ
    b[::2, :50] = a[::2, 9:59]
    for rc in (False, True):
        want = np.diag(E.distance_matrix(a, b, rc))
        assert np.array_equal(quality.edit_distance(a, b, revcomp=rc).cpu().numpy(), want) and want.min() < 30 < want.max()


def _library_ref(D, scores, k, min_dist):
    picked, rep, _ = E.select_of(D, scores, None, min_dist)
    N, P = D.shape[0], len(picked)
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


def test_library_quality_edit_equals_the_reference():
    from svdd_amd import quality
    x, scores, min_dist, _ = E.case("gosai")
    for rc, k in ((False, 3), (True, 3), (True, 10 ** 6)):
        got, want = quality.library_quality_edit(x, scores, k, min_dist, rc), _library_ref(E.case_distances("gosai", rc), scores, k, min_dist)
        assert list(got) == list(want) == list(quality.library_quality(x, scores, k, min_dist, rc))
        assert got == want, (got, want)                                       # the means are correctly rounded sums: exact too
        assert got["families"] > 3 and got["library_size"] == min(k, got["families"])
        assert got["families"] < quality.library_quality(x, scores, k, min_dist, rc)["families"]      # shifted copies are one family
    assert quality.library_quality_edit(x, scores, 10 ** 6, min_dist)["library_family_coverage"] == 1.0


def test_harness_select_library_edit_and_cli(tmp_path):
    from svdd_amd import cli
    from svdd_amd.harness import BaseModel
    from svdd_amd.value_nets import RewardModel
    from tests import e2e_parity
    model, emb, head = e2e_parity.tiny_engine(load_golden("nets_tiny.npz"), 50, 4, DEV)
    reward = RewardModel(emb, head).to(DEV).eval()
    model.rng_mode, model.philox_seed = "philox", 9
    hm = BaseModel(emb, head, model, reward, batch_size=4, task="dna")
    x = torch.cat(hm.controlled_decode(gen_batch_num=2, sample_M=2)[0])
    n = x.shape[0]
    fill = torch.tensor([1, 2], dtype=x.dtype, device=x.device)
    shifted = torch.cat([x[0, 2:], fill])                                     # row 0 shifted by two bases
    rc_shifted = 3 - torch.cat([fill, x[1, :-2]]).flip(0)                      # row 1 shifted the other way, on the other strand
    x = torch.cat([x, shifted[None], rc_shifted[None], x[2:4]])               # ... and two exact duplicates
    xn = x.cpu().numpy()
    scores = torch.cat([hm._reward(x[i:i + 4].long()) for i in range(0, x.shape[0], 4)]).reshape(-1).float().cpu().numpy()
    min_dist = 10
    for rc in (False, True):
        D = E.distance_matrix(xn, xn, rc)
        ham, edit = S.select_ref(xn, scores, None, min_dist, rc)[0], E.select_of(D, scores, None, min_dist)[0]
        # on the reference: Hamming distance keeps the shifted copies as families of their own, edit distance does not
        assert {0, n} <= set(ham.tolist()) and not {0, n} <= set(edit.tolist())
        if rc:
            assert {1, n + 1} <= set(ham.tolist()) and not {1, n + 1} <= set(edit.tolist())
        tokens, sc, idx, report = hm.select_library(x, 100, min_dist, revcomp=rc)
        assert np.array_equal(idx.cpu().numpy(), ham)
        tokens, sc, idx, report = hm.select_library_edit(x, 100, min_dist, revcomp=rc)
        assert np.array_equal(idx.cpu().numpy(), edit) and torch.equal(tokens, x[idx]) and np.array_equal(sc.cpu().numpy(), scores[edit])
        assert report == _library_ref(D, scores, 100, min_dist) and report["families"] == len(edit) < len(ham)
        short = hm.select_library_edit(list(x.split(4)), 3, min_dist, revcomp=rc)         # `samples` as in evaluate_nll
        assert np.array_equal(short[2].cpu().numpy(), edit[:3]) and short[3]["library_size"] == 3
    args = ["--task", "rna", "--batch_size", "4", "--sample_M", "2", "--val_batch_num", "2", "--rng", "philox"]
    flags = ["--select", "3", "--select_min_dist", "2", "--select_revcomp"]
    keys = ["library_size", "library_score_mean", "library_score_min", "library_topk_score_mean", "library_families",
            "library_largest_family_fraction", "library_family_coverage"]
    today = sorted(["baseline", "decoding", "selected", "selected_idx", "selected_scores"] + keys)
    path, out = cli.main("mc", args + flags + ["--out_dir", str(tmp_path / "edit"), "--select_metric", "edit"])
    z = np.load(path)
    assert sorted(z.files) == sorted(today + ["library_metric"]) and str(z["library_metric"]) == "edit"
    xs, decoding = torch.cat(out[0]).cpu().numpy(), z["decoding"].reshape(-1)
    assert np.array_equal(z["selected_idx"], E.select_of(E.distance_matrix(xs, xs, True), decoding, 3, 2)[0])
    assert np.array_equal(z["selected_scores"], decoding[z["selected_idx"]]) and np.array_equal(z["selected"], xs[z["selected_idx"]])
    assert int(z["library_size"]) == len(z["selected_idx"]) == 3
    path, out = cli.main("mc", args + flags + ["--out_dir", str(tmp_path / "hamming"), "--select_metric", "hamming"])
    z, xs = np.load(path), torch.cat(out[0]).cpu().numpy()
    assert sorted(z.files) == today                                           # hamming: exactly today's file
    assert np.array_equal(z["selected_idx"], S.select_ref(xs, z["decoding"].reshape(-1), 3, 2, True)[0])
    plain, _ = cli.main("mc", args + ["--out_dir", str(tmp_path / "off")])
    assert sorted(np.load(plain).files) == ["baseline", "decoding"]           # without the flags the file is what it was
    with pytest.raises(SystemExit):
        cli.main("mc", args + ["--select_metric", "edit"])                    # refused without --select
