"""Diverse library selection without a GPU: the numpy restatement of the contract (tests/select_ref.py) against an
independent property check, the non-vacuity of the case table that tests/test_select_gpu.py runs, and everything the two entries
and their Python wrappers refuse before a device is touched."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from tests import select_ref as S

KS = (1, 3, None)


def _rank(scores, N):
    rank = np.empty(N, np.int64)
    rank[S.order_of(scores, N)] = np.arange(N)
    return rank


# -------------------------------------------------------------------------------------------------- the reference ----
@pytest.mark.parametrize("rc", [False, True])
@pytest.mark.parametrize("name", ["odd", "word"] + list(S.DEGENERATE))
def test_reference_has_the_properties_of_the_contract(name, rc):
    x, scores, min_dist = S.case(name)[:3] if name in S.CASES else S.degenerate(name)
    N = x.shape[0]
    full = S.select_ref(x, scores, None, min_dist, rc)
    assert (full[1] >= 0).all() and (full[2] >= 0).all()                      # k = None: every row has a representative
    for k in KS + (N + 5,):
        got = S.select_ref(x, scores, k, min_dist, rc)
        S.check_selection(x, scores, k, min_dist, rc, *got)
        want = S.prefix_of(*full, N if k is None else k)                     # the prefix property
        for g, w in zip(got, want):
            assert np.array_equal(g, w), (name, k)
    # scores = None is the given order; min_dist = 1 keeps exactly one row of every group of equal rows (with rc: of every
    # group of rows equal up to the strand)
    S.check_selection(x, None, None, min_dist, rc, *S.select_ref(x, None, None, min_dist, rc))
    picked = S.select_ref(x, scores, None, 1, rc)[0]
    canon = {min(r.tobytes(), S.revcomp(r).astype(np.uint8).tobytes()) if rc else r.tobytes() for r in x}
    assert len(picked) == len(canon)


def test_order_is_a_stable_descending_sort():
    s = np.array([0.0, -0.0, 1.0, np.inf, 1.0, -np.inf, np.inf, 0.0], np.float32)
    assert S.order_of(s, 8).tolist() == [3, 6, 2, 4, 0, 1, 7, 5]
    assert S.order_of(None, 3).tolist() == [0, 1, 2]


@pytest.mark.parametrize("name", list(S.CASES))
def test_case_table_is_not_vacuous(name):
    """On the reference alone: each case of the shared table exercises what the kernels can get wrong."""
    x, scores, min_dist, T = S.case(name)
    N = x.shape[0]
    assert len(np.unique(scores)) < N                                         # tied scores
    rank = _rank(scores, N)
    for rc in (False, True):
        picked, rep, _ = S.select_ref(x, scores, None, min_dist, rc)
        assert 1 < len(picked) < N, (name, rc, len(picked))
        sup = rep != np.arange(N)                                             # the suppressed rows
        same = rank[rep] // T == rank // T
        assert (sup & same).any(), (name, rc, "no row suppressed by a pick of its own block")
        assert (sup & ~same).any(), (name, rc, "no row suppressed by a pick of an earlier block")
        if rc:
            xi = x.astype(np.int64)
            fwd = (xi != xi[rep]).sum(1)
            rev = (S.revcomp(xi) != xi[rep]).sum(1)
            assert (sup & (fwd >= min_dist) & (rev < min_dist)).any(), (name, "no row represented through the reverse strand only")


def test_kernel_references_agree_with_the_walk():
    """within_ref + greedy_pick_ref composed in blocks, as the host composes the kernels, is select_ref."""
    x, scores, min_dist, T = S.case("odd")
    N = x.shape[0]
    for rc, k in ((False, None), (True, None), (True, 5)):
        order = S.order_of(scores, N)
        xs = x[order]
        cap = N if k is None else k
        count, reps, picked_rank, rep_pick = 0, [], [], np.empty(N, np.int32)
        for r0 in range(0, N, T):
            blk = xs[r0:r0 + T]
            first = S.within_ref(blk, np.asarray(reps).reshape(-1, x.shape[1]), min_dist - 1, rc)[0] if reps else None
            _, mask = S.within_ref(blk, blk, min_dist - 1, rc)
            close = ((mask[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(len(blk), -1)[:, :len(blk)].astype(bool)
            rp, rows, count = S.greedy_pick_ref(close, first, cap, count, cap)
            rep_pick[r0:r0 + T] = rp
            reps += [blk[r] for r in rows]
            picked_rank += [r0 + r for r in rows]
        picked = order[np.asarray(picked_rank, np.int64)]
        rep = np.empty(N, np.int64)
        rep[order] = np.where(rep_pick >= 0, picked[np.maximum(rep_pick, 0)], -1)
        want = S.select_ref(x, scores, k, min_dist, rc)
        assert np.array_equal(picked, want[0]) and np.array_equal(rep, want[1]), (rc, k)


# ------------------------------------------------------------------------------------------------------ the entries ----
def test_entries_refuse_bad_arguments_without_a_device():
    from svdd_amd import _lib
    L_ = _lib.lib()
    assert _lib.ABI_VERSION == 17 and L_.svdd_abi_version() == 17
    for name, n in (("svdd_within", 12), ("svdd_greedy_pick", 14)):
        sig = _lib.SIGNATURES[name]
        assert name in _lib.EXPORTS and sig[-1] is _lib.vp and _lib.STREAM not in sig and len(sig) == n
    p = [ctypes.c_void_p(4096 * (i + 1)) for i in range(7)]                   # non-NULL pointers that are never dereferenced

    def within(**kw):
        a = dict(q=p[0], q_rc=p[1], db=p[2], db_count=p[3], B=3, N=70, L=20, radius=4, first=p[4], mask=p[5], mask_words=3, stream=None)
        a.update(kw)
        return L_.svdd_within(*a.values())
    for what, kw in {"q null": dict(q=None), "db null": dict(db=None), "both outputs null": dict(first=None, mask=None),
                     "radius < 0": dict(radius=-1), "radius = L": dict(radius=20), "radius > L": dict(radius=21),
                     "L = 0": dict(L=0, radius=0), "L < 0": dict(L=-1, radius=0), "L = 1025": dict(L=1025),
                     "B = 0": dict(B=0), "N = 0": dict(N=0), "B < 0": dict(B=-2), "N < 0": dict(N=-2),
                     "mask_words too small": dict(mask_words=2), "mask_words = 0": dict(mask_words=0),
                     "mask_words < 0": dict(mask_words=-1)}.items():
        assert within(**kw) == _lib.E_ARG, what

    def pick(**kw):
        a = dict(mask=p[0], mask_words=3, first=p[1], rows=p[2], T=70, L=20, base=0, k=5, count=p[3], reps=p[4], picked_rank=p[5],
                 cap=5, rep_pick=p[6], stream=None)
        a.update(kw)
        return L_.svdd_greedy_pick(*a.values())
    top = (1 << 31) - 1
    for what, kw in {"k = 0": dict(k=0), "k < 0": dict(k=-3), "T = 0": dict(T=0), "T < 0": dict(T=-1), "T = 4097": dict(T=4097, mask_words=200),
                     "mask_words too small": dict(mask_words=2), "mask_words = 0": dict(mask_words=0), "cap = 0": dict(cap=0),
                     "L = 0": dict(L=0), "L = 1025": dict(L=1025), "base < 0": dict(base=-1), "base + T = 2^31": dict(base=top - 69),
                     "mask null": dict(mask=None), "rows null": dict(rows=None), "count null": dict(count=None),
                     "reps null": dict(reps=None), "picked_rank null": dict(picked_rank=None), "rep_pick null": dict(rep_pick=None)}.items():
        assert pick(**kw) == _lib.E_ARG, what


# ------------------------------------------------------------------------------------------------------- the python ----
def test_wrappers_refuse_bad_arguments_before_any_launch():
    from svdd_amd import ops, quality
    x = torch.randint(0, 4, (6, 20), generator=torch.Generator().manual_seed(0))
    s = torch.rand(6, generator=torch.Generator().manual_seed(1))
    bad = x.clone()
    bad[1, 3] = 4
    for fn in (quality.select_diverse, lambda t: quality.library_quality(t, s[:t.shape[0]] if t.dim() == 2 else s, 2, 3)):
        with pytest.raises(ValueError, match="token"):
            fn(bad)                                                           # MASK has no 2-bit code
        with pytest.raises(ValueError, match="integer"):
            fn(x.float())
        with pytest.raises(ValueError, match=r"\[N, L\]"):
            fn(x[0])
        with pytest.raises(ValueError, match=r"\[N, L\]"):
            fn(x[:0])
    with pytest.raises(ValueError, match="1024"):
        quality.select_diverse(torch.zeros(2, 1025, dtype=torch.uint8))
    nan = s.clone()
    nan[2] = float("nan")
    for scores in (nan, nan.numpy(), s[:5], s.reshape(6, 1), torch.arange(6), [0.0] * 6):
        with pytest.raises(ValueError, match="scores"):
            quality.select_diverse(x, scores)
    with pytest.raises(ValueError, match="scores"):
        quality.library_quality(x, nan, 2, 3)
    with pytest.raises(ValueError, match="scores"):
        quality.library_quality(x, None, 2, 3)
    for min_dist in (0, -1, 21, 2.0, True, None):
        with pytest.raises(ValueError, match="min_dist ="):
            quality.select_diverse(x, s, min_dist=min_dist)
        with pytest.raises(ValueError, match="min_dist ="):
            quality.library_quality(x, s, 2, min_dist)
    for k in (0, -2, 1.5, True):
        with pytest.raises(ValueError, match="k ="):
            quality.select_diverse(x, s, k=k)
        with pytest.raises(ValueError, match="k ="):
            quality.library_quality(x, s, k, 3)
    with pytest.raises(ValueError, match="k ="):
        quality.library_quality(x, s, None, 3)                                # a library has a size
    for rows in (0, -4, 1.5, True, 4097):
        with pytest.raises(ValueError, match="block_rows ="):
            quality.select_diverse(x, s, block_rows=rows)
    if not torch.cuda.is_available():
        with pytest.raises(ops.SvddError, match="GPU"):                       # valid arguments: no CPU fallback
            quality.select_diverse(x, s, k=2, min_dist=3, revcomp=True, block_rows=4)
    # the raw wrappers check their numbers first and take device tensors only
    q, m = torch.zeros(3, 2, dtype=torch.int32), torch.zeros(3, 1, dtype=torch.int32)
    c, f = torch.zeros(1, dtype=torch.int32), torch.zeros(3, dtype=torch.int32)
    for L in (0, 1025, 20.0):
        with pytest.raises(ops.SvddError, match="L ="):
            ops.within(q, q, L, 0, first=f)
        with pytest.raises(ops.SvddError, match="L ="):
            ops.greedy_pick(m, f, q, L, 0, 1, c, q, f, f)
    for radius in (-1, 20, 1.0, True):
        with pytest.raises(ops.SvddError, match="radius ="):
            ops.within(q, q, 20, radius, first=f)
    for k in (0, -1, 2.0):
        with pytest.raises(ops.SvddError, match="k ="):
            ops.greedy_pick(m, f, q, 20, 0, k, c, q, f, f)
    with pytest.raises(ops.SvddError, match="base ="):
        ops.greedy_pick(m, f, torch.zeros(3, 2, dtype=torch.int32), 20, -1, 1, c, q, f, f)
    with pytest.raises(ops.SvddError, match="GPU"):
        ops.within(q, q, 20, 3, first=f)
    with pytest.raises(ops.SvddError, match="GPU"):
        ops.greedy_pick(m, f, q, 20, 0, 1, c, q, f, f)


def test_public_signatures_and_the_flags():
    from svdd_amd import cli, ops, quality
    from svdd_amd.harness import BaseModel
    sig = lambda f: list(inspect.signature(f).parameters)                     # noqa: E731
    assert sig(ops.within) == ["q", "db", "L", "radius", "q_rc", "db_count", "first", "mask"]
    assert sig(ops.greedy_pick) == ["mask", "first", "rows", "L", "base", "k", "count", "reps", "picked_rank", "rep_pick"]
    assert sig(quality.select_diverse) == ["x", "scores", "k", "min_dist", "revcomp", "block_rows"]
    d = {n: p.default for n, p in inspect.signature(quality.select_diverse).parameters.items()}
    assert d == {"x": inspect.Parameter.empty, "scores": None, "k": None, "min_dist": 1, "revcomp": False, "block_rows": None}
    assert quality.Selection._fields == ("picked", "rep", "rep_dist")
    assert sig(quality.library_quality) == ["x", "scores", "k", "min_dist", "revcomp"]
    assert sig(BaseModel.select_library) == ["self", "samples", "k", "min_dist", "revcomp"]
    assert sig(quality.sample_quality) == ["x", "refs", "train", "k", "scores", "ref_scores"]          # pinned, unchanged
    assert 1 <= quality.SELECT_BLOCK_ROWS <= ops.PICK_MAX_ROWS == 4096
    # the flags: absent from the default namespace, parsed when given, refused without --select before any model is built
    ns = cli.build_parser().parse_args([])
    assert not any(hasattr(ns, f) for f in ("select", "select_min_dist", "select_revcomp"))
    ns = cli.build_parser().parse_args(["--select", "8", "--select_min_dist", "5", "--select_revcomp"])
    assert ns.select == 8 and ns.select_min_dist == 5 and ns.select_revcomp is True
    ns = cli.build_parser().parse_args(["--select", "8"])
    assert ns.select == 8 and not hasattr(ns, "select_min_dist") and not hasattr(ns, "select_revcomp")
    assert not hasattr(ns, "eval_quality")                                    # --select does not need --eval_quality
    for flags in (["--select_min_dist", "5"], ["--select_revcomp"], ["--select_min_dist", "5", "--select_revcomp"]):
        with pytest.raises(SystemExit):
            cli.main("mc", flags)
        with pytest.raises(ValueError, match="needs --select K"):
            cli.run(cli.build_parser().parse_args(flags))
