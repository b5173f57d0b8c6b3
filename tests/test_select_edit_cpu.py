"""Diverse library selection under a minimum edit distance without a GPU: the numpy restatement of the contract
(tests/select_edit_ref.py) against an independent property check, the non-vacuity of the case table that
tests/test_select_edit_gpu.py runs, and everything the two entries and their Python wrappers refuse before a device is touched."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from tests import select_edit_ref as E
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
    x, scores, min_dist = E.case(name)[:3] if name in E.CASES else S.degenerate(name)
    N = x.shape[0]
    D = E.case_distances(name, rc)
    full = E.select_of(D, scores, None, min_dist)
    assert (full[1] >= 0).all() and (full[2] >= 0).all()                      # k = None: every row has a representative
    for k in KS + (N + 5,):
        got = E.select_of(D, scores, k, min_dist)
        E.check_selection(D, scores, k, min_dist, *got)
        want = S.prefix_of(*full, N if k is None else k)                     # the prefix property
        for g, w in zip(got, want):
            assert np.array_equal(g, w), (name, k)
    E.check_selection(D, None, None, min_dist, *E.select_of(D, None, None, min_dist))      # scores = None is the given order
    # min_dist = 1: distance 0 means the rows are equal (with rc: up to the strand), whatever the metric
    for g, w in zip(E.select_of(D, scores, None, 1), S.select_ref(x, scores, None, 1, rc)):
        assert np.array_equal(g, w), name


def test_distances_are_levenshtein_distances():
    """The table against the textbook recursion on a handful of rows, the strand identity the kernel rests on, and the example of
    the README: a shifted copy is near by edit distance and far by Hamming distance."""
    rng = np.random.default_rng(0)
    a, b = rng.integers(0, 4, (5, 9)), rng.integers(0, 4, (6, 7))

    def lev(s, t):
        d = list(range(len(t) + 1))
        for i, cs in enumerate(s):
            prev, d[0] = d[0], i + 1
            for j, ct in enumerate(t):
                prev, d[j + 1] = d[j + 1], min(prev + (cs != ct), d[j] + 1, d[j + 1] + 1)
        return d[-1]
    want = np.array([[lev(s.tolist(), t.tolist()) for t in b] for s in a])
    assert np.array_equal(E.distance_matrix(a, b), want)
    assert np.array_equal(E.edit_matrix(S.revcomp(a), b), E.edit_matrix(a, S.revcomp(b)))        # lev(rc(q), db) = lev(q, rc(db))
    assert np.array_equal(E.distance_matrix(a, b, True), np.minimum(want, E.edit_matrix(a, S.revcomp(b))))
    row = rng.integers(0, 4, (1, 200))
    shifted = np.concatenate([row[:, 3:], rng.integers(0, 4, (1, 3))], 1)
    assert E.distance_matrix(row, shifted)[0, 0] <= 6 and E.hamming_matrix(row, shifted)[0, 0] > 100


@pytest.mark.parametrize("name", list(E.CASES))
def test_case_table_is_not_vacuous(name):
    """On the reference alone: each case of the shared table exercises what the kernels can get wrong."""
    x, scores, min_dist, T = E.case(name)
    N = x.shape[0]
    assert len(np.unique(scores)) < N                                         # tied scores
    rank = _rank(scores, N)
    fwd = E.case_distances(name, False)
    for rc in (False, True):
        D = E.case_distances(name, rc)
        picked, rep, _ = E.select_of(D, scores, None, min_dist)
        assert 1 < len(picked) < N, (name, rc, len(picked))
        sup = rep != np.arange(N)                                             # the suppressed rows
        same = rank[rep] // T == rank // T
        assert (sup & same).any(), (name, rc, "no row suppressed by a pick of its own block")
        assert (sup & ~same).any(), (name, rc, "no row suppressed by a pick of an earlier block")
        ham = E.hamming_matrix(x, x, rc)[np.arange(N), rep]
        assert (sup & (ham >= min_dist)).any(), (name, rc, "no row represented through an indel only")
        if rc:
            assert (sup & (fwd[np.arange(N), rep] >= min_dist)).any(), (name, "no row represented through the reverse strand only")
        to_picks = D[:, picked]
        assert (to_picks == min_dist - 1).any(), (name, rc, "no (row, pick) pair at exactly min_dist - 1")
        assert (to_picks == min_dist).any(), (name, rc, "no (row, pick) pair at exactly min_dist")
        assert not np.array_equal(picked, S.select_ref(x, scores, None, min_dist, rc)[0]), (name, rc, "the Hamming picks")


def test_kernel_references_agree_with_the_walk():
    """within_of + greedy_pick_ref composed in blocks, as the host composes the kernels, is the walk."""
    name = "odd"
    x, scores, min_dist, T = E.case(name)
    N = x.shape[0]
    for rc, k in ((False, None), (True, None), (True, 5)):
        D = E.case_distances(name, rc)
        order = S.order_of(scores, N)
        Ds = D[np.ix_(order, order)]                                          # the distances of the ranked rows
        cap = N if k is None else k
        count, picked_rank, rep_pick = 0, [], np.empty(N, np.int32)
        for r0 in range(0, N, T):
            r1 = min(r0 + T, N)
            first = S.within_of(Ds[r0:r1][:, picked_rank], min_dist - 1)[0] if picked_rank else None
            _, mask = S.within_of(Ds[r0:r1, r0:r1], min_dist - 1)
            close = ((mask[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(r1 - r0, -1)[:, :r1 - r0].astype(bool)
            rp, rows, count = S.greedy_pick_ref(close, first, cap, count, cap)
            rep_pick[r0:r1] = rp
            picked_rank += [r0 + r for r in rows]
        picked = order[np.asarray(picked_rank, np.int64)]
        rep = np.empty(N, np.int64)
        rep[order] = np.where(rep_pick >= 0, picked[np.maximum(rep_pick, 0)], -1)
        want = E.select_of(D, scores, k, min_dist)
        assert np.array_equal(picked, want[0]) and np.array_equal(rep, want[1]), (rc, k)


def test_recorded_tables_are_the_reference():
    """tests/golden/g41_select_edit.npz (the tables of the raw kernel tests that take minutes of numpy): the recorded inputs are what
    the generators give today, the cheapest tables recomputed equal the record, and the record exercises what it is there for."""
    z = np.load(E.GOLDEN)
    recorded = [L for L in E.KERNEL_LS if L >= E.GOLDEN_MIN_L]
    for L in recorded:
        for si in range(len(E.kernel_sizes(L))):
            xq, xdb = E.kernel_rows(L, si)
            assert np.array_equal(z[f"xq_{L}_{si}"], xq) and np.array_equal(z[f"xdb_{L}_{si}"], xdb), (L, si)
            assert z[f"d0_{L}_{si}"].shape == z[f"d1_{L}_{si}"].shape == (xq.shape[0], xdb.shape[0])
        assert E.kernel_case_is_not_vacuous(L) == [True] * 4, L
    L = 128                                                                   # the cheapest: 65 x 63 and 1 x 130 rows
    for si in range(len(E.kernel_sizes(L))):
        xq, xdb, D = E.kernel_case(L, si)
        for rc in (False, True):
            assert np.array_equal(E.distance_matrix(xq, xdb, rc), D[rc]), (L, si, rc)
    xq, xdb, hits = E.segment_case()                                          # asserts the inputs' record itself
    d = E.edit_matrix(xq, xdb[:1500])
    assert np.array_equal(d <= E.SEG_RADIUS, hits[:, :1500])
    assert (d == 0).any() and (d == E.SEG_RADIUS).any() and (d == E.SEG_RADIUS + 1).any()        # copies, shifts, near misses
    assert hits.any(1).sum() > E.SEG_B // 2 and hits[:, :8888].any(1).sum() > E.SEG_B // 2 and 1000 < hits.sum() < 20000


# ------------------------------------------------------------------------------------------------------ the entries ----
def test_entries_refuse_bad_arguments_without_a_device():
    from svdd_amd import _lib
    L_ = _lib.lib()
    assert _lib.ABI_VERSION == 17 and L_.svdd_abi_version() == 17
    for name, n in (("svdd_edit_within", 12), ("svdd_edit_pairs", 11)):
        sig = _lib.SIGNATURES[name]
        assert name in _lib.EXPORTS and sig[-1] is _lib.vp and _lib.STREAM not in sig and len(sig) == n
    p = [ctypes.c_void_p(4096 * (i + 1)) for i in range(6)]                   # non-NULL pointers that are never dereferenced

    def within(**kw):
        a = dict(q=p[0], db=p[1], db_count=p[2], B=3, N=70, L=20, radius=4, both_strands=1, first=p[3], mask=p[4], mask_words=3,
                 stream=None)
        a.update(kw)
        return L_.svdd_edit_within(*a.values())
    for what, kw in {"q null": dict(q=None), "db null": dict(db=None), "both outputs null": dict(first=None, mask=None),
                     "radius < 0": dict(radius=-1), "radius = L": dict(radius=20), "radius > L": dict(radius=21),
                     "L = 0": dict(L=0, radius=0), "L < 0": dict(L=-1, radius=0), "L = 1025": dict(L=1025),
                     "B = 0": dict(B=0), "N = 0": dict(N=0), "B < 0": dict(B=-2), "N < 0": dict(N=-2),
                     "mask_words too small": dict(mask_words=2), "mask_words = 0": dict(mask_words=0),
                     "mask_words < 0": dict(mask_words=-1)}.items():
        assert within(**kw) == _lib.E_ARG, what
        assert within(both_strands=0, **kw) == _lib.E_ARG, what

    def pairs(**kw):
        a = dict(q=p[0], db=p[1], idx=p[2], B=3, N=70, Lq=20, Ld=24, cap=4, both_strands=0, dist=p[3], stream=None)
        a.update(kw)
        return L_.svdd_edit_pairs(*a.values())
    for what, kw in {"q null": dict(q=None), "db null": dict(db=None), "idx null": dict(idx=None), "dist null": dict(dist=None),
                     "B = 0": dict(B=0), "N = 0": dict(N=0), "B < 0": dict(B=-1), "N < 0": dict(N=-1),
                     "Lq = 0": dict(Lq=0), "Ld = 0": dict(Ld=0), "Lq < 0": dict(Lq=-3), "Ld < 0": dict(Ld=-3),
                     "Lq = 1025": dict(Lq=1025), "Ld = 1025": dict(Ld=1025), "cap < 0": dict(cap=-1),
                     "cap > max(Lq, Ld)": dict(cap=25)}.items():
        assert pairs(**kw) == _lib.E_ARG, what
        assert pairs(both_strands=1, **kw) == _lib.E_ARG, what


# ------------------------------------------------------------------------------------------------------- the python ----
def test_wrappers_refuse_bad_arguments_before_any_launch():
    from svdd_amd import ops, quality
    x = torch.randint(0, 4, (6, 20), generator=torch.Generator().manual_seed(0))
    s = torch.rand(6, generator=torch.Generator().manual_seed(1))
    bad = x.clone()
    bad[1, 3] = 4
    for fn in (quality.select_diverse_edit, lambda t: quality.library_quality_edit(t, s[:t.shape[0]] if t.dim() == 2 else s, 2, 3),
               lambda t: quality.edit_distance(t, x), lambda t: quality.edit_distance(x, t)):
        with pytest.raises(ValueError, match="token"):
            fn(bad)                                                           # MASK has no 2-bit code
        with pytest.raises(ValueError, match="integer"):
            fn(x.float())
        with pytest.raises(ValueError, match=r"\[N, L\]"):
            fn(x[0])
        with pytest.raises(ValueError, match=r"\[N, L\]"):
            fn(x[:0])
    with pytest.raises(ValueError, match="1024"):
        quality.select_diverse_edit(torch.zeros(2, 1025, dtype=torch.uint8))
    with pytest.raises(ValueError, match="1024"):
        quality.edit_distance(x, torch.zeros(6, 1025, dtype=torch.uint8))
    with pytest.raises(ValueError, match="number of rows"):
        quality.edit_distance(x, x[:5])
    for cap in (-1, 31, 2.0, True):
        with pytest.raises(ValueError, match="cap ="):
            quality.edit_distance(x, torch.zeros(6, 30, dtype=torch.uint8), cap=cap)
    nan = s.clone()
    nan[2] = float("nan")
    for scores in (nan, nan.numpy(), s[:5], s.reshape(6, 1), torch.arange(6), [0.0] * 6):
        with pytest.raises(ValueError, match="scores"):
            quality.select_diverse_edit(x, scores)
    with pytest.raises(ValueError, match="scores"):
        quality.library_quality_edit(x, nan, 2, 3)
    with pytest.raises(ValueError, match="scores"):
        quality.library_quality_edit(x, None, 2, 3)
    for min_dist in (0, -1, 21, 2.0, True, None):
        with pytest.raises(ValueError, match="min_dist ="):
            quality.select_diverse_edit(x, s, min_dist=min_dist)
        with pytest.raises(ValueError, match="min_dist ="):
            quality.library_quality_edit(x, s, 2, min_dist)
    for k in (0, -2, 1.5, True):
        with pytest.raises(ValueError, match="k ="):
            quality.select_diverse_edit(x, s, k=k)
        with pytest.raises(ValueError, match="k ="):
            quality.library_quality_edit(x, s, k, 3)
    with pytest.raises(ValueError, match="k ="):
        quality.library_quality_edit(x, s, None, 3)                           # a library has a size
    for rows in (0, -4, 1.5, True, 4097):
        with pytest.raises(ValueError, match="block_rows ="):
            quality.select_diverse_edit(x, s, block_rows=rows)
    if not torch.cuda.is_available():
        with pytest.raises(ops.SvddError, match="GPU"):                       # valid arguments: no CPU fallback
            quality.select_diverse_edit(x, s, k=2, min_dist=3, revcomp=True, block_rows=4)
        with pytest.raises(ops.SvddError, match="GPU"):
            quality.edit_distance(x, x[:, :17], cap=5, revcomp=True)
    # the raw wrappers check their numbers first and take device tensors only
    q, m = torch.zeros(3, 2, dtype=torch.int32), torch.zeros(3, 1, dtype=torch.int32)
    f = torch.zeros(3, dtype=torch.int32)
    for L in (0, 1025, 20.0, True):
        with pytest.raises(ops.SvddError, match="L ="):
            ops.edit_within(q, q, L, 0, first=f)
    for radius in (-1, 20, 1.0, True):
        with pytest.raises(ops.SvddError, match="radius ="):
            ops.edit_within(q, q, 20, radius, first=f)
    for kw, what in ((dict(Lq=0), "Lq ="), (dict(Lq=1025), "Lq ="), (dict(Ld=0), "Ld ="), (dict(Ld=1025), "Ld ="), (dict(Ld=2.0), "Ld ="),
                     (dict(cap=-1), "cap ="), (dict(cap=21), "cap ="), (dict(cap=1.0), "cap ="), (dict(cap=True), "cap =")):
        a = dict(Lq=20, Ld=20, cap=3)
        a.update(kw)
        with pytest.raises(ops.SvddError, match=what):
            ops.edit_pairs(q, q, f, a["Lq"], a["Ld"], a["cap"])
    with pytest.raises(ops.SvddError, match="GPU"):
        ops.edit_within(q, q, 20, 3, both_strands=True, first=f, mask=m)
    with pytest.raises(ops.SvddError, match="GPU"):
        ops.edit_pairs(q, q, f, 20, 20, 3)


def test_public_signatures_and_the_flag():
    from svdd_amd import cli, ops, quality
    from svdd_amd.harness import BaseModel
    sig = lambda f: list(inspect.signature(f).parameters)                     # noqa: E731
    defaults = lambda f: {n: p.default for n, p in inspect.signature(f).parameters.items()}      # noqa: E731
    none = inspect.Parameter.empty
    # the new ones
    assert defaults(ops.edit_within) == {"q": none, "db": none, "L": none, "radius": none, "both_strands": False, "db_count": None,
                                         "first": None, "mask": None}
    assert defaults(ops.edit_pairs) == {"q": none, "db": none, "idx": none, "Lq": none, "Ld": none, "cap": none, "both_strands": False,
                                        "dist": None}
    assert defaults(quality.select_diverse_edit) == defaults(quality.select_diverse)
    assert sig(quality.library_quality_edit) == sig(quality.library_quality)
    assert defaults(quality.edit_distance) == {"a": none, "b": none, "cap": None, "revcomp": False}
    assert sig(BaseModel.select_library_edit) == sig(BaseModel.select_library)
    assert 1 <= quality.SELECT_EDIT_BLOCK_ROWS <= ops.PICK_MAX_ROWS == 4096
    # the pinned old ones are what they were
    assert sig(ops.within) == ["q", "db", "L", "radius", "q_rc", "db_count", "first", "mask"]
    assert sig(ops.greedy_pick) == ["mask", "first", "rows", "L", "base", "k", "count", "reps", "picked_rank", "rep_pick"]
    assert sig(ops.edit_nn) == ["q", "db", "Lq", "Ld", "cap", "nn_key", "hist", "q_base", "db_base", "exclude_diag"]
    assert defaults(quality.select_diverse) == {"x": none, "scores": None, "k": None, "min_dist": 1, "revcomp": False, "block_rows": None}
    assert quality.Selection._fields == ("picked", "rep", "rep_dist")
    assert sig(quality.library_quality) == ["x", "scores", "k", "min_dist", "revcomp"]
    assert sig(BaseModel.select_library) == ["self", "samples", "k", "min_dist", "revcomp"]
    assert sig(quality.sample_quality) == ["x", "refs", "train", "k", "scores", "ref_scores"]
    assert sig(quality.edit_nn) == ["x", "db", "cap", "chunk_rows", "seed_hamming"]
    # the flag: absent from the default namespace, parsed when given, refused without --select before any model is built
    assert not hasattr(cli.build_parser().parse_args([]), "select_metric")
    assert not hasattr(cli.build_parser().parse_args(["--select", "8"]), "select_metric")
    for metric in ("hamming", "edit"):
        ns = cli.build_parser().parse_args(["--select", "8", "--select_metric", metric])
        assert ns.select == 8 and ns.select_metric == metric
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["--select", "8", "--select_metric", "levenshtein"])
    for flags in (["--select_metric", "edit"], ["--select_metric", "hamming", "--select_revcomp"]):
        with pytest.raises(SystemExit):
            cli.main("mc", flags)
        with pytest.raises(ValueError, match="needs --select K"):
            cli.run(cli.build_parser().parse_args(flags))
