"""No GPU: edit-distance novelty.

  restatement  tests/edit_ref.py equals a three-line dynamic programme on random pairs (alphabets of 1, 2 and 4 letters, unequal
               lengths, nothing in common); cap, bases, diagonal, first-wins key, every cut of the database
  entry        svdd_edit_nn refuses bad arguments before it touches a device; explicit stream
  python       the wrappers refuse bad arguments before any launch; signatures; --eval_edit
  report       edit_quality_ref on planted shifted copies: what Hamming distance misses
"""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from tests import edit_ref as E
from tests import quality_ref as Q


def _dp(a, b):
    prev = list(range(len(b) + 1))
    for i, ca in enumerate(a, 1):
        cur = [i]
        for j, cb in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (ca != cb)))
        prev = cur
    return prev[-1]


def shifted(row, s, rng):
    """row moved left by s positions, the freed end filled at random."""
    return np.concatenate([row[s:], rng.integers(0, 4, s).astype(row.dtype)])


# ------------------------------------------------------------------------------------------------ the restatement ----
def test_restated_distance_equals_the_plain_programme():
    rng = np.random.default_rng(0)
    pairs = 0
    for hi in (1, 2, 4):
        for m, n in ((1, 1), (1, 7), (7, 1), (5, 5), (31, 33), (33, 31), (32, 32), (40, 17), (17, 40), (65, 64)):
            xq = rng.integers(0, hi, (4, m)).astype(np.uint8)
            xdb = rng.integers(0, hi, (5, n)).astype(np.uint8)
            if m == n and m > 4:
                xdb[1] = shifted(xq[2], 2, rng) % hi                          # a near pair among the far ones
            d = E.edit_matrix(xq, xdb)
            for i in range(4):
                for j in range(5):
                    assert d[i, j] == _dp(xq[i].tolist(), xdb[j].tolist()), (hi, m, n, i, j)
                    pairs += 1
            if hi == 1:
                assert (d == abs(m - n)).all()                                # one letter: only the lengths differ
    assert pairs >= 300
    a, c = np.zeros((1, 9), np.uint8), np.ones((1, 12), np.uint8)             # nothing in common: max(m, n)
    assert E.edit_matrix(a, c)[0, 0] == 12 and E.edit_matrix(c, a)[0, 0] == 12
    x = rng.integers(0, 4, (1, 200)).astype(np.uint8)                         # the issue's example: a shift by 3 is 6 edits
    y = shifted(x[0], 3, rng)[None]
    assert E.edit_matrix(x, y)[0, 0] == 6 and Q.hamming_matrix(x, y)[0, 0] > 100


def test_restated_key_hist_cap_and_cuts():
    rng = np.random.default_rng(1)
    x = rng.integers(0, 4, (5, 20)).astype(np.uint8)
    db = rng.integers(0, 4, (12, 22)).astype(np.uint8)
    db[7, :20] = db[3, :20] = x[2]                                            # two rows 2 insertions from query 2: the lower wins
    d = E.edit_matrix(x, db)
    assert d[2, 3] == 2 == d[2, 7]
    for cap in (0, 1, 2, 5, 22):
        key, hist = E.edit_nn_ref(x, db, cap)
        dist, idx = Q.nn_decode_ref(key)
        assert hist.shape == (cap + 2,) and hist.sum() == 5 * 12 and hist[cap + 1] == (d > cap).sum()
        assert np.array_equal(hist[:cap + 1], np.bincount(d[d <= cap], minlength=cap + 1))
        assert (dist[2], idx[2]) == ((2, 3) if cap >= 2 else (-1, -1))
        for i in range(5):
            near = np.flatnonzero(d[i] <= cap)
            assert (dist[i], idx[i]) == ((d[i].min(), int(np.flatnonzero(d[i] == d[i].min())[0])) if near.size else (-1, -1))
        key2, hist2 = None, None
        for r0 in (8, 0, 4):                                                  # any order of the chunks, the key carried along
            key2, hist2 = E.edit_nn_ref(x, db[r0:r0 + 4], cap, db_base=r0, nn_key=key2, hist=hist2)
        assert np.array_equal(key, key2) and np.array_equal(hist, hist2)
        assert np.array_equal(E.edit_hist_ref(x, db, cap), hist)
    key, hist = E.edit_nn_ref(x[:1], x[:1], 20, exclude_diag=True)
    assert Q.nn_decode_ref(key) == (-1, -1) and hist.sum() == 0
    rep = np.stack([x[0]] * 3)
    dist, idx = Q.nn_decode_ref(E.edit_nn_ref(rep, rep, 0, exclude_diag=True)[0])
    assert dist.tolist() == [0, 0, 0] and idx.tolist() == [1, 0, 0]
    key, _ = E.edit_nn_ref(x, db, 22, q_base=3, db_base=1, exclude_diag=True)  # the diagonal follows the bases: (i, j) with 3 + i == 1 + j
    want = d.copy()
    for i in range(5):
        want[i, i + 2] = 99
    assert np.array_equal(Q.nn_decode_ref(key)[0], want.min(1)) and np.array_equal(Q.nn_decode_ref(key)[1], 1 + want.argmin(1))


def test_restated_report_sees_what_hamming_misses():
    rng = np.random.default_rng(2)
    train = rng.integers(0, 4, (30, 60)).astype(np.uint8)
    x = rng.integers(0, 4, (8, 60)).astype(np.uint8)
    for n, s in enumerate((1, 2, 3)):
        x[2 * n] = shifted(train[5 * n + 1], s, rng)                          # three of eight designs are shifted training rows
    x[7] = shifted(x[6], 1, rng)                                              # and one is a shifted copy of another design
    rep = E.edit_quality_ref(x, 6, train)
    assert rep == {"edit_near_batch_fraction": 2 / 8, "edit_near_train_fraction": 3 / 8, "edit_near_train_min": 2,
                   "hamming_missed_fraction": 3 / 8}
    ham = Q.sample_quality_ref(x, train=train)
    assert ham["memorised_fraction"] == 0.0 and ham["novelty_nn_min"] > 6     # the Hamming report calls all eight novel
    assert E.edit_quality_ref(x, 1, train)["edit_near_train_min"] == -1       # nothing within one edit
    assert sorted(E.edit_quality_ref(x, 6)) == ["edit_near_batch_fraction"]
    assert "hamming_missed_fraction" not in E.edit_quality_ref(x, 6, train[:, :50])


# ------------------------------------------------------------------------------------------------------ the entry ----
def test_edit_entry_refuses_bad_arguments_without_a_device():
    from svdd_amd import _lib
    L_ = _lib.lib()
    assert _lib.ABI_VERSION == 17 and L_.svdd_abi_version() == 17 and "svdd_edit_nn" in _lib.EXPORTS
    sig = _lib.SIGNATURES["svdd_edit_nn"]
    assert sig[-1] is _lib.vp and _lib.STREAM not in sig and len(sig) == 13   # the stream is the caller's (`on_stream`)
    p = [ctypes.c_void_p(4096 * (i + 1)) for i in range(4)]                   # non-NULL pointers that are never dereferenced

    def nn(**kw):
        a = dict(q=p[0], db=p[1], B=3, N=5, Lq=20, Ld=30, cap=4, q_base=0, db_base=0, exclude_diag=0, nn_key=p[2], hist=p[3], stream=None)
        a.update(kw)
        return L_.svdd_edit_nn(*a.values())
    top = (1 << 31) - 1
    for what, kw in {"B = 0": dict(B=0), "B < 0": dict(B=-1), "N = 0": dict(N=0), "N < 0": dict(N=-1), "Lq = 0": dict(Lq=0),
                     "Ld = 0": dict(Ld=0), "Lq < 0": dict(Lq=-1), "Ld < 0": dict(Ld=-3), "Lq = 1025": dict(Lq=1025),
                     "Ld = 1025": dict(Ld=1025), "cap < 0": dict(cap=-1), "cap > max L": dict(cap=31),
                     "cap > max L, Lq longer": dict(Lq=40, cap=41), "q_base < 0": dict(q_base=-1), "db_base < 0": dict(db_base=-1),
                     "db_base + N = 2^31": dict(db_base=top - 4), "q_base + B = 2^31": dict(q_base=top - 2),
                     "db_base + N > 2^31": dict(db_base=top), "q null": dict(q=None), "db null": dict(db=None),
                     "neither output": dict(nn_key=None, hist=None)}.items():
        assert nn(**kw) == _lib.E_ARG, what


# ------------------------------------------------------------------------------------------------------- the python ----
def test_wrappers_refuse_bad_arguments_before_any_launch():
    from svdd_amd import ops, quality
    x = torch.randint(0, 4, (4, 20), generator=torch.Generator().manual_seed(0))
    bad = x.clone()
    bad[1, 3] = 4
    for fn in (quality.edit_nn, quality.pairwise_edit_hist, lambda t: quality.edit_quality(t, 3)):
        with pytest.raises(ValueError, match="token"):
            fn(bad)                                                           # MASK has no 2-bit code
        with pytest.raises(ValueError, match="integer"):
            fn(x.float())
        with pytest.raises(ValueError, match=r"\[N, L\]"):
            fn(x[0])
        with pytest.raises(ValueError, match=r"\[N, L\]"):
            fn(x[:0])
    with pytest.raises(ValueError, match="token"):
        quality.edit_nn(x, bad)
    with pytest.raises(ValueError, match="token"):
        quality.edit_quality(x, 3, train=bad)
    with pytest.raises(ValueError, match="1024"):
        quality.edit_nn(x, torch.zeros(1, 1025, dtype=torch.uint8))
    for cap in (-1, 21, 2.0, True):
        with pytest.raises(ValueError, match="cap ="):
            quality.edit_nn(x, cap=cap)
        with pytest.raises(ValueError, match="cap ="):
            quality.pairwise_edit_hist(x, cap=cap)
        with pytest.raises(ValueError, match="edit_cap ="):
            quality.edit_quality(x, cap)
    with pytest.raises(ValueError, match="cap ="):
        quality.edit_nn(x, x[:, :10], cap=21)                                 # the longer side bounds the cap ...
    with pytest.raises(ValueError, match="edit_cap ="):
        quality.edit_quality(x, None)                                         # the report has no default reach
    for rows in (0, -4, 1.5):
        with pytest.raises(ValueError, match="chunk_rows"):
            quality.edit_nn(x, chunk_rows=rows)
    if not torch.cuda.is_available():
        with pytest.raises(ops.SvddError, match="GPU"):                       # valid arguments: no CPU fallback
            quality.edit_nn(x)
        with pytest.raises(ops.SvddError, match="GPU"):
            quality.edit_nn(x, torch.zeros(3, 30, dtype=torch.uint8), cap=30)  # ... here the database
    # the raw wrapper takes device tensors only
    q, db = torch.zeros(2, 2, dtype=torch.int32), torch.zeros(2, 3, dtype=torch.int32)
    with pytest.raises(ops.SvddError, match="GPU"):
        ops.edit_nn(q, db, 20, 40, 5, hist=torch.zeros(7, dtype=torch.int64))
    with pytest.raises(ops.SvddError, match="outside"):
        ops.edit_nn(q, db, 2000, 40, 5)
    with pytest.raises(ops.SvddError, match="outside"):
        ops.edit_nn(q, db, 20, 0, 5)
    for cap in (-1, 41, 3.0):
        with pytest.raises(ops.SvddError, match="cap ="):
            ops.edit_nn(q, db, 20, 40, cap)


def test_public_signatures_and_the_flag():
    from svdd_amd import cli, ops, quality
    from svdd_amd.harness import BaseModel
    sig = lambda f: list(inspect.signature(f).parameters)                     # noqa: E731
    assert sig(ops.edit_nn) == ["q", "db", "Lq", "Ld", "cap", "nn_key", "hist", "q_base", "db_base", "exclude_diag"]
    assert sig(quality.edit_nn) == ["x", "db", "cap", "chunk_rows", "seed_hamming"]
    assert inspect.signature(quality.edit_nn).parameters["seed_hamming"].default is True
    assert sig(quality.pairwise_edit_hist) == ["x", "db", "cap"]
    assert sig(quality.edit_quality) == ["x", "edit_cap", "train"]
    assert sig(BaseModel.evaluate_edit) == ["self", "samples", "edit_cap", "train"]
    # the flag: absent from the default namespace, present when given, refused without --eval_quality before any model is built
    assert not hasattr(cli.build_parser().parse_args([]), "eval_edit")
    both = cli.build_parser().parse_args(["--eval_quality", "sets.npz", "--eval_edit", "6"])
    assert both.eval_edit == 6 and both.eval_quality == "sets.npz"
    with pytest.raises(SystemExit):
        cli.main("mc", ["--eval_edit", "6"])
    with pytest.raises(ValueError, match="--eval_edit needs --eval_quality"):
        cli.run(cli.build_parser().parse_args(["--eval_edit", "6"]))
