"""No GPU: in-silico mutagenesis and ISM-driven directed evolution.

  restatement  tests/ism_ref.py against a hand-made scorer (a per-position, per-base weight table summed over the row) whose ISM
               table and evolve trajectories are known in closed form; a constant scorer; a scorer that returns NaN
  entries      svdd_ism_mutants / svdd_ism_fold / svdd_evolve_apply refuse bad arguments before they touch a device
  python       Diffusion.ism_scores / evolve refuse a CPU tensor, a MASK token, bad positions, an unknown compare / stop
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import ism_ref as R

# score(row) = sum_l W[l, row[l]], W[l, a] = (l + 1) a for l < 5 and 100 a at l = 5: integers, exact in fp32. Position 5 is not
# among the mutated positions: it gives each row an offset of its own, so that one row can keep the batch maximum rising
# while the other already sits at its optimum.
W = np.array([[(l + 1) * a for a in range(4)] for l in range(5)] + [[100 * a for a in range(4)]], dtype=np.float32)
POS = [0, 1, 2, 3, 4]
X0 = np.array([[0, 0, 0, 0, 0, 3], [3, 3, 3, 3, 0, 0]], dtype=np.uint8)


def table_score(tok):
    tok = np.asarray(tok)
    return W[np.arange(tok.shape[1])[None, :], tok].sum(1).astype(np.float32)


def test_mutant_order_is_sequence_position_allele_without_the_reference_base():
    m = R.mutants_ref(X0, [1, 4])
    assert m.shape == (2, 6, 6)
    assert [int(m[0, i, 1]) for i in range(3)] == [1, 2, 3] and [int(m[1, i, 1]) for i in range(3)] == [0, 1, 2]
    assert [int(m[1, 3 + i, 4]) for i in range(3)] == [1, 2, 3]
    for b in range(2):
        for j, pos in enumerate([1, 4]):
            for k in range(3):
                diff = np.flatnonzero(m[b, 3 * j + k] != X0[b])
                assert diff.tolist() == [pos]
    dead = R.mutants_ref(X0, [1, 4], live=[1, 0])
    assert np.array_equal(dead[0], m[0]) and all(np.array_equal(r, X0[1]) for r in dead[1])
    assert np.array_equal(R.onehot_ref(np.array([0, 3, 4])), np.array([[1, 0, 0, 0], [0, 0, 0, 1], [0, 0, 0, 0]], np.float32))


def test_ism_table_of_the_weight_table_scorer():
    ism = R.ism_ref(X0, POS, table_score)
    base = table_score(X0)
    assert base.tolist() == [300.0, 30.0]
    for b in range(2):
        for j, pos in enumerate(POS):
            for a in range(4):
                assert ism[b, j, a] == base[b] - W[pos, X0[b, pos]] + W[pos, a], (b, j, a)
            assert ism[b, j, X0[b, pos]] == base[b]
    sub = R.ism_ref(X0, [2, 4], table_score)
    assert np.array_equal(sub, ism[:, [2, 4]])


def test_chunked_folds_give_the_one_fold():
    rng = np.random.default_rng(0)
    x = rng.integers(0, 4, (3, 9)).astype(np.uint8)
    pos = [0, 2, 3, 5, 7, 8]
    sc = rng.integers(-3, 4, (3, 18)).astype(np.float32)                   # many exact ties
    sc[0, 4] = np.nan
    sc[1, :] = np.nan
    ps = np.array([0.5, 1.5, 2.5], np.float32)
    want_ism, want_best = np.empty((3, 6, 4), np.float32), R.new_best(3)
    R.fold_ref(sc, ps, x, pos, 0, 6, want_ism, want_best)
    assert want_best[1][1] == -1 and want_best[2][1] == -1 and want_best[0][1] == -np.inf        # the all-NaN row has no pick
    for chunk in (1, 3, 4):
        ism, best = np.empty((3, 6, 4), np.float32), R.new_best(3)
        for p0 in range(0, 6, chunk):
            pc = min(chunk, 6 - p0)
            R.fold_ref(sc[:, 3 * p0:3 * (p0 + pc)], ps, x, pos, p0, pc, ism, best)
        assert ism.tobytes() == want_ism.tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(best, want_best))


def test_evolve_row_stop_climbs_and_stops_on_its_own():
    xb, sb, tr = R.evolve_ref(X0, POS, table_score, 10, "row")
    assert tr["iters"] == 6
    assert tr["position"].tolist() == [[4, 4], [3, 0], [2, -1], [1, -1], [0, -1], [0, -1]]
    assert tr["allele"].tolist() == [[3, 3], [3, 2], [3, -1], [3, -1], [3, -1], [2, -1]]
    assert tr["taken"].tolist() == [[1, 1], [1, 0], [1, 0], [1, 0], [1, 0], [0, 0]]
    assert tr["score"].tolist() == [[300, 30], [315, 45], [327, 44], [336, 45], [342, 45], [345, 45], [344, 45]]
    assert xb.tolist() == [[3, 3, 3, 3, 3, 3], [3, 3, 3, 3, 3, 0]] and sb.tolist() == [345.0, 45.0]
    # fewer iterations than the climb needs: the run ends at max_iter, nothing has stopped
    xb, sb, tr = R.evolve_ref(X0, POS, table_score, 2, "row")
    assert tr["iters"] == 2 and sb.tolist() == [327.0, 45.0] and xb[0].tolist() == [0, 0, 0, 3, 3, 3]


def test_evolve_global_stop_moves_downhill_until_the_batch_maximum_stalls():
    xb, sb, tr = R.evolve_ref(X0, POS, table_score, 10, "global")
    assert tr["iters"] == 6                                                # the stalling iteration is in the trace
    assert tr["position"].tolist() == [[4, 4], [3, 0], [2, 0], [1, 0], [0, 0], [0, 0]]
    assert tr["allele"].tolist() == [[3, 3], [3, 2], [3, 3], [3, 2], [3, 3], [2, 2]]
    assert tr["taken"].tolist() == [[1, 1]] * 5 + [[0, 0]]
    assert tr["score"].tolist() == [[300, 30], [315, 45], [327, 44], [336, 45], [342, 44], [345, 45], [344, 44]]
    assert xb.tolist() == [[3, 3, 3, 3, 3, 3], [3, 3, 3, 3, 3, 0]] and sb.tolist() == [345.0, 45.0]   # row 1: the FIRST 45
    x0, s0, tr0 = R.evolve_ref(X0, POS, table_score, 0, "global")
    assert tr0["iters"] == 0 and np.array_equal(x0, X0) and s0.tolist() == [300.0, 30.0] and tr0["score"].shape == (1, 2)


@pytest.mark.parametrize("stop", ["global", "row"])
def test_constant_scorer_stops_at_iteration_one(stop):
    const = lambda t: np.full(len(t), 2.0, np.float32)                     # noqa: E731
    xb, sb, tr = R.evolve_ref(X0, [1, 3], const, 5, stop)
    assert tr["iters"] == 1 and np.array_equal(xb, X0) and sb.tolist() == [2.0, 2.0]
    assert tr["position"].tolist() == [[1, 1]] and tr["allele"].tolist() == [[1, 0]]     # the first base that is not the row's own
    assert tr["taken"].tolist() == [[0, 0]] and tr["score"].tolist() == [[2.0, 2.0], [2.0, 2.0]]


@pytest.mark.parametrize("stop", ["global", "row"])
def test_nan_scores_are_never_selected(stop):
    def scorer(t):
        s = table_score(t)
        s[np.asarray(t)[:, 4] == 3] = np.nan                              # the best move of both rows (position 4 -> T) scores NaN
        return s
    xb, sb, tr = R.evolve_ref(X0, POS, scorer, 3, stop)
    assert not np.isnan(tr["score"]).any() and not np.isnan(sb).any() and (xb[:, 4] != 3).all()
    assert tr["position"][0].tolist() == [3, 4] and tr["allele"][0].tolist() == [3, 2]     # the next best: +12 at position 3, +10 by G
    ism = R.ism_ref(X0, POS, scorer)
    assert np.isnan(ism[:, 4, 3]).all() and not np.isnan(ism[:, :4]).any()
    allnan = lambda t: np.full(len(t), np.nan, np.float32)                 # noqa: E731
    xb, sb, tr = R.evolve_ref(X0, POS, allnan, 3, stop)
    assert tr["iters"] == 1 and tr["position"].tolist() == [[-1, -1]] and tr["taken"].tolist() == [[0, 0]] and np.array_equal(xb, X0)


def test_ism_entries_refuse_bad_arguments_without_a_device():
    from svdd_amd import _lib
    L_ = _lib.lib()
    assert _lib.ABI_VERSION == 17 and L_.svdd_abi_version() == 17
    p = [ctypes.c_void_p(4096 * (i + 1)) for i in range(16)]               # non-NULL pointers that are never dereferenced
    for name in ("svdd_ism_mutants", "svdd_ism_fold", "svdd_evolve_apply"):
        sig = _lib.SIGNATURES[name]
        assert sig[-1] is _lib.vp and sig[-1] is not _lib.STREAM          # the stream is the caller's to pass (`on_stream`)

    def mutants(**kw):
        a = dict(x=p[0], positions=p[1], live=None, B=2, L=8, P=3, cand=p[2], onehot=None, err=None, stream=None)
        a.update(kw)
        return L_.svdd_ism_mutants(*a.values())
    for what, kw in {"B = 0": dict(B=0), "B < 0": dict(B=-1), "L = 0": dict(L=0), "P = 0": dict(P=0), "P < 0": dict(P=-2),
                     "x null": dict(x=None), "positions null": dict(positions=None), "cand null": dict(cand=None),
                     "cand is x": dict(cand=p[0])}.items():
        assert mutants(**kw) == _lib.E_ARG, what

    def fold(**kw):
        a = dict(scores=p[0], slot=None, parent=p[1], x=p[2], positions=p[3], live=None, B=2, L=8, P=3, p0=0, Pc=3, ism=p[4],
                 bs=p[5], bp=p[6], ba=p[7], stream=None)
        a.update(kw)
        return L_.svdd_ism_fold(*a.values())
    for what, kw in {"B = 0": dict(B=0), "L = 0": dict(L=0), "P = 0": dict(P=0), "Pc = 0": dict(Pc=0), "p0 < 0": dict(p0=-1),
                     "chunk past P": dict(p0=1), "scores null": dict(scores=None), "parent null": dict(parent=None),
                     "x null": dict(x=None), "positions null": dict(positions=None), "no output": dict(ism=None, bs=None, bp=None, ba=None),
                     "partial best": dict(bp=None), "ism is scores": dict(ism=p[0])}.items():
        assert fold(**kw) == _lib.E_ARG, what

    def apply(**kw):
        a = dict(bs=p[0], bp=p[1], ba=p[2], B=2, L=8, stop=_lib.EVOLVE_GLOBAL, x=p[3], cur=p[4], live=p[5], bsf=p[6], stopped=p[7],
                 x_best=p[8], score_best=p[9], tp=None, ta=None, ts=None, tt=None, stream=None)
        a.update(kw)
        return L_.svdd_evolve_apply(*a.values())
    for what, kw in {"B = 0": dict(B=0), "L = 0": dict(L=0), "stop 2": dict(stop=2), "stop -1": dict(stop=-1), "x null": dict(x=None),
                     "best null": dict(bs=None), "pos null": dict(bp=None), "allele null": dict(ba=None), "cur null": dict(cur=None),
                     "best_so_far null": dict(bsf=None), "stopped null": dict(stopped=None), "x_best null": dict(x_best=None),
                     "score_best null": dict(score_best=None), "row without live": dict(stop=_lib.EVOLVE_ROW, live=None),
                     "x_best is x": dict(x_best=p[3])}.items():
        assert apply(**kw) == _lib.E_ARG, what


def _tiny():
    from svdd_amd.config import Config, ModelConfig, SamplingConfig
    from svdd_amd.diffusion import Diffusion
    torch.manual_seed(0)
    return Diffusion(Config(model=ModelConfig(hidden_dim=16, num_cnn_stacks=1, length=20), sampling=SamplingConfig(steps=4))).eval()


def test_python_entries_refuse_bad_inputs_without_a_device():
    from svdd_amd import ops
    d = _tiny()
    emb = head = lambda t: t                                               # noqa: E731  (never called)
    x = torch.randint(0, 4, (2, 20), generator=torch.Generator().manual_seed(1))
    for call in (lambda **kw: d.ism_scores(x, emb, head, **kw), lambda **kw: d.evolve(x, emb, head, **kw)):
        with pytest.raises(ops.SvddError, match="GPU"):                    # a CPU tensor: no CPU fallback
            call()
        for bad in ([3, 1], [1, 1], [0, 20], [-1, 2], []):                 # unsorted, duplicated, out of range, empty
            with pytest.raises(ValueError, match="positions"):
                call(positions=bad)
        with pytest.raises(ValueError, match="chunk_rows"):
            call(chunk_rows=0)
    xm = x.clone()
    xm[1, 3] = 4
    with pytest.raises(ops.SvddError, match="MASK"):
        d.ism_scores(xm, emb, head)
    with pytest.raises(ops.SvddError, match="MASK"):
        d.evolve(xm, emb, head)
    with pytest.raises(ValueError, match="compare"):
        d.ism_scores(x, emb, head, compare="ratio")
    with pytest.raises(ValueError, match="stop"):
        d.evolve(x, emb, head, stop="batch")
    with pytest.raises(ValueError, match="max_iter"):
        d.evolve(x, emb, head, max_iter=-1)
    with pytest.raises(ValueError):
        d.ism_scores(x[0], emb, head)


def test_harness_exposes_ism_predict_and_evolve():
    import inspect
    from svdd_amd.harness import BaseModel
    assert list(inspect.signature(BaseModel.ism_predict).parameters) == ["self", "samples", "positions", "compare"]
    assert list(inspect.signature(BaseModel.evolve).parameters) == ["self", "samples", "max_iter", "positions", "stop"]
    assert inspect.signature(BaseModel.evolve).parameters["max_iter"].default == 10
    from svdd_amd.diffusion import Diffusion
    assert list(inspect.signature(Diffusion.ism_scores).parameters) == ["self", "x", "pre_scorer_embedding", "pre_scorer_head", "reward_model",
                                                                        "positions", "compare", "chunk_rows"]
    assert list(inspect.signature(Diffusion.evolve).parameters) == ["self", "x", "pre_scorer_embedding", "pre_scorer_head", "reward_model",
                                                                    "max_iter", "positions", "stop", "chunk_rows"]
