"""No GPU: pattern scanning and pattern-driven directed evolution.

  restatement  tests/pattern_ref.py against brute force on tiny cases: a pattern that is already there gives a copy, the order is
               sequence, position, pattern, equal scores go to the first (position, pattern), a NaN never wins; a weight-table
               scorer whose trajectories are known in closed form
  entries      svdd_pattern_mutants / svdd_pattern_fold / svdd_pattern_apply are exported under ABI 17 with an explicit stream
               pointer and refuse bad arguments before they touch a device
  python       the four public functions' signatures; every ValueError / TypeError is raised without a device
  motifs       consensus_patterns on tests/golden/motifs_tiny.meme against a hand-written argmax, ties included
"""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

from tests import pattern_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))

# score(row) = sum_l W[l, row[l]] with W[l, a] = (l + 1) a for l < 8 and 100 a at l = 8: integers, exact in fp32. No start in POS lets
# a pattern reach position 8: it gives each row an offset of its own, so that row 0 keeps the batch maximum rising while row 1
# already sits at its optimum (all T on 0..7).
W = np.array([[(l + 1) * a for a in range(4)] for l in range(8)] + [[100 * a for a in range(4)]], dtype=np.float32)
X0 = np.array([[0, 1, 2, 3, 0, 1, 2, 3, 3], [3, 3, 3, 3, 3, 3, 0, 3, 0]], dtype=np.uint8)
PATTERNS = [[3], [3, 3, 3], [0, 1]]
POS = [0, 1, 2, 3, 4, 5]


def table_score(tok):
    tok = np.asarray(tok)
    return W[np.arange(tok.shape[1])[None, :], tok].sum(1).astype(np.float32)


def test_mutants_are_replacements_in_sequence_position_pattern_order():
    pos = [0, 2, 5]
    m = R.mutants_ref(X0, pos, PATTERNS)
    assert m.shape == (2, 9, 9)
    for b in range(2):
        for j, p in enumerate(pos):
            for k, pat in enumerate(PATTERNS):                                 # brute force: rebuild the row by concatenation
                want = np.concatenate([X0[b, :p], np.asarray(pat, np.uint8), X0[b, p + len(pat):]])
                assert len(want) == 9 and np.array_equal(m[b, j * 3 + k], want), (b, j, k)
    # a pattern equal to the parent's content gives a copy: row 0 holds (0, 1) at 0 and at 4, row 1 holds (3) at 0 and (0, 1) nowhere
    m = R.mutants_ref(X0, [0, 4], PATTERNS)
    assert np.array_equal(m[0, 2], X0[0]) and np.array_equal(m[0, 5], X0[0]) and np.array_equal(m[1, 0], X0[1])
    assert not np.array_equal(m[1, 2], X0[1])
    # dead rows, a pattern that does not fit, a bad parent token, a bad pattern token: copies
    dead = R.mutants_ref(X0, pos, PATTERNS, live=[1, 0])
    assert all(np.array_equal(r, X0[1]) for r in dead[1]) and np.array_equal(dead[0], R.mutants_ref(X0, pos, PATTERNS)[0])
    assert np.array_equal(R.mutants_ref(X0, [7], [[3, 3, 3]])[0, 0], X0[0])
    xb = X0.copy()
    xb[0, 7] = 4
    assert np.array_equal(R.mutants_ref(xb, [0], [[3]])[0, 0], xb[0]) and R.mutants_ref(xb, [0], [[3]])[1, 0, 0] == 3
    assert np.array_equal(R.mutants_ref(X0, [0], [[1, 4]])[0, 0], X0[0])


def test_table_of_the_weight_table_scorer_and_copies_keep_the_parents_bits():
    pos = [0, 4, 5]
    t = R.table_ref(X0, pos, PATTERNS, table_score)
    base = table_score(X0)
    for b in range(2):
        for j, p in enumerate(pos):
            for k, pat in enumerate(PATTERNS):
                want = base[b] + sum(W[p + i, a] - W[p + i, X0[b, p + i]] for i, a in enumerate(pat))
                assert t[b, j, k] == want, (b, j, k)
    # a scorer that would answer differently for a copy is never asked about one
    calls = []

    def scorer(tok):
        calls.append(np.asarray(tok).copy())
        return table_score(tok)
    R.table_ref(X0, [0, 4], PATTERNS, scorer)
    for batch in calls[1:]:
        assert not any(any(np.array_equal(r, p) for p in X0) for r in batch)


def test_fold_ties_go_to_the_first_and_a_nan_never_wins():
    K, P = 3, 4
    s = np.array([[1, 5, 5, 0, 5, 2, 1, 1, 1, 5, 0, 0],                      # the first 5 is (position 0, pattern 1)
                  [np.nan, 2, np.nan, 2, 1, 0, 0, 0, 0, 0, 0, np.nan],       # NaN in front: (0, 1) wins, not the NaN
                  [np.nan] * 12], np.float32)                                # all NaN: no pick
    parent = np.array([9, 9, 9], np.float32)
    want_t, want_b = np.empty((3, P, K), np.float32), R.new_best(3)
    R.fold_ref(s, parent, K, 0, P, want_t, want_b)
    assert want_b[1].tolist() == [0, 0, -1] and want_b[2].tolist() == [1, 1, -1]
    assert want_b[0][:2].tolist() == [5.0, 2.0] and want_b[0][2] == -np.inf
    # brute force: argmax over the non-NaN entries, the first among equals
    for b in range(2):
        flat = np.where(np.isnan(s[b]), -np.inf, s[b])
        assert int(np.argmax(flat)) == want_b[1][b] * K + want_b[2][b]
    assert np.array_equal(np.isnan(want_t), np.isnan(s.reshape(3, P, K)))
    # chunked folds give the one fold: the running best of the earlier chunks wins a tie across the border
    for chunk in (1, 2, 3):
        t, best = np.empty((3, P, K), np.float32), R.new_best(3)
        for p0 in range(0, P, chunk):
            pc = min(chunk, P - p0)
            R.fold_ref(s[:, K * p0:K * (p0 + pc)], parent, K, p0, pc, t, best)
        assert t.tobytes() == want_t.tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(best, want_b))
    # slot: -1 entries take the parent's score; a dead row offers nothing but its table is written
    slot = np.arange(36, dtype=np.int32).reshape(3, 12)
    slot[0, 1] = -1
    t, best = np.empty((3, P, K), np.float32), R.new_best(3)
    R.fold_ref(s, parent, K, 0, P, t, best, live=[1, 0, 1], slot=slot)
    assert t[0, 0, 1] == 9 and best[0][0] == 9 and (best[1][0], best[2][0]) == (0, 1) and best[1][1] == -1 and t[1, 0, 1] == 2


def test_evolve_row_stop_climbs_and_stops_on_its_own():
    """Row 0: 364, TTT at 4 (+34), TTT at 0 (+10), then nothing improves. Row 1: 87, TTT at 4 (+21; the start 5 ties and comes
    second), then its best entry is the first no-op, T at 0 with the row's own score: not strictly better, the row stops."""
    xb, sb, tr = R.evolve_patterns_ref(table_score, X0, PATTERNS, POS, 10, "row")
    assert tr["iters"] == 3
    assert tr["position"].tolist() == [[4, 4], [0, 0], [0, -1]] and tr["pattern"].tolist() == [[1, 1], [1, 0], [0, -1]]
    assert tr["taken"].tolist() == [[1, 1], [1, 0], [0, 0]]
    assert tr["score"].tolist() == [[364, 87], [398, 108], [408, 108], [408, 108]]
    assert (xb[:, :8] == 3).all() and sb.tolist() == [408.0, 108.0]
    xb, sb, tr = R.evolve_patterns_ref(table_score, X0, PATTERNS, POS, 1, "row")       # the run ends at max_iter, nothing has stopped
    assert tr["iters"] == 1 and sb.tolist() == [398.0, 108.0] and xb[0].tolist() == [0, 1, 2, 3, 3, 3, 3, 3, 3]
    x0, s0, t0 = R.evolve_patterns_ref(table_score, X0, PATTERNS, POS, 0, "row")
    assert t0["iters"] == 0 and np.array_equal(x0, X0) and t0["score"].shape == (1, 2) and t0["pattern"].shape == (0, 2)


def test_evolve_global_stop_takes_no_op_picks_until_the_batch_maximum_stalls():
    """Iteration 2: row 1 is at its optimum, its pick is the no-op T at 0 with its own score, and it is TAKEN because row 0 lifts
    the batch maximum to 408. Iteration 3 offers 408 again: the run stops, that iteration is in the trace."""
    xb, sb, tr = R.evolve_patterns_ref(table_score, X0, PATTERNS, POS, 10, "global")
    assert tr["iters"] == 3 and tr["taken"].tolist() == [[1, 1], [1, 1], [0, 0]]
    assert tr["position"].tolist() == [[4, 4], [0, 0], [0, 0]] and tr["pattern"].tolist() == [[1, 1], [1, 0], [0, 0]]
    assert tr["score"].tolist() == [[364, 87], [398, 108], [408, 108], [408, 108]]
    assert sb.tolist() == [408.0, 108.0] and (xb[:, :8] == 3).all()
    # positions None: every start at which the longest pattern fits, 0 .. L - 3 = 6; TTT at 6 would reach the offset position
    assert R.evolve_patterns_ref(table_score, X0, PATTERNS, None, 1, "global")[2]["position"].tolist() == [[4, 6]]


@pytest.mark.parametrize("stop", ["global", "row"])
def test_constant_and_nan_scorers(stop):
    const = lambda t: np.full(len(t), 2.0, np.float32)                     # noqa: E731
    xb, sb, tr = R.evolve_patterns_ref(const, X0, PATTERNS, [1, 3], 5, stop)
    assert tr["iters"] == 1 and np.array_equal(xb, X0) and tr["position"].tolist() == [[1, 1]] and tr["pattern"].tolist() == [[0, 0]]
    assert tr["taken"].tolist() == [[0, 0]]
    allnan = lambda t: np.full(len(t), np.nan, np.float32)                 # noqa: E731
    xb, sb, tr = R.evolve_patterns_ref(allnan, X0[:1], [[3]], [1, 2], 3, stop)  # no copy among the mutants: every entry is NaN
    assert tr["iters"] == 1 and tr["position"].tolist() == [[-1]] and tr["pattern"].tolist() == [[-1]] and np.array_equal(xb, X0[:1])


def test_pattern_entries_are_exported_and_refuse_bad_arguments_without_a_device():
    from svdd_amd import _lib
    L_ = _lib.lib()
    assert _lib.ABI_VERSION == 17 and L_.svdd_abi_version() == 17
    for name in ("svdd_pattern_mutants", "svdd_pattern_fold", "svdd_pattern_apply"):
        assert name in _lib.EXPORTS and hasattr(L_, name)
        sig = _lib.SIGNATURES[name]
        assert sig[-1] is _lib.vp and sig[-1] is not _lib.STREAM          # the stream is the caller's to pass (`on_stream`)
    assert _lib.PATTERN_MAX_WIDTH == 32
    p = [ctypes.c_void_p(4096 * (i + 1)) for i in range(16)]               # non-NULL pointers that are never dereferenced

    def mutants(**kw):
        a = dict(x=p[0], positions=p[1], patterns=p[2], widths=p[3], live=None, B=2, L=8, P=3, K=2, cand=p[4], onehot=None,
                 err=None, stream=None)
        a.update(kw)
        return L_.svdd_pattern_mutants(*a.values())
    for what, kw in {"B = 0": dict(B=0), "L = 0": dict(L=0), "P = 0": dict(P=0), "K = 0": dict(K=0), "K < 0": dict(K=-1),
                     "x null": dict(x=None), "positions null": dict(positions=None), "patterns null": dict(patterns=None),
                     "widths null": dict(widths=None), "cand null": dict(cand=None), "cand is x": dict(cand=p[0]),
                     "patterns misaligned": dict(patterns=ctypes.c_void_p(4097)), "P K too large": dict(P=1 << 20, K=1 << 11)}.items():
        assert mutants(**kw) == _lib.E_ARG, what

    def fold(**kw):
        a = dict(scores=p[0], slot=None, parent=p[1], live=None, B=2, P=3, K=2, p0=0, Pc=3, table=p[4], bs=p[5], bp=p[6], bk=p[7],
                 stream=None)
        a.update(kw)
        return L_.svdd_pattern_fold(*a.values())
    for what, kw in {"B = 0": dict(B=0), "P = 0": dict(P=0), "K = 0": dict(K=0), "Pc = 0": dict(Pc=0), "p0 < 0": dict(p0=-1),
                     "chunk past P": dict(p0=1), "scores null": dict(scores=None), "parent null": dict(parent=None),
                     "no output": dict(table=None, bs=None, bp=None, bk=None), "partial best": dict(bk=None),
                     "table is scores": dict(table=p[0])}.items():
        assert fold(**kw) == _lib.E_ARG, what

    def apply(**kw):
        a = dict(bs=p[0], bp=p[1], bk=p[2], positions=p[10], patterns=p[11], widths=p[12], B=2, L=8, P=3, K=2, stop=_lib.EVOLVE_GLOBAL,
                 x=p[3], cur=p[4], live=p[5], bsf=p[6], stopped=p[7], x_best=p[8], score_best=p[9], tp=None, tk=None, ts=None, tt=None,
                 stream=None)
        a.update(kw)
        return L_.svdd_pattern_apply(*a.values())
    for what, kw in {"B = 0": dict(B=0), "L = 0": dict(L=0), "P = 0": dict(P=0), "K = 0": dict(K=0), "stop 2": dict(stop=2),
                     "x null": dict(x=None), "best null": dict(bs=None), "pos null": dict(bp=None), "pattern null": dict(bk=None),
                     "positions null": dict(positions=None), "patterns null": dict(patterns=None), "widths null": dict(widths=None),
                     "cur null": dict(cur=None), "best_so_far null": dict(bsf=None), "stopped null": dict(stopped=None),
                     "x_best null": dict(x_best=None), "score_best null": dict(score_best=None),
                     "row without live": dict(stop=_lib.EVOLVE_ROW, live=None), "x_best is x": dict(x_best=p[3])}.items():
        assert apply(**kw) == _lib.E_ARG, what


def test_public_signatures_are_pinned():
    from svdd_amd.diffusion import Diffusion
    from svdd_amd.harness import BaseModel

    def names(f):
        return list(inspect.signature(f).parameters)

    def defaults(f):
        return {k: v.default for k, v in inspect.signature(f).parameters.items() if v.default is not inspect.Parameter.empty}
    assert names(Diffusion.pattern_scores) == ["self", "x", "patterns", "pre_scorer_embedding", "pre_scorer_head", "reward_model",
                                               "positions", "compare", "chunk_rows"]
    assert defaults(Diffusion.pattern_scores) == dict(reward_model=None, positions=None, compare=None, chunk_rows=None)
    assert names(Diffusion.evolve_patterns) == ["self", "x", "patterns", "pre_scorer_embedding", "pre_scorer_head", "reward_model",
                                                "max_iter", "positions", "stop", "chunk_rows"]
    assert defaults(Diffusion.evolve_patterns) == dict(reward_model=None, max_iter=10, positions=None, stop="global", chunk_rows=None)
    assert names(BaseModel.pattern_scan) == ["self", "samples", "patterns", "positions", "compare"]
    assert defaults(BaseModel.pattern_scan) == dict(positions=None, compare=None)
    assert names(BaseModel.evolve_patterns) == ["self", "samples", "patterns", "max_iter", "positions", "stop"]
    assert defaults(BaseModel.evolve_patterns) == dict(max_iter=10, positions=None, stop="global")


def _tiny():
    from svdd_amd.config import Config, ModelConfig, SamplingConfig
    from svdd_amd.diffusion import Diffusion
    torch.manual_seed(0)
    return Diffusion(Config(model=ModelConfig(hidden_dim=16, num_cnn_stacks=1, length=40), sampling=SamplingConfig(steps=4))).eval()


def test_python_entries_refuse_bad_inputs_without_a_device():
    from svdd_amd import motifs, ops
    d = _tiny()
    emb = head = lambda t: t                                               # noqa: E731  (never called)
    x = torch.randint(0, 4, (2, 40), generator=torch.Generator().manual_seed(1))
    ok = ["ACGT", [0, 1, 2]]
    for call in (lambda pats=ok, **kw: d.pattern_scores(x, pats, emb, head, **kw),
                 lambda pats=ok, **kw: d.evolve_patterns(x, pats, emb, head, **kw)):
        with pytest.raises(ops.SvddError, match="GPU"):                    # a CPU tensor: no CPU fallback
            call()
        with pytest.raises(ops.SvddError, match="GPU"):
            call([np.array([0, 3], np.uint8), torch.tensor([1, 2]), "T" * 32], positions=[0, 8])
        for bad in ([], [""], ["ACGT", []], ["A" * 33], [list(range(4)) * 9], ["ACGU"], ["acgt"], [[0, 4]], [[-1]], [[0.5, 1.0]],
                    "ACGT", [[[0, 1]]], None):
            with pytest.raises(ValueError, match="pattern"):
                call(bad)
        for bad in ([3, 1], [1, 1], [0, 37], [-1, 2], []):                 # unsorted, duplicated, the 4-wide pattern leaves the row, empty
            with pytest.raises(ValueError, match="positions"):
                call(positions=bad)
        with pytest.raises(ops.SvddError, match="GPU"):                    # 36 + 4 = L: accepted, refused only for the device
            call(positions=[0, 36])
        with pytest.raises(ValueError, match="positions"):                 # 9 + 32 > L: the LONGEST pattern decides
            call(["A" * 32, "ACGT"], positions=[9])
        with pytest.raises(ValueError, match="chunk_rows"):
            call(chunk_rows=0)
        guided = object.__new__(motifs.GuidedReward)                       # never run: the refusal looks at the type alone
        with pytest.raises(TypeError, match="GuidedReward"):
            call(reward_model=guided)
    for f in (d.pattern_scores, d.evolve_patterns):
        with pytest.raises(ValueError, match=r"\[B, L\]"):
            f(x[0], ok, emb, head)
        with pytest.raises(ValueError, match="fit into the sequence"):
            f(x[:, :20], ["A" * 32], emb, head)
    xm = x.clone()
    xm[1, 3] = 4
    with pytest.raises(ops.SvddError, match="MASK"):
        d.pattern_scores(xm, ok, emb, head)
    with pytest.raises(ops.SvddError, match="MASK"):
        d.evolve_patterns(xm, ok, emb, head)
    with pytest.raises(ValueError, match="compare"):
        d.pattern_scores(x, ok, emb, head, compare="ratio")
    with pytest.raises(ValueError, match="stop"):
        d.evolve_patterns(x, ok, emb, head, stop="batch")
    with pytest.raises(ValueError, match="max_iter"):
        d.evolve_patterns(x, ok, emb, head, max_iter=-1)


def test_pattern_list_packs_strings_and_token_sequences():
    from svdd_amd.diffusion import Diffusion
    pat, w = Diffusion._pattern_list(["ACGT", [3, 2], np.array([1], np.uint8), torch.tensor([0] * 32)])
    assert pat.shape == (4, 32) and pat.dtype == np.uint8 and w.tolist() == [4, 2, 1, 32] and w.dtype == np.int32
    assert pat[0, :5].tolist() == [0, 1, 2, 3, 0] and pat[1, :3].tolist() == [3, 2, 0] and pat[2, 0] == 1 and not pat[3].any()


def test_consensus_patterns_against_a_hand_written_argmax():
    from svdd_amd import motifs
    mset = motifs.load_meme(os.path.join(HERE, "golden", "motifs_tiny.meme"))
    got = motifs.consensus_patterns(mset)
    assert len(got) == len(mset) == 6 and [len(g) for g in got] == [1, 4, 7, 8, 17, 32] and all(g.dtype == np.uint8 for g in got)
    for m, g in enumerate(got):
        total = 0
        for c in range(int(mset.width[m])):
            best = 0
            for a in range(1, 4):                                              # strictly greater: the lowest base among ties
                if mset.pwm[m, c, a] > mset.pwm[m, c, best]:
                    best = a
            assert g[c] == best, (m, c)
            total += int(mset.pwm[m, c, best])
        assert total == mset.max_score[m]                                      # the consensus is the motif's best window
    assert "".join("ACGT"[t] for t in got[1]) == "GATA" and "".join("ACGT"[t] for t in got[3]) == "GCGCGCGC"
    sub = motifs.consensus_patterns(mset, [mset.names[3], mset.names[1]])
    assert [s.tolist() for s in sub] == [got[3].tolist(), got[1].tolist()]
    assert motifs.consensus_patterns(mset, mset.names[0])[0].tolist() == got[0].tolist()
    with pytest.raises(ValueError, match="no motif named"):
        motifs.consensus_patterns(mset, ["nope"])
    with pytest.raises(ValueError, match="MotifSet"):
        motifs.consensus_patterns("GATA")
    # ties: equal entries in a column go to the lowest base (uniform background: equal frequencies are equal log-odds)
    tied = motifs.MotifSet.from_pfms([np.array([[0.25, 0.25, 0.25, 0.25], [0.1, 0.4, 0.4, 0.1], [0.1, 0.1, 0.4, 0.4], [0.0, 0.0, 0.0, 1.0]])],
                                     names=["tied"], thresholds=[0])
    assert tied.pwm[0, 1, 1] == tied.pwm[0, 1, 2] and motifs.consensus_patterns(tied)[0].tolist() == [0, 1, 2, 3]
