"""No GPU: PWM motif scanning.

  parser       load_meme on tests/golden/motifs_tiny.meme (six motifs of widths 1, 4, 7, 8, 17, 32: a palindrome, a header without
               nsites, a background block, a URL line ending a block) and on malformed text
  tables       integerisation equals tests/motif_ref.py; the dynamic-programming thresholds EQUAL the brute force over all 4^w
               strings for every fixture motif with w <= 8 at p = 1e-2, 1e-3, 3e-4 (no tail lies within 1e-12 of p: asserted);
               unreachable motifs; negative thresholds keep their sign
  restatement  the reverse-strand identity of scan_ref; rank-average Spearman and Pearson by hand and against scipy
  entry        svdd_motif_scan refuses every bad argument before it touches a device; ABI 17; explicit stream
  python       the wrappers refuse bad arguments before any launch; signatures; --eval_motifs
"""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

from svdd_amd import motifs
from tests import motif_ref as R

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "motifs_tiny.meme")
BG = (0.29, 0.21, 0.21, 0.29)
NSITES = (35, 50, 20, 120, 88, 412)


@pytest.fixture(scope="module")
def tiny():
    return motifs.load_meme(FIXTURE, pvalue=1e-2)


def _file_pfms():
    """The fixture's matrices read by hand: the rows of four numbers after each header."""
    out, rows = [], None
    for line in open(FIXTURE):
        cells = line.split()
        if line.startswith("letter-probability"):
            rows = []
            out.append(rows)
        elif rows is not None and len(cells) == 4 and cells[0][0].isdigit():
            rows.append([float(c) for c in cells])
        else:
            rows = None
    return [np.array(r) for r in out]


# ----------------------------------------------------------------------------------------------------- the parser ----
def test_load_meme_reads_the_fixture(tiny):
    assert tiny.names == [f"MT000{i}.1" for i in range(1, 7)] and len(tiny) == 6
    assert tiny.width.tolist() == [1, 4, 7, 8, 17, 32] and tiny.width.dtype == np.int32
    assert tiny.pwm.shape == (6, 32, 4) and tiny.pwm.dtype == np.int16 and tiny.threshold.dtype == np.int32
    pfms = _file_pfms()
    assert [p.shape[0] for p in pfms] == [1, 4, 7, 8, 17, 32]
    for m, (pfm, ns) in enumerate(zip(pfms, NSITES)):                    # the third header has no nsites: 20; the file's background
        want = R.integerise_ref(pfm, ns, BG)
        assert np.array_equal(tiny.pwm[m, :pfm.shape[0]], want), tiny.names[m]
        assert not tiny.pwm[m, pfm.shape[0]:].any()
        assert tiny.max_score[m] == want.max(1).sum() and tiny.min_score[m] == want.min(1).sum()
    pal = tiny.pwm[3, :8].astype(int)
    assert np.array_equal(pal, pal[::-1, ::-1])                           # a perfect palindrome: its own reverse complement
    text = open(FIXTURE).read()
    again = motifs.load_meme(text, pvalue=1e-2)                           # the text itself instead of a path
    assert np.array_equal(again.pwm, tiny.pwm) and np.array_equal(again.threshold, tiny.threshold)
    uniform = motifs.load_meme(FIXTURE, pvalue=1e-2, background=(0.25,) * 4, nsites=20)     # the caller's values win
    assert np.array_equal(uniform.pwm[1, :4], R.integerise_ref(pfms[1], 20.0))
    # the rows count where they disagree with w= and the block ends cleanly
    assert motifs.load_meme(text.replace("w= 7", "w= 9"), pvalue=1e-2).width.tolist() == [1, 4, 7, 8, 17, 32]


def test_load_meme_refuses_malformed_text():
    text = open(FIXTURE).read()
    lines = text.splitlines()
    row = next(i for i, l in enumerate(lines) if l.startswith("MOTIF MT0002.1")) + 3         # the second row of the width-4 motif
    short = lines[:row] + [" 0.800000  0.050000  0.150000"] + lines[row + 1:]
    with pytest.raises(ValueError, match=rf"line {row + 1}\b.*MT0002\.1"):
        motifs.load_meme("\n".join(short))
    with pytest.raises(ValueError, match=r"MT0001\.1.*alength= 20"):
        motifs.load_meme(text.replace("alength= 4 w= 1", "alength= 20 w= 1"))
    wide = "MEME version 4\n\nMOTIF wide33\nletter-probability matrix: alength= 4 w= 33 nsites= 10\n" + "0.25 0.25 0.25 0.25\n" * 33
    with pytest.raises(ValueError, match="wide33.*width 33"):
        motifs.load_meme(wide)
    neg = lines[:row] + [" 0.900000  -0.050000  0.050000  0.100000"] + lines[row + 1:]
    with pytest.raises(ValueError, match=r"MT0002\.1.*negative"):
        motifs.load_meme("\n".join(neg))
    with pytest.raises(ValueError, match="no motif"):
        motifs.load_meme("MEME version 4\n\nALPHABET= ACGT\n")
    with pytest.raises(ValueError, match="alphabet"):
        motifs.load_meme(text.replace("ALPHABET= ACGT", "ALPHABET= ACDEFGHIKLMNPQRSTVWY"))


def test_from_pfms_refuses_bad_arguments():
    ok = np.full((3, 4), 0.25)
    F = motifs.MotifSet.from_pfms
    assert F([ok]).names == ["motif_0"]
    zero = ok.copy()
    zero[1] = 0
    for bad, what in ((zero, "sums to zero"), (np.where(np.eye(3, 4) > 0, np.nan, ok), "non-finite"), (-ok, "negative"),
                      (np.full((33, 4), 0.25), "width 33"), (np.zeros((0, 4)), "width 0"), (np.ones((3, 5)), r"\[w, 4\]")):
        with pytest.raises(ValueError, match=f"motif tf.*{what}"):
            F([bad], names=["tf"])
    with pytest.raises(ValueError, match="motif tf.*outside int16"):
        F([np.array([[1.0, 0, 0, 0]])], names=["tf"], scale=1e4)          # log2(4) * 1e4 = 20000 fits, the zeros' -8.7 * 1e4 do not
    with pytest.raises(ValueError, match="motif tf.*outside int16"):
        F([np.array([[1.0, 0, 0, 0]])], names=["tf"], pseudocount=0)      # log2(0)
    for bg in ((0.5, 0.5, 0, 0), (0.25, 0.25, 0.25), (0.3, 0.3, 0.3, 0.3), (0.5, 0.6, -0.2, 0.1), (0.25, 0.25, 0.25, 0.25 + 1e-8)):
        with pytest.raises(ValueError, match="background"):
            F([ok], background=bg)
    for scale in (0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="scale"):
            F([ok], scale=scale)
    for pv in (0, 1, -0.1, 1.5):
        with pytest.raises(ValueError, match="pvalue"):
            F([ok], pvalue=pv)
    for thr in ([1, 2], [1.5], [True]):
        with pytest.raises(ValueError, match="thresholds"):
            F([ok], thresholds=thr)
    assert F([ok, ok], thresholds=[-7, 12]).threshold.tolist() == [-7, 12]
    with pytest.raises(ValueError, match="names"):
        F([ok], names=["a", "b"])


# ----------------------------------------------------------------------------------------------------- thresholds ----
@pytest.mark.parametrize("pvalue", [1e-2, 1e-3, 3e-4])
def test_thresholds_equal_the_brute_force(pvalue):
    ms = motifs.load_meme(FIXTURE, pvalue=pvalue)
    for m in range(4):                                                    # widths 1, 4, 7, 8
        w = int(ms.width[m])
        want, gap = R.threshold_brute_ref(ms.pwm[m, :w], pvalue, BG)
        assert gap > 1e-12, (ms.names[m], pvalue, gap)                    # the precondition: no tail sits on the p-value
        assert int(ms.threshold[m]) == want, (ms.names[m], pvalue)
        assert R.threshold_dp_ref(ms.pwm[m, :w], pvalue, BG) == want
    for m in (4, 5):                                                      # the wide ones against the restated DP
        w = int(ms.width[m])
        assert int(ms.threshold[m]) == R.threshold_dp_ref(ms.pwm[m, :w], pvalue, BG)


def test_unreachable_and_negative_thresholds(tiny):
    at4 = motifs.load_meme(FIXTURE, pvalue=1e-4)
    # widths 1 and 4 cannot reach 1e-4 under this background (0.21^4 = 1.9e-3): max_score + 1, never a hit
    assert at4.reachable.tolist() == [False, False, True, True, True, True]
    assert at4.threshold[:2].tolist() == (at4.max_score[:2] + 1).tolist()
    rng = np.random.default_rng(0)
    six = motifs.MotifSet.from_pfms([rng.dirichlet([0.5] * 4, 6), rng.dirichlet([0.5] * 4, 7)], pvalue=1e-4)
    assert six.reachable.tolist() == [False, True]                        # 4^-6 = 2.4e-4 > 1e-4 >= 4^-7 under the uniform background
    assert six.threshold[0] == six.max_score[0] + 1 and six.threshold[1] == six.max_score[1]
    # weak wide motifs: the 99th percentile of the score is below zero, and the sign is kept
    assert tiny.threshold[5] < 0 and tiny.threshold[4] < 0 and tiny.threshold.dtype == np.int32
    assert int(tiny.threshold[5]) == R.threshold_dp_ref(tiny.pwm[5], 1e-2, BG)
    assert tiny.reachable.tolist() == [False, True, True, True, True, True]
    low, dist = motifs.score_distribution(tiny.pwm[2, :7], np.array(BG))
    assert low == tiny.min_score[2] and low + dist.size - 1 == tiny.max_score[2] and abs(dist.sum() - 1.0) < 1e-12


# ---------------------------------------------------------------------------------------------- the restatement ----
def test_reverse_strand_identity_of_the_restatement(tiny):
    rng = np.random.default_rng(5)
    x = rng.integers(0, 4, (7, 41))
    for m in range(6):
        w = int(tiny.width[m])
        f, r = R.window_scores_ref(x, tiny.pwm[m], w)
        f_rc, r_rc = R.window_scores_ref(R.revcomp(x), tiny.pwm[m], w)
        assert np.array_equal(f_rc, r[:, ::-1]) and np.array_equal(r_rc, f[:, ::-1])
    pal = R.window_scores_ref(x, tiny.pwm[3], 8)
    assert np.array_equal(pal[0], pal[1])                                 # the palindrome scores both strands alike
    both, fwd = R.scan_ref(x, tiny), R.scan_ref(x, tiny, both=False)
    assert np.array_equal(both["hits"][3], 2 * fwd["hits"][3]) and (both["best_strand"][:, 3] == 0).all()
    short = R.scan_ref(x[:, :5], tiny)                                    # L < w: no window
    assert short["hits"][2:].sum() == 0 and (short["best_start"][:, 2:] == -1).all() and (short["best_score"][:, 2:] == R.INT32_MIN).all()
    key = R.best_key_ref([5, -3, R.INT32_MIN], [2, 0, -1], [1, 0, -1])
    assert key.tolist() == [(0x80000005 << 32) | (0xFFFFFFFF - 5), (0x7FFFFFFD << 32) | 0xFFFFFFFF, 0]


def test_spearman_and_pearson():
    nan = np.isnan
    assert motifs.rank_average([10.0, 20.0, 10.0, 30.0, 10.0]).tolist() == [2.0, 4.0, 2.0, 5.0, 2.0] == R.rank_average_ref([10, 20, 10, 30, 10])
    assert motifs.spearmanr([1, 2, 3, 4], [10, 100, 1000, 1e4]) == 1.0 and motifs.spearmanr([1, 2, 3], [3, 2, 1]) == -1.0
    a, b = [1, 2, 2, 3], [1, 3, 2, 2]                                     # ranks 1 2.5 2.5 4 / 1 4 2.5 2.5: r = 2.25 / 4.5
    assert abs(motifs.spearmanr(a, b) - 0.5) <= 1e-15 and abs(R.spearman_ref(a, b) - 0.5) <= 1e-15
    assert abs(motifs.pearsonr([1, 2, 3], [2, 4, 7]) - 5 / np.sqrt(2 * 38 / 3)) <= 1e-15
    for f in (motifs.spearmanr, motifs.pearsonr, R.spearman_ref, R.pearson_ref):
        assert nan(f([1.0], [2.0])) and nan(f([], [])) and nan(f([1, 1, 1], [1, 2, 3])) and nan(f([1, 2, 3], [5, 5, 5]))
    with pytest.raises(ValueError, match="one length"):
        motifs.spearmanr([1, 2], [1, 2, 3])
    rng = np.random.default_rng(3)
    for n in (2, 5, 64):
        a, b = rng.integers(0, 6, n) / 7.0, rng.normal(size=n)           # ties on one side
        assert abs(motifs.spearmanr(a, b) - R.spearman_ref(a, b)) <= 1e-12 or nan(R.spearman_ref(a, b))
        assert abs(motifs.pearsonr(a, b) - R.pearson_ref(a, b)) <= 1e-12 or nan(R.pearson_ref(a, b))
    assert motifs.spearmanr(torch.tensor([1.0, 2.0, 3.0]), np.array([1, 2, 4])) == 1.0


def test_spearman_and_pearson_against_scipy():
    stats = pytest.importorskip("scipy").stats
    rng = np.random.default_rng(4)
    for n in (3, 10, 200):
        a, b = rng.integers(0, 8, n).astype(float), rng.integers(0, 8, n).astype(float)
        assert abs(motifs.spearmanr(a, b) - stats.spearmanr(a, b)[0]) <= 1e-12
        assert abs(motifs.pearsonr(a, b) - stats.pearsonr(a, b)[0]) <= 1e-12


# ------------------------------------------------------------------------------------------------------ the entry ----
def test_motif_entry_refuses_bad_arguments_without_a_device():
    from svdd_amd import _lib
    L_ = _lib.lib()
    assert _lib.ABI_VERSION == 17 and L_.svdd_abi_version() == 17
    assert "svdd_motif_scan" in _lib.EXPORTS
    sig = _lib.SIGNATURES["svdd_motif_scan"]
    assert len(sig) == 13 and sig[-1] is _lib.vp and _lib.STREAM not in sig                       # the stream is the caller's
    p = [ctypes.c_void_p(4096 * (i + 1)) for i in range(8)]              # non-NULL pointers that are never dereferenced

    def scan(**kw):
        a = dict(packed=p[0], N=4, L=20, pwm=p[1], width=p[2], threshold=p[3], M=3, both=1, hits=p[4], rows_hit=p[5],
                 row_hits=p[6], row_best=p[7], stream=None)
        a.update(kw)
        return L_.svdd_motif_scan(*a.values())
    none = dict(hits=None, rows_hit=None, row_hits=None, row_best=None)
    for what, kw in {"N = 0": dict(N=0), "N < 0": dict(N=-1), "L = 0": dict(L=0), "L < 0": dict(L=-3), "L = 1025": dict(L=1025),
                     "M = 0": dict(M=0), "M < 0": dict(M=-2), "packed null": dict(packed=None), "pwm null": dict(pwm=None),
                     "width null": dict(width=None), "threshold null": dict(threshold=None), "no output": none,
                     "no output, forward": dict(none, both=0)}.items():
        assert scan(**kw) == _lib.E_ARG, what


# ----------------------------------------------------------------------------------------------------- the python ----
def test_wrappers_refuse_bad_arguments_before_any_launch(tiny):
    from svdd_amd import ops
    x = torch.randint(0, 4, (4, 20), generator=torch.Generator().manual_seed(0))
    bad = x.clone()
    bad[1, 3] = 4
    calls = (lambda t, **kw: motifs.scan_counts(t, tiny, **kw), lambda t, **kw: motifs.scan_rows(t, tiny, **kw),
             lambda t, **kw: motifs.motif_frequencies(t, tiny, **kw), lambda t, **kw: motifs.motif_corr(t, np.zeros(6), tiny, **kw))
    for fn in calls:
        with pytest.raises(ValueError, match="token"):
            fn(bad)                                                        # MASK is not a finished sequence
        with pytest.raises(ValueError, match="token"):
            fn(x.numpy() - 1)
        with pytest.raises(ValueError, match="integer"):
            fn(x.float())
        with pytest.raises(ValueError, match=r"\[N, L\]"):
            fn(x[0])
        with pytest.raises(ValueError, match="1024"):
            fn(torch.zeros(1, 1025, dtype=torch.uint8))
        with pytest.raises(ValueError, match="strands"):
            fn(x, strands="reverse")
    for fn in calls[:2]:
        for rows in (0, -4, 1.5):
            with pytest.raises(ValueError, match="chunk_rows"):
                fn(x, chunk_rows=rows)
    with pytest.raises(ValueError, match="MotifSet"):
        motifs.scan_counts(x, tiny.pwm)
    with pytest.raises(ValueError, match="per ="):
        motifs.motif_frequencies(x, tiny, per="window")
    with pytest.raises(ValueError, match="method"):
        motifs.motif_corr(x, x, tiny, method="kendall")
    if not torch.cuda.is_available():
        for fn in calls:
            with pytest.raises(ops.SvddError, match="GPU"):                # valid arguments: no CPU fallback
                fn(x)
        with pytest.raises(ops.SvddError, match="GPU"):
            tiny.to_device()
    # the raw wrapper takes device tensors only
    t = ops.MotifTables(torch.from_numpy(tiny.pwm), torch.from_numpy(tiny.width), torch.from_numpy(tiny.threshold))
    with pytest.raises(ops.SvddError, match="GPU"):
        ops.motif_scan(torch.zeros(4, 2, dtype=torch.int32), 20, t, hits=torch.zeros(6, dtype=torch.int64))
    with pytest.raises(ops.SvddError, match="outside"):
        ops.motif_scan(torch.zeros(4, 2, dtype=torch.int32), 2000, t)
    with pytest.raises(ops.SvddError, match="MotifTables"):
        ops.motif_scan(torch.zeros(4, 2, dtype=torch.int32), 20, tiny)
    score, start, strand = ops.motif_best_decode(torch.from_numpy(R.best_key_ref([5, -3, R.INT32_MIN], [2, 0, -1], [1, 0, -1]).view(np.int64)))
    assert (score.tolist(), start.tolist(), strand.tolist()) == ([5, -3, R.INT32_MIN], [2, 0, -1], [1, 0, -1])
    assert (score.dtype, start.dtype, strand.dtype) == (torch.int32, torch.int32, torch.int8)


def test_public_signatures_and_flags():
    from svdd_amd import cli, ops
    from svdd_amd.harness import BaseModel
    sig = lambda f: list(inspect.signature(f).parameters)                  # noqa: E731
    dflt = lambda f: {k: v.default for k, v in inspect.signature(f).parameters.items() if v.default is not inspect.Parameter.empty}   # noqa: E731
    assert sig(motifs.MotifSet.from_pfms) == ["pfms", "names", "nsites", "background", "pseudocount", "scale", "pvalue", "thresholds"]
    assert dflt(motifs.MotifSet.from_pfms) == dict(names=None, nsites=None, background=(0.25,) * 4, pseudocount=0.1, scale=100,
                                                   pvalue=1e-4, thresholds=None)
    assert sig(motifs.load_meme) == ["path_or_text", "from_pfms_kwargs"]
    assert sig(motifs.spearmanr) == ["a", "b"] == sig(motifs.pearsonr)
    assert sig(motifs.scan_counts) == ["x", "mset", "strands", "chunk_rows"] == sig(motifs.scan_rows)
    assert dflt(motifs.scan_counts) == dict(strands="both", chunk_rows=None) == dflt(motifs.scan_rows)
    assert sig(motifs.motif_frequencies) == ["x", "mset", "per", "strands"] and dflt(motifs.motif_frequencies) == dict(per="row", strands="both")
    assert sig(motifs.motif_corr) == ["x", "ref", "mset", "method", "per", "strands"]
    assert dflt(motifs.motif_corr) == dict(method="spearman", per="row", strands="both")
    assert sig(BaseModel.evaluate_motifs) == ["self", "samples", "mset", "refs"]
    assert sig(ops.motif_scan)[:3] == ["packed", "L", "mset_dev"] and sig(ops.motif_best_decode) == ["row_best"]
    # the flag: absent from the default namespace, present when given, refused without --eval_quality before any model is built
    assert not hasattr(cli.build_parser().parse_args([]), "eval_motifs")
    both = cli.build_parser().parse_args(["--eval_quality", "sets.npz", "--eval_motifs", "tf.meme"])
    assert both.eval_motifs == "tf.meme" and both.eval_quality == "sets.npz"
    with pytest.raises(SystemExit):
        cli.main("mc", ["--eval_motifs", FIXTURE])
    with pytest.raises(ValueError, match="--eval_quality"):
        cli.run(cli.build_parser().parse_args(["--eval_motifs", FIXTURE]))
