"""-m gpu: PWM motif scanning. Every output is an exact integer and must EQUAL tests/motif_ref.py's scan_ref.

  entry    svdd_motif_scan through the raw C entry in sentinel-guarded buffers (tests/kernel_harness.py): one case table over the
           lengths, widths, row and motif counts at which the kernel takes another path (one pass and several, one word and 64, L = w,
           L < w, fewer rows than a wave's group, more than one workgroup, more motifs than one table stage), both strands and
           forward only, every legal combination of NULL outputs; the edges of the contract (>= not >, max_score + 1, a palindrome,
           an all-negative motif, ties between starts and between strands, +-32767 over 32 columns, garbage in the padding columns
           and bits, totals added onto non-zero values)
  public   scan_counts / scan_rows for every chunking; a token 4; motif_corr, BaseModel.evaluate_motifs and --eval_motifs
"""
import itertools
import os

import numpy as np
import pytest
import torch

from svdd_amd import _lib, motifs, ops
from tests import motif_ref as R
from tests import quality_ref as Q
from tests.conftest import load_golden
from tests.kernel_harness import DEV, _Buf, _st

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "motifs_tiny.meme")
WIDTHS = (1, 2, 7, 8, 16, 17, 31, 32)
OUTPUTS = [c for c in itertools.product((True, False), repeat=4) if any(c)]      # the 15 legal (hits, rows_hit, row_hits, row_best)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _i64(init):
    init = np.asarray(init, np.int64).reshape(-1)
    b = _Buf(2 * init.size, torch.int64)
    b.body().copy_(_dev(init))
    return b


def _packed(x, dirty=False):
    """svdd_pack_tokens' rule with numpy shifts (its first rows are compared with quality_ref.pack_ref); dirty: ones in the
    padding bits of the last word, which the scan must never read as tokens."""
    N, L = x.shape
    W = (L + 15) // 16
    pad = np.zeros((N, 16 * W), np.uint32)
    pad[:, :L] = x
    out = (pad.reshape(N, W, 16) << (2 * np.arange(16, dtype=np.uint32))).sum(-1).astype(np.uint32)
    assert np.array_equal(out[:2], Q.pack_ref(x[:2])[0])
    if dirty and L % 16:
        out[:, -1] |= np.uint32(0xFFFFFFFF) << np.uint32(2 * (L % 16))
    return _dev(out.view(np.int32))


def _scan(x, ms, both, outputs=(True,) * 4, start=None, dirty=False):
    """One launch into guarded buffers -> dict of the outputs asked for (numpy); the totals start from `start` = (hits, rows_hit)."""
    N, L = x.shape
    M = len(ms.width)
    start = (np.zeros(M, np.int64),) * 2 if start is None else start
    hits = _i64(start[0]) if outputs[0] else None
    rows_hit = _i64(start[1]) if outputs[1] else None
    row_hits = _Buf(N * M, torch.int32) if outputs[2] else None
    row_best = _Buf(2 * N * M, torch.int64) if outputs[3] else None
    packed, pwm, width, thr = _packed(x, dirty), _dev(ms.pwm), _dev(ms.width), _dev(ms.threshold)
    rc = _lib.lib().svdd_motif_scan(packed.data_ptr(), N, L, pwm.data_ptr(), width.data_ptr(), thr.data_ptr(), M, int(both),
                                    *[None if b is None else b.ptr for b in (hits, rows_hit, row_hits, row_best)], _st())
    _lib.check(rc, "svdd_motif_scan")
    torch.cuda.synchronize()
    out = {}
    if hits is not None:
        hits.untouched()                                                  # the guards
        out["hits"] = hits.cpu().numpy().copy()
    if rows_hit is not None:
        rows_hit.untouched()
        out["rows_hit"] = rows_hit.cpu().numpy().copy()
    if row_hits is not None:
        row_hits.assert_written("svdd_motif_scan row_hits")
        out["row_hits"] = row_hits.cpu(N, M).numpy().copy()
    if row_best is not None:
        row_best.assert_written("svdd_motif_scan row_best")
        out["row_best"] = row_best.cpu(N, M).numpy().view(np.uint64).copy()
    return out


def _equal(got, want, start=None, what=None):
    M = want["hits"].size
    start = (np.zeros(M, np.int64),) * 2 if start is None else start
    if "hits" in got:
        assert np.array_equal(got["hits"], want["hits"] + start[0]), what
    if "rows_hit" in got:
        assert np.array_equal(got["rows_hit"], want["rows_hit"] + start[1]), what
    if "row_hits" in got:
        assert got["row_hits"].dtype == np.int32 and np.array_equal(got["row_hits"], want["row_hits"]), what
    if "row_best" in got:
        assert np.array_equal(got["row_best"], R.best_key_ref(want["best_score"], want["best_start"], want["best_strand"])), what


def _consensus(ms, m):
    return ms.pwm[m, :ms.width[m]].argmax(1)


def _random_set(widths, seed, pvalue=1e-2):
    """Random motifs of the given widths with their p = 1e-2 thresholds; a motif that cannot reach it (w <= 3: 4^-w > 1e-2) takes
    its maximum score instead, so that it can hit at all."""
    rng = np.random.default_rng(seed)
    ms = motifs.MotifSet.from_pfms([rng.dirichlet([0.6] * 4, w) for w in widths], pvalue=pvalue)
    thr = np.where(ms.reachable, ms.threshold, ms.max_score)
    return motifs.MotifSet(ms.names, ms.width, ms.pwm, thr)


def _planted(N, L, ms, seed):
    """Random rows with consensus sites at start 0 and at start L - w on each strand (L = w: at start 0 only), every motif's first
    site before any motif's second, dealt over the rows; a site that would overlap an earlier one is left out."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 4, (N, L)).astype(np.uint8)
    taken = np.zeros((N, L), bool)
    M = len(ms.width)
    for j in range(4):
        for m in range(M):
            w = int(ms.width[m])
            if w > L or (w == L and j % 2):
                continue
            site, p, r = _consensus(ms, m), (0, L - w)[j % 2], (m + j * M) % N
            if not taken[r, p:p + w].any():
                x[r, p:p + w], taken[r, p:p + w] = (site if j < 2 else R.revcomp(site)), True
    return x


#        L     N    M   first width (motif m has width WIDTHS[(first + m) % 8])
CASES = [(1, 1, 1, 0), (1, 65, 3, 0), (7, 1, 1, 2), (7, 2, 3, 1), (8, 63, 3, 2), (16, 2, 1, 4), (16, 65, 3, 3), (17, 2, 3, 5),
         (33, 1, 1, 7), (33, 2, 1, 6), (33, 257, 65, 0), (200, 1, 1, 5), (200, 65, 3, 7), (200, 63, 65, 3), (1024, 2, 3, 6),
         (1024, 65, 65, 5), (1024, 257, 3, 2)]


def test_case_table_covers_what_it_says():
    assert {c[0] for c in CASES} == {1, 7, 8, 16, 17, 33, 200, 1024} and {c[1] for c in CASES} == {1, 2, 63, 65, 257}
    assert {c[2] for c in CASES} == {1, 3, 65}
    used = {(L, WIDTHS[(f + m) % 8]) for L, N, M, f in CASES for m in range(M)}
    assert {w for _, w in used} == set(WIDTHS)
    assert {L for L, w in used if L == w} >= {1, 7, 8, 16, 17} and any(L < w for L, w in used)      # one window, and none


@pytest.mark.parametrize("both", [True, False])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_scan_equals_the_restatement(case, both):
    L, N, M, first = CASES[case]
    ms = _random_set([WIDTHS[(first + m) % 8] for m in range(M)], 100 + case)
    x = _planted(N, L, ms, 200 + case)
    want = R.scan_ref(x, ms, both)
    for m in range(M):                                                    # on the reference alone: the case proves something
        windows = N * max(L - int(ms.width[m]) + 1, 0) * (2 if both else 1)
        if windows >= 2:                                                  # non-degenerate: there can be a hit and a non-hit
            assert want["hits"][m] >= 1 and want["any_nonhit"][m], (CASES[case], both, m, int(ms.width[m]))
        if L < ms.width[m]:
            assert want["hits"][m] == 0 and (want["best_start"][:, m] == -1).all()
    start = (np.arange(M, dtype=np.int64) * 7 + 3, np.arange(M, dtype=np.int64) + (1 << 40))     # added to, not overwritten
    _equal(_scan(x, ms, both, start=start), want, start, CASES[case])
    outputs = OUTPUTS[1 + (2 * case + both) % 14]                         # and one of the other 14 combinations of outputs
    got = _scan(x, ms, both, outputs, dirty=True)
    assert sorted(got) == sorted(k for k, o in zip(("hits", "rows_hit", "row_hits", "row_best"), outputs) if o)
    _equal(got, want, None, (CASES[case], outputs))


@pytest.mark.parametrize("both", [True, False])
def test_every_combination_of_outputs(both):
    ms = _random_set([7, 32, 2], 7)
    x = _planted(65, 33, ms, 8)
    want = R.scan_ref(x, ms, both)
    assert (want["hits"] >= 1).all() and want["any_nonhit"].all()
    for outputs in OUTPUTS:
        got = _scan(x, ms, both, outputs)
        assert len(got) == sum(outputs)
        _equal(got, want, None, outputs)


def _hand_set(pwms, thresholds):
    M = len(pwms)
    pwm, width = np.zeros((M, 32, 4), np.int16), np.zeros(M, np.int32)
    for m, p in enumerate(pwms):
        p = np.asarray(p)
        width[m], pwm[m, :p.shape[0]] = p.shape[0], p
    return motifs.MotifSet([f"hand_{m}" for m in range(M)], width, pwm, thresholds)


def test_threshold_edges_palindrome_and_padding():
    tiny = motifs.load_meme(FIXTURE, pvalue=1e-2)
    at_max = motifs.MotifSet(tiny.names, tiny.width, tiny.pwm, tiny.max_score)
    x = _planted(24, 40, at_max, 1)
    want = R.scan_ref(x, at_max)
    assert (want["hits"] >= 1).all()                                      # a window AT the threshold is a hit: >=, not >
    _equal(_scan(x, at_max, True), want)
    above = motifs.MotifSet(tiny.names, tiny.width, tiny.pwm, tiny.max_score + 1)
    assert not above.reachable.any()
    want0 = R.scan_ref(x, above)
    assert want0["hits"].sum() == 0 and np.array_equal(want0["best_score"], want["best_score"])
    got0 = _scan(x, above, True)
    assert got0["hits"].sum() == 0 and got0["row_hits"].sum() == 0
    _equal(got0, want0)
    # the palindrome (motif 3): every site counts on both strands, and at one start forward wins
    fwd = R.scan_ref(x, at_max, both=False)
    assert want["hits"][3] == 2 * fwd["hits"][3] >= 2 and (want["best_strand"][:, 3] == 0).all()
    _equal(_scan(x, at_max, False), fwd)
    # garbage in the columns at and beyond each width changes nothing
    dirty = tiny.pwm.copy()
    for m, w in enumerate(tiny.width):
        dirty[m, w:] = 12345
    garbage = motifs.MotifSet(tiny.names, tiny.width, dirty, tiny.max_score)
    assert np.array_equal(garbage.max_score, tiny.max_score)
    _equal(_scan(x, garbage, True), want)


def test_best_window_ties_negative_motifs_and_the_int16_range():
    rng = np.random.default_rng(11)
    neg = -rng.integers(5, 900, (9, 4))                                   # every entry negative: every score is below zero
    big = np.full((32, 4), -32767)
    big[np.arange(32), rng.integers(0, 4, 32)] = 32767                    # +-32767 over 32 columns: no 16-bit accumulator survives
    asym = rng.integers(-300, 300, (6, 4))
    ms = _hand_set([neg, big, asym], [int(neg.max(1).sum()), 32 * 32767, int(asym.max(1).sum())])
    x = rng.integers(0, 4, (5, 70)).astype(np.uint8)
    site = _consensus(ms, 2)
    x[0, 10:16] = x[0, 40:46] = site                                      # the same best score at two starts: the lowest wins
    x[1, 20:26], x[1, 3:9] = site, R.revcomp(site)                        # forward at 20 and reverse at 3: the lowest start wins
    x[2, 0:32] = _consensus(ms, 1)                                        # 32 * 32767
    x[3, 5:37] = R.revcomp((_consensus(ms, 1) + 1) % 4)                   # reverse strand, every column -32767
    x[4, 61:70] = _consensus(ms, 0)                                       # the last window of the row
    want = R.scan_ref(x, ms)
    assert (want["best_score"][:, 0] < 0).all() and want["best_score"][4, 0] == ms.max_score[0] and want["best_start"][4, 0] == 61
    assert (want["best_start"][0, 2], want["best_strand"][0, 2]) == (10, 0) and want["row_hits"][0, 2] >= 2
    assert (want["best_start"][1, 2], want["best_strand"][1, 2]) == (3, 1)
    assert want["best_score"][2, 1] == 32 * 32767 and want["row_hits"][2, 1] == 1
    f, r = R.window_scores_ref(x, ms.pwm[1], 32)
    assert r[3, 5] == -32 * 32767 and want["best_score"][:, 1].min() > -32 * 32767
    _equal(_scan(x, ms, True), want)
    _equal(_scan(x, ms, False), R.scan_ref(x, ms, both=False))
    # a symmetric motif scores both strands alike at every start: forward wins the tie
    half = rng.integers(-200, 200, (3, 4))
    pal = _hand_set([np.concatenate([half, half[::-1, ::-1]])], [0])
    y = rng.integers(0, 4, (4, 30)).astype(np.uint8)
    wantp = R.scan_ref(y, pal)
    assert (wantp["best_strand"] == 0).all() and (wantp["row_hits"] % 2 == 0).all()
    _equal(_scan(y, pal, True), wantp)
    # the lowest possible score, as the only window
    low = _hand_set([np.where(big > 0, -32767, -32768)], [0])
    z = np.zeros((1, 32), np.uint8)
    wantl = R.scan_ref(z, low, both=False)
    assert -32 * 32768 <= wantl["best_score"][0, 0] <= -32 * 32767
    _equal(_scan(z, low, False), wantl)


# ----------------------------------------------------------------------------------------------------- the public API ----
def test_chunks_tokens_and_dtypes():
    tiny = motifs.load_meme(FIXTURE, pvalue=1e-2)
    x = _planted(130, 50, tiny, 3)
    want = R.scan_ref(x, tiny)
    for rows in (None, 1, 7, 64, 130):
        c = motifs.scan_counts(x if rows else _dev(x).long(), tiny, chunk_rows=rows)
        assert c["rows"] == 130 and c["hits"].dtype == torch.int64 and c["hits"].is_cuda
        assert np.array_equal(c["hits"].cpu().numpy(), want["hits"]) and np.array_equal(c["rows_hit"].cpu().numpy(), want["rows_hit"]), rows
        row_hits, score, start, strand = motifs.scan_rows(_dev(x), tiny, chunk_rows=rows)
        assert (row_hits.dtype, score.dtype, start.dtype, strand.dtype) == (torch.int32, torch.int32, torch.int32, torch.int8)
        for got, key in ((row_hits, "row_hits"), (score, "best_score"), (start, "best_start"), (strand, "best_strand")):
            assert np.array_equal(got.cpu().numpy(), want[key]), (rows, key)
    fwd = R.scan_ref(x, tiny, both=False)
    assert np.array_equal(motifs.scan_counts(x, tiny, strands="forward")["hits"].cpu().numpy(), fwd["hits"])
    assert np.array_equal(motifs.motif_frequencies(x, tiny), want["rows_hit"] / 130)
    assert np.array_equal(motifs.motif_frequencies(x, tiny, per="site", strands="forward"), fwd["hits"] / 130)
    short = motifs.scan_rows(x[:3, :10], tiny)                            # L < w for the two wide motifs
    assert (short[1][:, 4:] == R.INT32_MIN).all() and (short[2][:, 4:] == -1).all() and (short[3][:, 4:] == -1).all()
    assert (short[0][:, 4:] == 0).all()
    bad = _dev(x).clone()
    bad[4, 4] = 4                                                         # on the device the pack kernel's err word speaks
    for fn in (motifs.scan_counts, motifs.scan_rows, motifs.motif_frequencies):
        with pytest.raises(ops.SvddError, match="token > 3"):
            fn(bad, tiny)
    with pytest.raises(ops.SvddError, match="row_hits"):
        ops.motif_scan(ops.pack_tokens(_dev(x)), 50, tiny.to_device(DEV), row_hits=torch.zeros((130, 5), dtype=torch.int32, device=DEV))


def test_motif_corr_evaluate_motifs_and_cli(tmp_path):
    from svdd_amd import cli
    from svdd_amd.harness import BaseModel
    from svdd_amd.value_nets import RewardModel
    from tests import e2e_parity
    ms = motifs.load_meme(FIXTURE, pvalue=1e-3)
    rng = np.random.default_rng(17)
    plain, rich = rng.integers(0, 4, (96, 50)).astype(np.uint8), rng.integers(0, 4, (80, 50)).astype(np.uint8)
    for r in range(0, 80, 2):                                             # enriched for two of the motifs
        rich[r, 5:12], rich[r, 30:38] = _consensus(ms, 2), _consensus(ms, 3)
    f_plain, f_rich = R.scan_ref(plain, ms)["rows_hit"] / 96, R.scan_ref(rich, ms)["rows_hit"] / 80
    want = R.spearman_ref(f_rich, f_plain)
    assert want < 0.9 and f_rich[2] >= 0.5 and f_rich[3] >= 0.5           # on the reference: r is well below 1
    # float64 sums of six terms in another order: 1e-12 is four orders above that and far below any difference of ranks
    assert abs(motifs.motif_corr(rich, plain, ms) - want) <= 1e-12
    assert abs(motifs.motif_corr(_dev(rich), f_plain, ms) - want) <= 1e-12
    assert abs(motifs.motif_corr(rich, plain, ms, method="pearson") - R.pearson_ref(f_rich, f_plain)) <= 1e-12
    assert motifs.motif_corr(rich, rich, ms) == 1.0
    model, emb, head = e2e_parity.tiny_engine(load_golden("nets_tiny.npz"), 50, 4, DEV)
    reward = RewardModel(emb, head).to(DEV).eval()
    hm = BaseModel(emb, head, model, reward, batch_size=4, task="dna")
    refs = {"valid": plain, "freq": f_plain}
    rep = hm.evaluate_motifs([_dev(rich[:40]).long(), _dev(rich[40:]).long()], ms, refs)
    wantr = R.motif_report_ref(rich, ms, refs)
    assert sorted(rep) == sorted(wantr) == ["motif_spearman_freq", "motif_spearman_valid", "motifs_per_row_mean", "motifs_reachable"]
    assert rep["motifs_reachable"] == wantr["motifs_reachable"] == 4 and rep["motifs_per_row_mean"] == wantr["motifs_per_row_mean"] > 1
    assert abs(rep["motif_spearman_valid"] - want) <= 1e-12 and rep["motif_spearman_freq"] == rep["motif_spearman_valid"]
    sets = tmp_path / "sets.npz"
    np.savez(sets, train=plain, test=rich)
    args = ["--task", "rna", "--batch_size", "2", "--sample_M", "2", "--val_batch_num", "1", "--rng", "philox", "--out_dir", str(tmp_path)]
    path, out = cli.main("mc", args + ["--eval_quality", str(sets), "--eval_motifs", FIXTURE])
    z = np.load(path)
    new = ["motif_spearman_train", "motif_spearman_test", "motifs_per_row_mean", "motifs_reachable"]
    assert sorted(z.files) == sorted(["baseline", "decoding"] + ["quality_" + k for k in new + [
        "kmer_pearsonr_train", "kmer_pearsonr_test", "diversity_mean", "diversity_nn_median", "unique_fraction", "novelty_nn_median",
        "novelty_nn_min", "memorised_fraction", "ws_scores_train", "ws_scores_test"]])
    decoded = torch.cat([s.reshape(-1, s.shape[-1]) for s in out[0]]).cpu().numpy()
    wantc = R.motif_report_ref(decoded, motifs.load_meme(FIXTURE), {"train": plain, "test": rich})
    for k in new:
        assert abs(float(z["quality_" + k]) - wantc[k]) <= 1e-12 or (np.isnan(wantc[k]) and np.isnan(float(z["quality_" + k]))), k
