"""-m gpu: sample-quality metrics. Everything here is an exact integer and must EQUAL tests/quality_ref.py.

  kernels    svdd_kmer_counts / svdd_pack_tokens / svdd_hamming_nn through the raw C entries in sentinel-guarded buffers
             (tests/kernel_harness.py): every shape at which the code takes another path (k > L, one row, more rows than one
             workgroup takes, every word-count bucket of the Hamming kernel, one and several tiles and segments), accumulation into
             non-zero outputs, every chunking of rows, queries and database
  public     sample_quality on g40's sets against the recorded r (1e-10) and the restatement's integers; duplicates; the harness
"""
import numpy as np
import pytest
import torch

from svdd_amd import _lib
from tests import quality_ref as Q
from tests.conftest import load_golden
from tests.kernel_harness import DEV, _Buf, _st

pytestmark = pytest.mark.gpu
BAR = 1e-10                                # tests/test_quality_cpu.py: the bar of the recorded float64 values


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _i64(init):
    """A guarded i64 buffer holding `init` (the accumulated-into outputs start from the caller's values)."""
    init = np.asarray(init, np.int64).reshape(-1)
    b = _Buf(2 * init.size, torch.int64)
    b.body().copy_(_dev(init))
    return b


def _tokens(N, L, seed, hi=4):
    return np.random.default_rng(seed).integers(0, hi, (N, L)).astype(np.uint8)


# ---------------------------------------------------------------------------------------------- svdd_kmer_counts ----
def _kmer(x, k, counts, skipped):
    """One launch into the guarded accumulators (skipped may be None)."""
    xd = _dev(x)
    rc = _lib.lib().svdd_kmer_counts(xd.data_ptr(), x.shape[0], x.shape[1], k, counts.ptr, None if skipped is None else skipped.ptr, _st())
    _lib.check(rc, "svdd_kmer_counts")
    torch.cuda.synchronize()
    counts.untouched(), skipped is None or skipped.untouched()            # the guards
    return counts.cpu().numpy().copy(), None if skipped is None else int(skipped.cpu()[0])


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6])
def test_kmer_counts_equal_the_restatement(k):
    for L in (1, 2, 5, 6, 7, 50, 200):
        for N in (1, 3, 257):
            x = _tokens(N, L, 100 * k + L + N)
            if L >= 3:
                x[0, 0] = 4                                               # MASK at the first,
                x[N // 2, L - 1] = 4                                      # the last
                x[N - 1, L // 2] = 4                                      # and an interior position
            start = np.arange(4 ** k, dtype=np.int64) * 3 + 1            # added to, not overwritten
            got, skipped = _kmer(x, k, _i64(start), _i64([5]))
            want, want_skipped = Q.kmer_counts_ref(x, k, start, 5)
            assert np.array_equal(got, want), (k, L, N)
            assert skipped == want_skipped, (k, L, N)
            if k > L:
                assert np.array_equal(got, start) and skipped == 5       # no windows: nothing written
            else:
                assert got.sum() - start.sum() + skipped - 5 == N * (L - k + 1)


def test_kmer_counts_do_not_depend_on_the_chunking():
    x = _tokens(257, 50, 7, hi=5)                                         # MASK tokens all over
    want, want_skipped = Q.kmer_counts_ref(x, 3)
    assert want_skipped > 0
    for rows in (257, 1, 7, 64):
        counts, skipped = _i64(np.zeros(64)), _i64([0])
        for r0 in range(0, 257, rows):
            got, sk = _kmer(x[r0:r0 + rows], 3, counts, skipped)
        assert np.array_equal(got, want) and sk == want_skipped, rows
    got, sk = _kmer(x, 3, _i64(np.zeros(64)), None)                       # skipped is optional
    assert np.array_equal(got, want) and sk is None


# ---------------------------------------------------------------------------------------------- svdd_pack_tokens ----
def _pack(x, err_start=0):
    xd = _dev(x)
    N, L = x.shape
    W = (L + 15) // 16
    out, err = _Buf(N * W, torch.int32), _Buf(1, torch.int32)
    err.body().fill_(err_start)
    rc = _lib.lib().svdd_pack_tokens(xd.data_ptr(), N, L, out.ptr, err.ptr, _st())
    _lib.check(rc, "svdd_pack_tokens")
    torch.cuda.synchronize()
    out.assert_written("svdd_pack_tokens packed")
    err.untouched()
    return out.cpu(N, W).numpy().view(np.uint32), int(err.cpu()[0])


@pytest.mark.parametrize("L", [1, 15, 16, 17, 33, 200, 1024])
def test_pack_tokens_equal_the_restatement(L):
    x = _tokens(5, L, L)
    x[:, -1] = 3                                                          # the last valid position has both bits set
    got, err = _pack(x, err_start=0)
    want, _ = Q.pack_ref(x)
    assert np.array_equal(got, want) and err == 0
    if L % 16:
        assert (got[:, -1] >> np.uint32(2 * (L % 16)) == 0).all()         # padding bits are zero
    assert _pack(x, err_start=7)[1] == 7                                  # the err word is untouched by clean rows
    bad = x.copy()
    bad[3, L // 2] = 4
    got, err = _pack(bad)
    want, want_err = Q.pack_ref(bad)
    assert np.array_equal(got, want) and err == 1 == want_err             # a token 4 packs as 0 and sets the word


def test_pack_tokens_without_an_err_word():
    x = _tokens(3, 20, 0)
    x[1, 4] = 4
    xd = _dev(x)
    out = _Buf(3 * 2, torch.int32)
    _lib.check(_lib.lib().svdd_pack_tokens(xd.data_ptr(), 3, 20, out.ptr, None, _st()), "svdd_pack_tokens")
    torch.cuda.synchronize()
    out.assert_written("svdd_pack_tokens packed")
    assert np.array_equal(out.cpu(3, 2).numpy().view(np.uint32), Q.pack_ref(x)[0])


# ----------------------------------------------------------------------------------------------- svdd_hamming_nn ----
def _packed(x):
    """pack_ref's rule with numpy shifts (pack_ref itself loops over every token; its first rows are compared here)."""
    N, L = x.shape
    W = (L + 15) // 16
    pad = np.zeros((N, 16 * W), np.uint32)
    pad[:, :L] = x
    out = (pad.reshape(N, W, 16) << (2 * np.arange(16, dtype=np.uint32))).sum(-1).astype(np.uint32)
    assert np.array_equal(out[:2], Q.pack_ref(x[:2])[0])
    return _dev(out.view(np.int32))


def _nn(q, db, L, key, hist, q_base=0, db_base=0, exclude_diag=0):
    """One launch on packed device rows into the guarded key / hist buffers (either may be None) -> (key u64, hist i64)."""
    rc = _lib.lib().svdd_hamming_nn(q.data_ptr(), db.data_ptr(), q.shape[0], db.shape[0], L, q_base, db_base, exclude_diag,
                                    None if key is None else key.ptr, None if hist is None else hist.ptr, _st())
    _lib.check(rc, "svdd_hamming_nn")
    torch.cuda.synchronize()
    key is None or key.untouched(), hist is None or hist.untouched()     # the guards
    return (None if key is None else key.cpu().numpy().view(np.uint64).copy(), None if hist is None else hist.cpu().numpy().copy())


def _fresh(B, L):
    return _i64(np.full(B, -1)), _i64(np.zeros(L + 1))


@pytest.mark.parametrize("L", [1, 16, 17, 200, 1024])
@pytest.mark.parametrize("B,N", [(1, 1), (3, 5), (65, 130), (64, 1025)])
def test_hamming_nn_equals_the_restatement(B, N, L):
    hi = 2 if L == 1 else 4
    xq, xdb = _tokens(B, L, 3 * L + B, hi), _tokens(N, L, 5 * L + N, hi)
    if L >= 16:                                                           # near rows, so that the minimum is not a tie of far ones
        xdb[N // 2] = xq[B // 2]
        xdb[N // 2, L - 1] ^= 1
    key, hist = _nn(_packed(xq), _packed(xdb), L, *_fresh(B, L))
    want_key, want_hist = Q.hamming_nn_ref(xq, xdb)
    assert np.array_equal(hist, want_hist) and hist.sum() == B * N
    assert np.array_equal(key, want_key)
    # each output alone
    key1, none = _nn(_packed(xq), _packed(xdb), L, _fresh(B, L)[0], None)
    none2, hist1 = _nn(_packed(xq), _packed(xdb), L, None, _fresh(B, L)[1])
    assert none is None and none2 is None and np.array_equal(key1, want_key) and np.array_equal(hist1, want_hist)


@pytest.mark.parametrize("L", [33, 64, 100, 250, 500])
def test_hamming_nn_every_word_count_bucket(L):
    """The kernel is compiled for rows of 1, 2, 4, 8, 13, 16, 32 and 64 words; the lengths of the test above reach 1, 2, 13 and 64.
    These reach the others (3 -> 4, 4, 7 -> 8, 16, 32 words), with more database rows than one tile of 64."""
    xq, xdb = _tokens(3, L, L), _tokens(70, L, L + 1)
    xdb[66] = xq[1]
    xdb[66, L - 1] ^= 2
    key, hist = _nn(_packed(xq), _packed(xdb), L, *_fresh(3, L))
    want_key, want_hist = Q.hamming_nn_ref(xq, xdb)
    assert np.array_equal(key, want_key) and np.array_equal(hist, want_hist)
    assert Q.nn_decode_ref(key)[1][1] == 66


@pytest.mark.parametrize("L", [17, 200])
def test_hamming_nn_ties_duplicates_and_edges(L):
    x = _tokens(6, L, L)
    db = _tokens(40, L, L + 1)
    db[31] = db[9] = x[2]                                                 # exact duplicates of query 2 at two indices: the lower wins
    db[20] = x[4]
    db[20, L - 1] = (x[4, L - 1] + 1) % 4                                 # differs only in the last valid position of the last word
    db[25] = x[5]
    db[25, 0] = (x[5, 0] + 2) % 4                                         # differs only in position 0
    key, hist = _nn(_packed(x), _packed(db), L, *_fresh(6, L))
    dist, idx = Q.nn_decode_ref(key)
    assert (dist[2], idx[2]) == (0, 9) and (dist[4], idx[4]) == (1, 20) and (dist[5], idx[5]) == (1, 25)
    want_key, want_hist = Q.hamming_nn_ref(x, db)
    assert np.array_equal(key, want_key) and np.array_equal(hist, want_hist)
    # garbage in the padding bits of the last word changes nothing
    if L % 16:
        dirty = Q.pack_ref(db)[0].copy()
        dirty[:, -1] |= np.uint32(0xFFFFFFFF) << np.uint32(2 * (L % 16))
        key2, hist2 = _nn(_packed(x), _dev(dirty.view(np.int32)), L, *_fresh(6, L))
        assert np.array_equal(key2, want_key) and np.array_equal(hist2, want_hist)
    # all rows equal: distance 0, index 0; without the diagonal row 0 finds row 1
    same = np.repeat(x[:1], 70, axis=0)
    key, hist = _nn(_packed(same), _packed(same), L, *_fresh(70, L))
    dist, idx = Q.nn_decode_ref(key)
    assert (dist == 0).all() and (idx == 0).all() and hist[0] == 70 * 70 and hist.sum() == 70 * 70
    key, hist = _nn(_packed(same), _packed(same), L, *_fresh(70, L), exclude_diag=1)
    dist, idx = Q.nn_decode_ref(key)
    assert (dist == 0).all() and idx[0] == 1 and (idx[1:] == 0).all() and hist[0] == 70 * 69 and hist.sum() == 70 * 69
    # one row against itself: no pair at all, the key keeps its all-ones
    key, hist = _nn(_packed(x[:1]), _packed(x[:1]), L, *_fresh(1, L), exclude_diag=1)
    assert Q.nn_decode_ref(key) == (-1, -1) and hist.sum() == 0


@pytest.mark.parametrize("self_case", [False, True])
def test_hamming_nn_does_not_depend_on_the_cuts(self_case):
    L, B = 200, 65
    xq = _tokens(B, L, 11)
    xdb = xq if self_case else _tokens(130, L, 12)
    xq[40] = xq[7]                                                        # a duplicate inside the batch
    N, ex = xdb.shape[0], int(self_case)
    q, db = _packed(xq), _packed(xdb)
    want_key, want_hist = Q.hamming_nn_ref(xq, xdb, exclude_diag=self_case)
    assert want_hist.sum() == B * N - (B if self_case else 0)
    key, hist = _nn(q, db, L, *_fresh(B, L), exclude_diag=ex)
    assert np.array_equal(key, want_key) and np.array_equal(hist, want_hist)
    for rows in (1, 33):                                                  # the database in chunks (all rows: above)
        kb, hb = _fresh(B, L)
        for r0 in range(0, N, rows):
            key, hist = _nn(q, db[r0:r0 + rows], L, kb, hb, db_base=r0, exclude_diag=ex)
        assert np.array_equal(key, want_key) and np.array_equal(hist, want_hist), rows
    for rows in (1, 33):                                                  # the queries in chunks
        hb, keys = _i64(np.zeros(L + 1)), []
        for r0 in range(0, B, rows):
            n = min(rows, B - r0)
            kq = _i64(np.full(n, -1))
            key, hist = _nn(q[r0:r0 + rows], db, L, kq, hb, q_base=r0, exclude_diag=ex)
            keys.append(key)
        assert np.array_equal(np.concatenate(keys), want_key) and np.array_equal(hist, want_hist), rows
    kb, hb = _fresh(B, L)                                                 # both cut, the chunks in another order
    for q0 in (33, 0):
        for r0 in (66, 0, 99, 33):
            if r0 < N:
                n = min(33, B - q0)
                kq = _i64(kb.cpu().numpy()[q0:q0 + n])
                key, hist = _nn(q[q0:q0 + 33], db[r0:r0 + 33], L, kq, hb, q_base=q0, db_base=r0, exclude_diag=ex)
                kb.body()[q0:q0 + n] = _dev(key.view(np.int64))
    assert np.array_equal(kb.cpu().numpy().view(np.uint64), want_key) and np.array_equal(hist, want_hist)


def test_hamming_nn_over_several_segments():
    """More database rows than one workgroup's segment (the host cuts the database for about a thousand workgroups), more
    queries than one workgroup, bases near 2^31."""
    L, B, N = 40, 300, 70000
    xq, xdb = _tokens(B, L, 21), _tokens(N, L, 22)
    xdb[69999] = xdb[123] = xq[299]
    base = (1 << 31) - 1 - N
    key, hist = _nn(_packed(xq), _packed(xdb), L, *_fresh(B, L), db_base=base)
    d = torch.from_numpy(xq).to(DEV)[:, None, :] != torch.from_numpy(xdb).to(DEV)[None, :, :]
    d = d.sum(-1)                                                         # [B, N] on the device: this size is beyond the host loops
    want_hist = torch.bincount(d.reshape(-1), minlength=L + 1).cpu().numpy()
    want_key = ((d << 32) | (base + torch.arange(N, device=DEV))).min(1).values.cpu().numpy().view(np.uint64)
    dist, idx = Q.nn_decode_ref(key)
    assert np.array_equal(hist, want_hist) and hist.sum() == B * N
    assert np.array_equal(key, want_key) and (dist[299], idx[299]) == (0, base + 123)


# -------------------------------------------------------------------------------------------------- the public API ----
def test_sample_quality_on_the_recorded_sets():
    from svdd_amd import quality
    g = load_golden("g40_quality.npz")
    for xn, yn in (("a200", "b200"), ("a50", "b50"), ("s1", "s2")):
        x, y = g[xn], g[yn]
        counts, skipped = quality.kmer_counts(torch.from_numpy(x).to(DEV))
        assert np.array_equal(counts.cpu().numpy(), g["kmers_" + xn]) and skipped == 0
        assert np.array_equal(quality.kmer_counts(x, chunk_rows=5)[0].cpu().numpy(), g["kmers_" + xn])
        r = quality.kmer_pearsonr(x, y)
        print(f"ERR kmer_pearsonr_{xn}_{yn} {abs(r - float(g[f'r_{xn}_{yn}'])):.3e} bar {BAR:.1e}")
        assert abs(r - float(g[f"r_{xn}_{yn}"])) <= BAR
        assert quality.kmer_pearsonr(x, g["kmers_" + yn]) == r            # a ready count vector
        sa, sb = g["scores_a"][:x.shape[0]], g["scores_b"]
        got = quality.sample_quality(torch.from_numpy(x).to(DEV).long(), refs={"valid": y, "counts": g["kmers_" + yn]}, train=y,
                                     scores=sa, ref_scores={"valid": sb})
        want = Q.sample_quality_ref(x, refs={"valid": y, "counts": g["kmers_" + yn]}, train=y, scores=sa, ref_scores={"valid": sb})
        assert sorted(got) == sorted(want) == sorted(
            ["kmer_pearsonr_valid", "kmer_pearsonr_counts", "diversity_mean", "diversity_nn_median", "unique_fraction",
             "novelty_nn_median", "novelty_nn_min", "memorised_fraction", "ws_scores_valid"])
        for key in ("diversity_nn_median", "unique_fraction", "novelty_nn_median", "novelty_nn_min", "memorised_fraction"):
            assert got[key] == want[key], key                             # integers and ratios of integers
        assert abs(got["diversity_mean"] - want["diversity_mean"]) <= 1e-12
        assert abs(got["kmer_pearsonr_valid"] - float(g[f"r_{xn}_{yn}"])) <= BAR and got["kmer_pearsonr_counts"] == got["kmer_pearsonr_valid"]
        assert abs(got["ws_scores_valid"] - want["ws_scores_valid"]) <= BAR
        dist, idx = quality.hamming_nn(x, y, chunk_rows=7)
        wd, wi = Q.nn_decode_ref(Q.hamming_nn_ref(x, y)[0])
        assert dist.dtype == torch.int32 and idx.dtype == torch.int64
        assert np.array_equal(dist.cpu().numpy(), wd) and np.array_equal(idx.cpu().numpy(), wi)
        assert np.array_equal(quality.pairwise_hamming_hist(x, y).cpu().numpy(), Q.hamming_nn_ref(x, y)[1])
        assert np.array_equal(quality.pairwise_hamming_hist(x).cpu().numpy(), Q.hamming_nn_ref(x, x, exclude_diag=True)[1])
    ws = quality.wasserstein_1d(_dev(g["scores_a"]), g["scores_b"])
    fr = quality.frechet_distance(_dev(g["emb_a"]), _dev(g["emb_b"]))
    print(f"ERR wasserstein {abs(ws - float(g['ws_scores'])):.3e} bar {BAR:.1e}")
    print(f"ERR frechet {abs(fr - float(g['frechet'])):.3e} bar {BAR:.1e}")
    assert abs(ws - float(g["ws_scores"])) <= BAR and abs(fr - float(g["frechet"])) <= BAR


def test_duplicates_masks_and_one_row():
    from svdd_amd import ops, quality
    x = _tokens(9, 50, 3)
    x[6] = x[2]
    dist, idx = quality.hamming_nn(_dev(x))
    assert dist[2] == 0 and dist[6] == 0 and idx[2] == 6 and idx[6] == 2 and int((dist == 0).sum()) == 2
    q = quality.sample_quality(x)
    assert q["unique_fraction"] == 8 / 9 == Q.unique_fraction_ref(x)
    x[7] = x[2]                                                           # a group of three: still one representative
    assert quality.sample_quality(x)["unique_fraction"] == 7 / 9
    dist, idx = quality.hamming_nn(x[:1])
    assert dist.tolist() == [-1] and idx.tolist() == [-1]
    one = quality.sample_quality(x[:1])
    assert np.isnan(one["diversity_mean"]) and np.isnan(one["diversity_nn_median"]) and one["unique_fraction"] == 1.0
    assert quality.sample_quality(x, train=x[3:5])["memorised_fraction"] == 2 / 9
    packed = quality.pack_tokens(_dev(x))
    assert np.array_equal(packed.cpu().numpy().view(np.uint32), Q.pack_ref(x)[0])
    bad = _dev(x).clone()
    bad[4, 4] = 4                                                         # on the device the kernel's err word speaks
    for fn in (quality.pack_tokens, quality.hamming_nn, quality.pairwise_hamming_hist, quality.sample_quality):
        with pytest.raises(ops.SvddError, match="token > 3"):
            fn(bad)
    with pytest.raises(ops.SvddError, match="token > 3"):
        quality.hamming_nn(_dev(x), bad.long())
    counts, skipped = quality.kmer_counts(bad)                            # the spectrum skips the windows instead
    want, want_skipped = Q.kmer_counts_ref(bad.cpu().numpy(), 3)
    assert skipped == want_skipped == 3 and np.array_equal(counts.cpu().numpy(), want)
    z = np.zeros((4, 10), np.uint8)                                       # one 3-mer only: fewer than two bins in the union
    assert np.isnan(quality.kmer_pearsonr(z, z))


def test_harness_evaluate_quality_and_cli(tmp_path):
    from svdd_amd import cli
    from svdd_amd.harness import BaseModel
    from svdd_amd.value_nets import RewardModel
    from tests import e2e_parity
    model, emb, head = e2e_parity.tiny_engine(load_golden("nets_tiny.npz"), 50, 4, DEV)
    reward = RewardModel(emb, head).to(DEV).eval()
    model.rng_mode, model.philox_seed = "philox", 9
    hm = BaseModel(emb, head, model, reward, batch_size=4, task="dna")
    samples = hm.controlled_decode(gen_batch_num=2, sample_M=2)[0]
    g = load_golden("g40_quality.npz")
    rep = hm.evaluate_quality(samples, refs={"valid": g["a50"], "test": g["kmers_b50"]}, train=g["b50"])
    assert sorted(rep) == sorted(["kmer_pearsonr_valid", "kmer_pearsonr_test", "diversity_mean", "diversity_nn_median",
                                  "unique_fraction", "novelty_nn_median", "novelty_nn_min", "memorised_fraction", "ws_scores_valid"])
    x = torch.cat(samples).cpu().numpy()
    by4 = lambda t: torch.cat([hm._reward(t[i:i + 4]) for i in range(0, t.shape[0], 4)]).cpu().numpy()     # noqa: E731  (its batches)
    scores, ref_scores = by4(torch.cat(samples)), by4(_dev(g["a50"]).long())
    want = Q.sample_quality_ref(x, refs={"valid": g["a50"], "test": g["kmers_b50"]}, train=g["b50"], scores=scores,
                                ref_scores={"valid": ref_scores})
    for key, v in want.items():
        assert abs(rep[key] - v) <= BAR or (np.isnan(v) and np.isnan(rep[key])), key
    sets = tmp_path / "sets.npz"
    np.savez(sets, train=_tokens(12, 50, 1), test=_tokens(6, 50, 2))
    args = ["--task", "rna", "--batch_size", "2", "--sample_M", "2", "--val_batch_num", "1", "--rng", "philox"]
    path, _ = cli.main("mc", args + ["--out_dir", str(tmp_path / "on"), "--eval_quality", str(sets)])
    z = np.load(path)
    assert sorted(z.files) == sorted(["baseline", "decoding"] + ["quality_" + k for k in (
        "kmer_pearsonr_train", "kmer_pearsonr_test", "diversity_mean", "diversity_nn_median", "unique_fraction", "novelty_nn_median",
        "novelty_nn_min", "memorised_fraction", "ws_scores_train", "ws_scores_test")])
    path0, _ = cli.main("mc", args + ["--out_dir", str(tmp_path / "off")])
    assert sorted(np.load(path0).files) == ["baseline", "decoding"]
    assert np.array_equal(np.load(path0)["decoding"], z["decoding"])
