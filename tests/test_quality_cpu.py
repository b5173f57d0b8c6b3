"""No GPU: sample-quality metrics.

  restatement  tests/quality_ref.py reproduces g40_quality.npz (the reference's count_kmers / compare_kmer / scipy's Wasserstein /
               get_wasserstein_dist, tests/golden/make_golden_quality.py): counts exactly; r, Wasserstein and Frechet within 1e-10
               (four orders above float64 summation-order error over <= 4096 terms, about 9e-13; six below the 1e-4 the project
               holds recorded soft values to). The packed-word rule equals the position count; first wins.
  host rules   svdd_amd.quality's float64 rules (union Pearson, wasserstein_1d, frechet_distance) equal the same recordings
  entries      svdd_kmer_counts / svdd_pack_tokens / svdd_hamming_nn refuse bad arguments before they touch a device; ABI 17;
               explicit streams
  python       the wrappers refuse wrong dtypes and shapes, and tokens > 3 where they are not allowed, before any launch
"""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from tests import quality_ref as Q
from tests.conftest import load_golden

BAR = 1e-10
PAIRS = (("a200", "b200"), ("a50", "b50"), ("s1", "s2"))


@pytest.fixture(scope="module")
def g40():
    return load_golden("g40_quality.npz")


# ------------------------------------------------------------------------------------------------ the restatement ----
def test_restated_counts_equal_the_references(g40):
    for name in ("a200", "b200", "a50", "b50", "s1", "s2"):
        counts, skipped = Q.kmer_counts_ref(g40[name], 3)
        assert skipped == 0 and np.array_equal(counts, g40["kmers_" + name]), name


def test_restated_pearson_follows_the_union_rule(g40):
    for x, y in PAIRS:
        r = Q.pearson_union_ref(g40["kmers_" + x], g40["kmers_" + y])
        print(f"ERR pearson_{x}_{y} {abs(r - float(g40[f'r_{x}_{y}'])):.3e} bar {BAR:.1e}")
        assert abs(r - float(g40[f"r_{x}_{y}"])) <= BAR, (x, y)
    # the skewed pair: 56 bins are zero on both sides, and a correlation over all 64 bins is another number
    k1, k2 = g40["kmers_s1"], g40["kmers_s2"]
    assert int(((k1 == 0) & (k2 == 0)).sum()) == 56
    a, b = k1 - k1.mean(), k2 - k2.mean()
    all64 = float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))
    assert abs(all64 - float(g40["r_all64_s1_s2"])) <= BAR and abs(all64 - float(g40["r_s1_s2"])) > 1e-3


def test_pearson_degenerate_inputs_give_nan():
    z = np.zeros(64, np.int64)
    one = z.copy()
    one[5] = 7
    flat = z.copy()
    flat[:4] = 3
    ramp = z.copy()
    ramp[:4] = [1, 2, 3, 4]
    assert np.isnan(Q.pearson_union_ref(z, z)) and np.isnan(Q.pearson_union_ref(one, one))      # 0 and 1 bins in the union
    assert np.isnan(Q.pearson_union_ref(flat, ramp)) and np.isnan(Q.pearson_union_ref(ramp, flat))   # no variance on a side
    assert abs(Q.pearson_union_ref(ramp, 3 * ramp) - 1.0) <= 1e-15                               # a positive factor changes nothing


def test_restated_wasserstein_and_frechet(g40):
    ws = Q.wasserstein_1d_ref(g40["scores_a"], g40["scores_b"])
    fr = Q.frechet_ref(g40["emb_a"], g40["emb_b"])
    print(f"ERR wasserstein {abs(ws - float(g40['ws_scores'])):.3e} bar {BAR:.1e}")
    print(f"ERR frechet {abs(fr - float(g40['frechet'])):.3e} bar {BAR:.1e}")
    assert g40["scores_a"].size != g40["scores_b"].size
    assert abs(ws - float(g40["ws_scores"])) <= BAR
    assert abs(fr - float(g40["frechet"])) <= BAR
    assert np.isnan(Q.frechet_ref(np.zeros((0, 8)), g40["emb_b"]))
    bad = g40["emb_a"].copy()
    bad[3, 2] = np.nan
    assert np.isnan(Q.frechet_ref(bad, g40["emb_b"]))


def test_packed_rule_equals_the_position_count():
    rng = np.random.default_rng(0)
    for L in (1, 15, 16, 17, 33, 200):
        x = rng.integers(0, 4, (6, L)).astype(np.uint8)
        p, err = Q.pack_ref(x)
        assert err == 0 and p.shape == (6, (L + 15) // 16)
        if L % 16:
            assert (p[:, -1] >> np.uint32(2 * (L % 16)) == 0).all()                              # padding bits
        d = Q.hamming_matrix(x, x)
        for i in range(6):
            for j in range(6):
                assert Q.packed_distance(p[i], p[j]) == d[i, j]
    x = np.array([[0, 4, 3]], np.uint8)
    p, err = Q.pack_ref(x)
    assert err == 1 and p[0, 0] == 3 << 4


def test_first_wins_and_chunk_independence_of_the_restatement():
    rng = np.random.default_rng(1)
    x = rng.integers(0, 4, (5, 20)).astype(np.uint8)
    db = rng.integers(0, 4, (12, 20)).astype(np.uint8)
    db[7] = db[3] = x[2]                                                                          # two exact copies of query 2
    key, hist = Q.hamming_nn_ref(x, db)
    dist, idx = Q.nn_decode_ref(key)
    assert dist[2] == 0 and idx[2] == 3 and hist.sum() == 5 * 12
    key2, hist2 = None, None
    for r0 in (8, 0, 4):                                                                          # any order of the chunks
        key2, hist2 = Q.hamming_nn_ref(x, db[r0:r0 + 4], db_base=r0, nn_key=key2, hist=hist2)
    assert np.array_equal(key, key2) and np.array_equal(hist, hist2)
    key, hist = Q.hamming_nn_ref(x[:1], x[:1], exclude_diag=True)
    assert Q.nn_decode_ref(key) == (-1, -1) and hist.sum() == 0
    rep = np.stack([x[0]] * 3)
    dist, idx = Q.nn_decode_ref(Q.hamming_nn_ref(rep, rep, exclude_diag=True)[0])
    assert dist.tolist() == [0, 0, 0] and idx.tolist() == [1, 0, 0]


# ------------------------------------------------------------------------------------------- the module's host rules ----
def test_module_host_rules_equal_the_recordings(g40):
    from svdd_amd import quality
    for x, y in PAIRS:
        r = quality._pearson_union(torch.from_numpy(g40["kmers_" + x]), torch.from_numpy(g40["kmers_" + y]))
        assert abs(r - float(g40[f"r_{x}_{y}"])) <= BAR, (x, y)
    z = torch.zeros(64, dtype=torch.int64)
    assert np.isnan(quality._pearson_union(z, z))
    ws = quality.wasserstein_1d(g40["scores_a"], torch.from_numpy(g40["scores_b"]))
    fr = quality.frechet_distance(g40["emb_a"], g40["emb_b"])
    print(f"ERR module_wasserstein {abs(ws - float(g40['ws_scores'])):.3e} bar {BAR:.1e}")
    print(f"ERR module_frechet {abs(fr - float(g40['frechet'])):.3e} bar {BAR:.1e}")
    assert abs(ws - float(g40["ws_scores"])) <= BAR and abs(fr - float(g40["frechet"])) <= BAR
    assert abs(ws - Q.wasserstein_1d_ref(g40["scores_a"], g40["scores_b"])) <= 1e-12
    assert np.isnan(quality.frechet_distance(np.zeros((0, 8)), g40["emb_b"])) and np.isnan(quality.wasserstein_1d([], [1.0]))
    bad = g40["emb_a"].copy()
    bad[0, 0] = np.nan
    assert np.isnan(quality.frechet_distance(bad, g40["emb_b"]))
    assert quality.wasserstein_1d([0.0, 1.0], [0.0, 1.0]) == 0.0 and abs(quality.wasserstein_1d([0.0], [2.5, 2.5]) - 2.5) <= 1e-15


# ------------------------------------------------------------------------------------------------------ the entries ----
def test_quality_entries_refuse_bad_arguments_without_a_device():
    from svdd_amd import _lib
    L_ = _lib.lib()
    assert _lib.ABI_VERSION == 17 and L_.svdd_abi_version() == 17
    for name in ("svdd_kmer_counts", "svdd_pack_tokens", "svdd_hamming_nn"):
        assert name in _lib.EXPORTS
        sig = _lib.SIGNATURES[name]
        assert sig[-1] is _lib.vp and sig[-1] is not _lib.STREAM and _lib.STREAM not in sig      # the stream is the caller's (`on_stream`)
    p = [ctypes.c_void_p(4096 * (i + 1)) for i in range(6)]               # non-NULL pointers that are never dereferenced

    def kmer(**kw):
        a = dict(x=p[0], N=4, L=20, k=3, counts=p[1], skipped=None, stream=None)
        a.update(kw)
        return L_.svdd_kmer_counts(*a.values())
    for what, kw in {"N = 0": dict(N=0), "N < 0": dict(N=-2), "L = 0": dict(L=0), "L < 0": dict(L=-1), "k = 0": dict(k=0),
                     "k = 7": dict(k=7), "k < 0": dict(k=-3), "x null": dict(x=None), "counts null": dict(counts=None),
                     "k > L but k = 7": dict(L=2, k=7), "k > L but counts null": dict(L=2, k=3, counts=None)}.items():
        assert kmer(**kw) == _lib.E_ARG, what
    assert kmer(L=2, k=3) == _lib.OK                                       # k > L: valid, no windows, no launch

    def pack(**kw):
        a = dict(x=p[0], N=4, L=20, packed=p[1], err=None, stream=None)
        a.update(kw)
        return L_.svdd_pack_tokens(*a.values())
    for what, kw in {"N = 0": dict(N=0), "N < 0": dict(N=-1), "L = 0": dict(L=0), "L < 0": dict(L=-5), "L = 1025": dict(L=1025),
                     "x null": dict(x=None), "packed null": dict(packed=None)}.items():
        assert pack(**kw) == _lib.E_ARG, what

    def nn(**kw):
        a = dict(q=p[0], db=p[1], B=3, N=5, L=20, q_base=0, db_base=0, exclude_diag=0, nn_key=p[2], hist=p[3], stream=None)
        a.update(kw)
        return L_.svdd_hamming_nn(*a.values())
    top = (1 << 31) - 1
    for what, kw in {"B = 0": dict(B=0), "B < 0": dict(B=-1), "N = 0": dict(N=0), "N < 0": dict(N=-1), "L = 0": dict(L=0),
                     "L < 0": dict(L=-1), "L = 1025": dict(L=1025), "q_base < 0": dict(q_base=-1), "db_base < 0": dict(db_base=-1),
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
    for fn in (quality.pack_tokens, quality.hamming_nn, quality.pairwise_hamming_hist, quality.sample_quality):
        with pytest.raises(ValueError, match="token"):
            fn(bad)                                                        # MASK has no 2-bit code
        with pytest.raises(ValueError, match="integer"):
            fn(x.float())
        with pytest.raises(ValueError, match=r"\[N, L\]"):
            fn(x[0])
        with pytest.raises(ValueError, match=r"\[N, L\]"):
            fn(x[:0])
    with pytest.raises(ValueError, match="token"):
        quality.hamming_nn(x, bad)
    with pytest.raises(ValueError, match="one length"):
        quality.hamming_nn(x, x[:, :10])
    with pytest.raises(ValueError, match="1024"):
        quality.pack_tokens(torch.zeros(1, 1025, dtype=torch.uint8))
    with pytest.raises(ValueError, match="token"):
        quality.kmer_counts(x - 1)
    with pytest.raises(ValueError, match="integer"):
        quality.kmer_counts(np.zeros((2, 5), np.float32))
    for k in (0, 7, 2.0, True):
        with pytest.raises(ValueError, match="k ="):
            quality.kmer_counts(x, k=k)
        with pytest.raises(ValueError, match="k ="):
            quality.kmer_pearsonr(x, x, k=k)
    for rows in (0, -4, 1.5):
        with pytest.raises(ValueError, match="chunk_rows"):
            quality.kmer_counts(x, chunk_rows=rows)
        with pytest.raises(ValueError, match="chunk_rows"):
            quality.hamming_nn(x, chunk_rows=rows)
    if not torch.cuda.is_available():
        with pytest.raises(ops.SvddError, match="GPU"):                    # valid arguments: no CPU fallback
            quality.kmer_counts(bad)
        with pytest.raises(ops.SvddError, match="GPU"):
            quality.hamming_nn(x)
    # the raw wrappers take device tensors only
    c = torch.zeros(64, dtype=torch.int64)
    with pytest.raises(ops.SvddError, match="GPU"):
        ops.kmer_counts(x.to(torch.uint8), 3, c)
    with pytest.raises(ValueError, match="k ="):
        ops.kmer_counts(x.to(torch.uint8), 9, c)
    with pytest.raises(ops.SvddError, match="GPU"):
        ops.pack_tokens(x.to(torch.uint8))
    with pytest.raises(ops.SvddError, match="GPU"):
        ops.hamming_nn(torch.zeros(2, 2, dtype=torch.int32), torch.zeros(2, 2, dtype=torch.int32), 20, hist=torch.zeros(21, dtype=torch.int64))
    with pytest.raises(ops.SvddError, match="outside"):
        ops.hamming_nn(torch.zeros(2, 2, dtype=torch.int32), torch.zeros(2, 2, dtype=torch.int32), 2000)


def test_public_signatures():
    from svdd_amd import cli, quality
    from svdd_amd.harness import BaseModel
    sig = lambda f: list(inspect.signature(f).parameters)                  # noqa: E731
    assert sig(quality.kmer_counts) == ["x", "k", "chunk_rows"] and inspect.signature(quality.kmer_counts).parameters["k"].default == 3
    assert sig(quality.kmer_pearsonr) == ["x", "ref", "k"]
    assert sig(quality.pack_tokens) == ["x"]
    assert sig(quality.hamming_nn) == ["x", "db", "chunk_rows"]
    assert sig(quality.pairwise_hamming_hist) == ["x", "db"]
    assert sig(quality.wasserstein_1d) == ["a", "b"] and sig(quality.frechet_distance) == ["e1", "e2"]
    assert sig(quality.sample_quality) == ["x", "refs", "train", "k", "scores", "ref_scores"]
    assert sig(BaseModel.evaluate_quality) == ["self", "samples", "refs", "train", "k"]
    assert not hasattr(cli.build_parser().parse_args([]), "eval_quality")      # without the flag the namespace is what it was
    assert cli.build_parser().parse_args(["--eval_quality", "sets.npz"]).eval_quality == "sets.npz"
