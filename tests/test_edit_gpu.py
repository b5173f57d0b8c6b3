"""-m gpu: edit-distance novelty. Everything here is an exact integer and must EQUAL tests/edit_ref.py.

  kernel   svdd_edit_nn through the raw C entry in sentinel-guarded buffers (tests/kernel_harness.py), each output once NULL and
           once given: every word edge of the query and of the score bit, unequal lengths in both directions, every word-count
           bucket the kernel is compiled for (1, 2, 4, 7, 8, 16, 32 words of 32 positions), carries that run through every word,
           one and several tiles, segments and workgroups, every cap with both of its sides populated, ties, the diagonal, every
           cut of queries and database, keys seeded at, above and below the answer
  public   quality.edit_nn / pairwise_edit_hist / edit_quality, BaseModel.evaluate_edit and --eval_edit; what Hamming misses
"""
import numpy as np
import pytest
import torch

from svdd_amd import _lib
from tests import edit_ref as E
from tests import quality_ref as Q
from tests.conftest import load_golden
from tests.kernel_harness import DEV, _Buf, _st

pytestmark = pytest.mark.gpu
ONES = Q.ALL_ONES


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _i64(init):
    """A guarded i64 buffer holding `init` (the outputs start from the caller's values)."""
    init = np.asarray(init).astype(np.int64).reshape(-1)
    b = _Buf(2 * init.size, torch.int64)
    b.body().copy_(_dev(init))
    return b


def _tokens(N, L, seed, hi=4):
    return np.random.default_rng(seed).integers(0, hi, (N, L)).astype(np.uint8)


def _packed(x, dirty=False):
    """svdd_pack_tokens' rule with numpy shifts, in a guarded buffer of its own; dirty: all ones in the padding bits."""
    N, L = x.shape
    W = (L + 15) // 16
    pad = np.full((N, 16 * W), 3 if dirty else 0, np.uint32)
    pad[:, :L] = x
    out = (pad.reshape(N, W, 16) << (2 * np.arange(16, dtype=np.uint32))).sum(-1).astype(np.uint32)
    b = _Buf(N * W, torch.int32)
    b.body().copy_(_dev(out.view(np.int32).reshape(-1)))
    return b


def _nn(xq, xdb, cap, key, hist, q_base=0, db_base=0, exclude_diag=0, dirty=False):
    """One launch on unpacked host rows into the guarded key / hist buffers (either may be None) -> (key u64, hist i64)."""
    q, db = _packed(xq, dirty), _packed(xdb, dirty)
    rc = _lib.lib().svdd_edit_nn(q.ptr, db.ptr, xq.shape[0], xdb.shape[0], xq.shape[1], xdb.shape[1], cap, q_base, db_base,
                                 exclude_diag, None if key is None else key.ptr, None if hist is None else hist.ptr, _st())
    _lib.check(rc, "svdd_edit_nn")
    torch.cuda.synchronize()
    q.untouched(), db.untouched(), key is None or key.untouched(), hist is None or hist.untouched()     # the guards
    return (None if key is None else key.cpu().numpy().view(np.uint64).copy(), None if hist is None else hist.cpu().numpy().copy())


def _fresh(B, cap):
    return _i64(np.full(B, -1)), _i64(np.zeros(cap + 2))


def _all_ways(xq, xdb, cap, d=None, **kw):
    """Both outputs, then each alone: all must equal the restatement (d: its table, where the caller has it) -> (key, hist)."""
    B = xq.shape[0]
    want_key, want_hist = E.edit_nn_ref(xq, xdb, cap, q_base=kw.get("q_base", 0), db_base=kw.get("db_base", 0),
                                        exclude_diag=bool(kw.get("exclude_diag", 0)), d=d)
    key, hist = _nn(xq, xdb, cap, *_fresh(B, cap), **kw)
    assert np.array_equal(hist, want_hist), (hist, want_hist)
    assert np.array_equal(key, want_key)
    key1, none = _nn(xq, xdb, cap, _fresh(B, cap)[0], None, **kw)
    none2, hist1 = _nn(xq, xdb, cap, None, _fresh(B, cap)[1], **kw)
    assert none is None and none2 is None and np.array_equal(key1, want_key) and np.array_equal(hist1, want_hist)
    return key, hist


def mutate(row, edits, rng, L):
    """`edits` random edits of row: a substitution if the number is odd, then insertions and deletions in turn, so that a row of
    length L keeps it (any other is cut or filled at the end)."""
    r = list(row)
    for e in range(edits):
        kind, p = 0 if e == 0 and edits % 2 else 1 + (edits - e) % 2, int(rng.integers(0, len(r)))
        if kind == 0:
            r[p] = (r[p] + 1 + int(rng.integers(0, 3))) % 4
        elif kind == 1:
            r.insert(p, int(rng.integers(0, 4)))
        else:
            del r[p]
    r = r[:L] + [int(t) for t in rng.integers(0, 4, max(0, L - len(r)))]
    return np.array(r, np.uint8)


# ------------------------------------------------------------------------------------------- words, lengths, shapes ----
@pytest.mark.parametrize("Lq", [1, 2, 31, 32, 33, 63, 64, 65, 200, 1024])
def test_edit_nn_word_and_score_bit_edges(Lq):
    for Ld in (1, 16, 17, 33, 200):
        if Ld == Lq:
            continue
        hi = 2 if min(Lq, Ld) == 1 else 4
        xq, xdb = _tokens(3, Lq, 3 * Lq + Ld, hi), _tokens(5, Ld, 5 * Lq + Ld, hi)
        n = min(Lq, Ld)
        xdb[2, :n] = xq[1, :n]                                            # a near pair: one row is the other's prefix
        _all_ways(xq, xdb, max(Lq, Ld), dirty=True)                       # garbage in the padding bits changes nothing
    x = _tokens(3, Lq, Lq)                                                # equal lengths, the self case
    _all_ways(x, x, Lq, exclude_diag=1)
    if Lq == 1024:
        a, b = _tokens(1, 1024, 1), _tokens(1, 1024, 2)
        b[0, 5:] = a[0, :-5]                                              # shifted by 5
        key, hist = _all_ways(a, b, 1024)
        assert Q.nn_decode_ref(key)[0][0] <= 10


@pytest.mark.parametrize("L", [17, 33])
@pytest.mark.parametrize("B,N", [(1, 1), (65, 130), (257, 64), (64, 1025)])
def test_edit_nn_tiles_segments_and_workgroups(B, N, L):
    """A tile is 64 database rows and, below 2^18 rows, so is a segment: 130 and 1025 rows cross tile and segment boundaries
    (3 and 17 segments), 257 queries are two workgroups."""
    rng = np.random.default_rng(L + B)
    xq, xdb = _tokens(B, L, 3 * L + B), _tokens(N, L + (B == 65), 5 * L + N)
    for i in range(0, B, 7):                                              # near rows, so that the minimum is not a tie of far ones
        xdb[(5 * i + 3) % N] = mutate(xq[i], i % 4, rng, xdb.shape[1])
    d = E.edit_matrix(xq, xdb)
    key, hist = _all_ways(xq, xdb, xdb.shape[1], d)
    assert hist.sum() == B * N and hist[-1] == 0
    _all_ways(xq, xdb, 3, d)


def test_edit_nn_over_many_segments_with_bases_near_the_top():
    """Rows of 3 positions: 64 possible rows, so the answer is known without the table: d = 0 where the row occurs (first index)."""
    B, N, L = 300, 70000, 3
    xq, xdb = _tokens(B, L, 21), _tokens(N, L, 22)
    base = (1 << 31) - 1 - N
    key, hist = _nn(xq, xdb, 0, *_fresh(B, 0), db_base=base)
    code = lambda x: (x.astype(np.int64) * np.array([16, 4, 1])).sum(1)   # noqa: E731
    cq, cdb = code(xq), code(xdb)
    first = np.array([np.flatnonzero(cdb == c)[0] for c in cq])
    dist, idx = Q.nn_decode_ref(key)
    assert (dist == 0).all() and np.array_equal(idx, base + first)
    same = int((np.bincount(cq, minlength=64) * np.bincount(cdb, minlength=64)).sum())
    assert hist.tolist() == [same, B * N - same]


# ---------------------------------------------------------------------------------------------------- carry chains ----
@pytest.mark.parametrize("L", [20, 50, 100, 200, 250, 500, 1000])
def test_edit_nn_carries_through_every_word(L):
    """One length in every word-count bucket (1, 2, 4, 7, 8, 16, 32 words). All-A against all-A: the add's carry ripples through
    every word at every column."""
    rng = np.random.default_rng(L)
    # the database's packed words end every 16 positions; the query sits at the top of the kernel's integer, so its 32-bit words
    # end where position + (-L mod 32) is a multiple of 32
    edges = sorted({p for p in range(L) if p % 16 in (15, 0, 1) or (p + -L % 32) % 32 in (31, 0, 1)} | {L - 1})
    if L > 250:
        edges = edges[:8] + edges[len(edges) // 2 - 4:len(edges) // 2 + 4] + edges[-8:]
    rand = _tokens(1, L, L + 1)[0]
    xq = np.stack([np.zeros(L, np.uint8), rand])
    # equal lengths: all-A, all-C, one C substituted at every word edge, the random row shifted by 1, 3 and 17
    rows = [np.zeros(L, np.uint8), np.ones(L, np.uint8)]
    for p in edges:
        r = np.zeros(L, np.uint8)
        r[p] = 1
        rows.append(r)
    for s in (1, 3, 17):
        rows.append(np.concatenate([rand[s:], rng.integers(0, 4, s).astype(np.uint8)]))
    d = E.edit_matrix(xq, np.stack(rows))
    key, hist = _all_ways(xq, np.stack(rows), L, d)
    assert d[0, 0] == 0 and d[0, 1] == L and (d[0, 2:2 + len(edges)] == 1).all()
    assert d[1, -3] == 2 and d[1, -2] <= 6 and d[1, -1] <= 34
    # one longer: all-A, all-C, one C INSERTED at every word edge
    rows = [np.zeros(L + 1, np.uint8), np.ones(L + 1, np.uint8)]
    for p in edges + [L]:
        r = np.zeros(L + 1, np.uint8)
        r[p] = 1
        rows.append(r)
    if L + 1 <= 1024:
        d = E.edit_matrix(xq, np.stack(rows))
        _all_ways(xq, np.stack(rows), 1, d)
        assert d[0, 0] == 1 and d[0, 1] == L + 1 and (d[0, 2:] == 1).all()


# ------------------------------------------------------------------------------------------------------------- cap ----
def test_edit_nn_caps_with_planted_mutants():
    L, N = 50, 40
    rng = np.random.default_rng(5)
    xdb = _tokens(N, L, 50)
    xq = np.stack([mutate(xdb[3 * e], e, rng, L) for e in range(9)] + list(_tokens(4, L, 51)))     # 0 .. 8 edits, and four strangers
    d = E.edit_matrix(xq, xdb)
    assert [int(d[e, 3 * e]) <= e for e in range(9)] == [True] * 9 and d[0, 0] == 0 and d[9:].min() > 8
    for cap in (0, 1, 5, L):
        key, hist = _all_ways(xq, xdb, cap, d)
        if cap < L:
            assert (d == cap).any() and (d[:9].min(1) > cap).any()        # both sides of the cap, the near side at the cap itself
        assert hist[cap + 1] == (d > cap).sum() and hist.sum() == 13 * N
        nothing = d.min(1) > cap
        assert nothing[9:].all() or cap == L
        assert (key[nothing] == ONES).all() and (key[~nothing] != ONES).all()


# ------------------------------------------------------------------------------------- ties, duplicates, diagonal ----
@pytest.mark.parametrize("L", [17, 200])
def test_edit_nn_ties_duplicates_and_the_diagonal(L):
    x, db = _tokens(6, L, L), _tokens(40, L, L + 1)
    db[31] = db[9] = x[2]                                                 # exact duplicates of query 2 at two indices: the lower wins
    db[20] = np.concatenate([x[4][1:], x[4][:1]])                         # query 4 rotated by one: 2 edits
    db[33] = db[20]
    key, hist = _all_ways(x, db, L)
    dist, idx = Q.nn_decode_ref(key)
    assert (dist[2], idx[2]) == (0, 9) and (dist[4], idx[4]) == (2, 20)
    same = np.repeat(x[:1], 70 if L == 17 else 6, axis=0)                 # all rows equal (more than one tile at the short length)
    n = same.shape[0]
    key, hist = _all_ways(same, same, 0)
    dist, idx = Q.nn_decode_ref(key)
    assert (dist == 0).all() and (idx == 0).all() and hist.tolist() == [n * n, 0]
    key, hist = _all_ways(same, same, 0, exclude_diag=1)
    dist, idx = Q.nn_decode_ref(key)
    assert (dist == 0).all() and idx[0] == 1 and (idx[1:] == 0).all() and hist.tolist() == [n * (n - 1), 0]
    key, hist = _nn(x[:1], x[:1], L, *_fresh(1, L), exclude_diag=1)       # one row against itself: no pair at all
    assert Q.nn_decode_ref(key) == (-1, -1) and hist.sum() == 0


# ------------------------------------------------------------------------------------------------------------ cuts ----
@pytest.mark.parametrize("self_case", [False, True])
def test_edit_nn_does_not_depend_on_the_cuts(self_case):
    L, B, cap = 33, 65, 8
    rng = np.random.default_rng(11)
    xq = _tokens(B, L, 11)
    xq[40] = xq[7]                                                        # a duplicate and a near copy inside the batch
    xq[50] = mutate(xq[9], 3, rng, L)
    xdb = xq if self_case else _tokens(130, L, 12)
    if not self_case:
        xdb[77] = mutate(xq[3], 2, rng, L)
    N, ex = xdb.shape[0], int(self_case)
    want_key, want_hist = E.edit_nn_ref(xq, xdb, cap, exclude_diag=self_case)
    assert want_hist.sum() == B * N - (B if self_case else 0) and (want_key == ONES).any() and (want_key != ONES).any()
    for rows in (1, 33):                                                  # the database in chunks, the key carried across the calls
        kb, hb = _fresh(B, cap)
        for r0 in range(0, N, rows):
            key, hist = _nn(xq, xdb[r0:r0 + rows], cap, kb, hb, db_base=r0, exclude_diag=ex)
        assert np.array_equal(key, want_key) and np.array_equal(hist, want_hist), rows
    for rows in (1, 33):                                                  # the queries in chunks
        hb, keys = _i64(np.zeros(cap + 2)), []
        for r0 in range(0, B, rows):
            kq = _i64(np.full(min(rows, B - r0), -1))
            key, hist = _nn(xq[r0:r0 + rows], xdb, cap, kq, hb, q_base=r0, exclude_diag=ex)
            keys.append(key)
        assert np.array_equal(np.concatenate(keys), want_key) and np.array_equal(hist, want_hist), rows
    kb, hb = _fresh(B, cap)                                               # both cut, the chunks in another order
    for q0 in (33, 0):
        for r0 in (66, 0, 99, 33):
            if r0 < N:
                n = min(33, B - q0)
                kq = _i64(kb.cpu().numpy()[q0:q0 + n])
                key, hist = _nn(xq[q0:q0 + 33], xdb[r0:r0 + 33], cap, kq, hb, q_base=q0, db_base=r0, exclude_diag=ex)
                kb.body()[q0:q0 + n] = _dev(key.view(np.int64))
    assert np.array_equal(kb.cpu().numpy().view(np.uint64), want_key) and np.array_equal(hist, want_hist)
    from svdd_amd import quality
    for rows in (None, 7, 64):                                            # the module's chunk_rows, seeded and not
        for seed in (True, False):
            dist, idx = quality.edit_nn(xq, None if self_case else xdb, cap=cap, chunk_rows=rows, seed_hamming=seed)
            wd, wi = Q.nn_decode_ref(want_key)
            assert np.array_equal(dist.cpu().numpy(), wd) and np.array_equal(idx.cpu().numpy(), wi), (rows, seed)


# ------------------------------------------------------------------------------------------- seeding and shortcuts ----
def test_edit_nn_seeded_keys_change_nothing():
    L, B, N = 200, 12, 90
    rng = np.random.default_rng(17)
    xq, xdb = _tokens(B, L, 17), _tokens(N, L, 18)
    for i in range(0, B, 2):
        xdb[7 * i + 2] = mutate(xq[i], 2 + i, rng, L)                     # half of the queries have a near row
        xdb[7 * i + 5] = xdb[7 * i + 2]                                   # ... twice
    d = E.edit_matrix(xq, xdb)
    for cap in (20, L):
        want_key, want_hist = E.edit_nn_ref(xq, xdb, cap, d=d)
        found = want_key != ONES
        assert found.any() and (cap == L or (~found).any())
        wd = (want_key >> np.uint64(32)).astype(np.int64)
        top = np.uint64(0xFFFFFFFF)
        seeds = {"the answer": want_key,
                 "the same distance at a higher index": np.where(found, want_key | top, ONES),
                 "one above": np.where(found, ((wd + 1).astype(np.uint64) << np.uint64(32)), ONES),
                 "far above": np.full(B, np.uint64(L + 5) << np.uint64(32)),
                 "one below": np.where(found & (wd > 0), (np.maximum(wd - 1, 0).astype(np.uint64) << np.uint64(32)) | np.uint64(3), want_key)}
        for name, seed in seeds.items():
            want = E.edit_nn_ref(xq, xdb, cap, nn_key=seed, d=d)[0]
            if name != "one below" and name != "far above":
                assert np.array_equal(want, want_key), name
            key, _ = _nn(xq, xdb, cap, _i64(seed.view(np.int64)), None)   # no hist: pairs that cannot win may be left
            assert np.array_equal(key, want), (cap, name)
            key, hist = _nn(xq, xdb, cap, _i64(seed.view(np.int64)), _i64(np.zeros(cap + 2)))
            assert np.array_equal(key, want) and np.array_equal(hist, want_hist), (cap, name)     # hist: every pair in its bin
    from svdd_amd import quality
    wd, wi = Q.nn_decode_ref(E.edit_nn_ref(xq, xdb, 20, d=d)[0])
    for seed in (True, False):
        dist, idx = quality.edit_nn(_dev(xq), _dev(xdb).long(), cap=20, seed_hamming=seed)
        assert dist.dtype == torch.int32 and idx.dtype == torch.int64
        assert np.array_equal(dist.cpu().numpy(), wd) and np.array_equal(idx.cpu().numpy(), wi), seed
    dist, idx = quality.edit_nn(xq, xdb)                                  # cap None: every row gets an answer
    wd, wi = Q.nn_decode_ref(E.edit_nn_ref(xq, xdb, L, d=d)[0])
    assert (wd >= 0).all() and np.array_equal(dist.cpu().numpy(), wd) and np.array_equal(idx.cpu().numpy(), wi)
    assert np.array_equal(quality.pairwise_edit_hist(xq, xdb, cap=20).cpu().numpy(), E.edit_hist_ref(xq, xdb, 20, d=d))
    short = xdb[:30, :150]                                                # unequal lengths: no seeding, same door
    dist, idx = quality.edit_nn(xq, short, cap=60)
    wd, wi = Q.nn_decode_ref(E.edit_nn_ref(xq, short, 60)[0])
    assert np.array_equal(dist.cpu().numpy(), wd) and np.array_equal(idx.cpu().numpy(), wi)
    assert np.array_equal(quality.pairwise_edit_hist(xq[:5]).cpu().numpy(), E.edit_hist_ref(xq[:5], xq[:5], L, exclude_diag=True))


# ------------------------------------------------------------------------------------------ the point of the feature ----
@pytest.fixture(scope="module")
def shifted_batch():
    """40 training rows of 100 positions; 10 designs, five of them training rows moved by 1 .. 5 positions with random fill."""
    rng = np.random.default_rng(23)
    train = _tokens(40, 100, 23)
    x = _tokens(10, 100, 24)
    for n, s in enumerate((3, 1, 5, 2, 4)):
        x[2 * n] = np.concatenate([train[7 * n + 1][s:], rng.integers(0, 4, s).astype(np.uint8)])
    return x, train, E.edit_quality_ref(x, 10, train)


def test_shifted_training_rows_are_found(shifted_batch):
    from svdd_amd import quality
    x, train, want = shifted_batch
    ham = quality.sample_quality(x, train=train)
    assert ham["memorised_fraction"] == 0.0 and ham["novelty_nn_min"] > 50   # Hamming: ten novel designs
    assert not [k for k in ham if "edit" in k or "missed" in k]               # and sample_quality reports what it did
    assert ham == quality.sample_quality(_dev(x), train=_dev(train))
    got = quality.edit_quality(x, 10, train=train)
    assert got == want
    assert got["edit_near_train_fraction"] == 0.5 == got["hamming_missed_fraction"] and got["edit_near_batch_fraction"] == 0.0
    assert got["edit_near_train_min"] == 2                                    # twice the smallest shift
    assert quality.edit_quality(_dev(x).long(), 1, train=train) == E.edit_quality_ref(x, 1, train)
    assert quality.edit_quality(x, 10) == E.edit_quality_ref(x, 10)
    assert quality.edit_quality(x, 100, train=train[:, :80]) == E.edit_quality_ref(x, 100, train[:, :80])   # no Hamming key


def test_a_token_above_3_raises():
    from svdd_amd import ops, quality
    x = _tokens(9, 50, 3)
    bad = _dev(x).clone()
    bad[4, 4] = 4                                                         # on the device the kernel's err word speaks
    for fn in (quality.edit_nn, quality.pairwise_edit_hist, lambda t: quality.edit_quality(t, 3)):
        with pytest.raises(ops.SvddError, match="token > 3"):
            fn(bad)
    with pytest.raises(ops.SvddError, match="token > 3"):
        quality.edit_nn(_dev(x), bad.long())
    with pytest.raises(ops.SvddError, match="token > 3"):
        quality.edit_quality(_dev(x), 3, train=bad)


def test_harness_evaluate_edit_and_cli(tmp_path, shifted_batch):
    from svdd_amd import cli
    from svdd_amd.harness import BaseModel
    from svdd_amd.value_nets import RewardModel
    from tests import e2e_parity
    model, emb, head = e2e_parity.tiny_engine(load_golden("nets_tiny.npz"), 50, 4, DEV)
    reward = RewardModel(emb, head).to(DEV).eval()
    model.rng_mode, model.philox_seed = "philox", 9
    hm = BaseModel(emb, head, model, reward, batch_size=4, task="dna")
    samples = hm.controlled_decode(gen_batch_num=2, sample_M=2)[0]
    x = torch.cat(samples).cpu().numpy()
    train = _tokens(12, 50, 1)
    train[5] = np.concatenate([x[3][2:], x[3][:2]])                       # a training row that IS a design, moved by two
    rep = hm.evaluate_edit(samples, 6, train=train)
    assert rep == E.edit_quality_ref(x, 6, train) and rep["edit_near_train_fraction"] >= 1 / 8 and rep["edit_near_train_min"] <= 4
    assert hm.evaluate_edit(torch.cat(samples), 6) == E.edit_quality_ref(x, 6)
    before = ["kmer_pearsonr_valid", "diversity_mean", "diversity_nn_median", "unique_fraction", "novelty_nn_median",
              "novelty_nn_min", "memorised_fraction", "ws_scores_valid"]
    assert sorted(hm.evaluate_quality(samples, refs={"valid": train}, train=train)) == sorted(before)    # unchanged
    sets = tmp_path / "sets.npz"
    np.savez(sets, train=_tokens(12, 50, 1), test=_tokens(6, 50, 2))
    args = ["--task", "rna", "--batch_size", "2", "--sample_M", "2", "--val_batch_num", "1", "--rng", "philox"]
    path, out = cli.main("mc", args + ["--out_dir", str(tmp_path / "on"), "--eval_quality", str(sets), "--eval_edit", "5"])
    z = np.load(path)
    plain = ["kmer_pearsonr_train", "kmer_pearsonr_test", "diversity_mean", "diversity_nn_median", "unique_fraction",
             "novelty_nn_median", "novelty_nn_min", "memorised_fraction", "ws_scores_train", "ws_scores_test"]
    new = ["edit_near_batch_fraction", "edit_near_train_fraction", "edit_near_train_min", "hamming_missed_fraction"]
    assert sorted(z.files) == sorted(["baseline", "decoding"] + ["quality_" + k for k in plain + new])
    want = E.edit_quality_ref(torch.cat(out[0]).cpu().numpy(), 5, _tokens(12, 50, 1))
    assert {k: float(z["quality_" + k]) for k in new} == {k: float(v) for k, v in want.items()}
    with pytest.raises(SystemExit):
        cli.main("mc", args + ["--eval_edit", "5"])                       # refused without --eval_quality
