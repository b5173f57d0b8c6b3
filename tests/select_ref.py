"""The contract of diverse library selection (svdd_amd.quality.select_diverse) restated in numpy by brute force, the
references of its two kernels, and the planted-family data and case table that tests/test_select_cpu.py and
tests/test_select_gpu.py share. Nothing here imports the package."""
import numpy as np

INT32_MAX = 2 ** 31 - 1


def revcomp(x):
    """rc(a)[l] = 3 - a[L - 1 - l], row-wise."""
    return (3 - x.astype(np.int64))[..., ::-1]


def distances(a, b, rc):
    """a [L] against b [n, L] -> int64 [n]: the Hamming distance, with rc the smaller of that and the distance of rc(a)."""
    b = b.reshape(-1, a.shape[0])
    d = (a[None, :] != b).sum(1)
    return np.minimum(d, (revcomp(a)[None, :] != b).sum(1)) if rc else d


def order_of(scores, N):
    """Descending score, the lower index first among equal scores (-0.0 == 0.0); None: the given order."""
    return np.arange(N) if scores is None else np.argsort(-np.asarray(scores), kind="stable")


def select_ref(x, scores=None, k=None, min_dist=1, rc=False):
    """-> (picked i64 [P], rep i64 [N], rep_dist i32 [N]) by the walk of the contract, one row at a time."""
    x = np.asarray(x).astype(np.int64)
    N = x.shape[0]
    k = N if k is None else min(k, N)
    picked, rep, rep_dist = [], np.full(N, -1, np.int64), np.full(N, -1, np.int32)
    for i in order_of(scores, N):
        d = distances(x[i], x[picked], rc) if picked else np.zeros(0, np.int64)
        close = np.nonzero(d < min_dist)[0]
        if close.size:
            rep[i], rep_dist[i] = picked[close[0]], d[close[0]]
        elif len(picked) < k:
            picked.append(int(i))
            rep[i], rep_dist[i] = i, 0
    return np.asarray(picked, np.int64), rep, rep_dist


def check_selection(x, scores, k, min_dist, rc, picked, rep, rep_dist):
    """The properties of a selection, checked without the walk: the picks are pairwise >= min_dist apart and in rank order; a
    picked row represents itself; every other row that has a pick within the radius has the EARLIEST such pick as its
    representative, and that pick ranks before it (a row that was far from every pick when its turn came was picked, unless k
    picks existed, and then no pick came after it); rep = -1 only when k picks exist and none is within the radius."""
    x = np.asarray(x).astype(np.int64)
    N = x.shape[0]
    kk = N if k is None else min(k, N)
    rank = np.empty(N, np.int64)
    rank[order_of(scores, N)] = np.arange(N)
    assert len(picked) <= kk and len(set(picked.tolist())) == len(picked)
    assert (np.diff(rank[picked]) > 0).all()
    P = x[picked]
    for n, p in enumerate(picked):
        assert (distances(x[p], P[:n], rc) >= min_dist).all()
        assert rep[p] == p and rep_dist[p] == 0
    is_pick = np.zeros(N, bool)
    is_pick[picked] = True
    for i in np.nonzero(~is_pick)[0]:
        d = distances(x[i], P, rc)
        close = np.nonzero(d < min_dist)[0]
        if close.size:
            assert rep[i] == picked[close[0]] and rep_dist[i] == d[close[0]]
            # not picked although it came before that pick: impossible
            assert rank[picked[close[0]]] < rank[i]
        else:
            assert len(picked) == kk and rep[i] == -1 and rep_dist[i] == -1


def prefix_of(picked, rep, rep_dist, k):
    """The selection with limit k from the selection without: the first k picks, and every representative whose pick number is
    >= k replaced by -1."""
    N = rep.shape[0]
    number = np.full(N + 1, -1, np.int64)
    number[picked] = np.arange(len(picked))
    gone = (rep >= 0) & (number[rep] >= k)
    return picked[:k], np.where(gone, -1, rep), np.where(gone, -1, rep_dist).astype(np.int32)


def pack_ref(x):
    """svdd_pack_tokens: [N, L] tokens -> uint32 [N, ceil(L / 16)], position l in word l // 16 at bits 2 (l % 16)."""
    x = np.asarray(x).astype(np.uint32)
    N, L = x.shape
    W = (L + 15) // 16
    pad = np.zeros((N, 16 * W), np.uint32)
    pad[:, :L] = x
    return (pad.reshape(N, W, 16) << (2 * np.arange(16, dtype=np.uint32))).sum(2, dtype=np.uint32)


def distance_matrix(q, db, rc=False):
    """q [B, L], db [N, L] -> int64 [B, N] of distances(q_i, db_j)."""
    q, db = np.asarray(q).astype(np.int64), np.asarray(db).astype(np.int64)
    return np.stack([distances(a, db, rc) for a in q]) if db.shape[0] else np.zeros((q.shape[0], 0), np.int64)


def within_of(D, radius, count=None, first0=None, mask_words=None):
    """svdd_within from the distances D [B, N] -> (first i32 [B], mask u32 [B, mask_words])."""
    B, N = D.shape
    n = N if count is None else max(0, min(N, count))
    mask_words = (N + 31) // 32 if mask_words is None else mask_words
    first = np.full(B, INT32_MAX, np.int64) if first0 is None else np.asarray(first0).astype(np.int64).copy()
    bits = np.zeros((B, 32 * mask_words), bool)
    bits[:, :n] = D[:, :n] <= radius
    any_hit = bits.any(1)
    first[any_hit] = np.minimum(first[any_hit], bits[any_hit].argmax(1))
    mask = (bits.reshape(B, mask_words, 32).astype(np.uint32) << np.arange(32, dtype=np.uint32)).sum(2, dtype=np.uint32)
    return first.astype(np.int32), mask


def within_ref(q, db, radius, rc=False, count=None, first0=None, mask_words=None):
    """svdd_within on unpacked tokens q [B, L], db [N, L] -> (first i32 [B], mask u32 [B, mask_words])."""
    return within_of(distance_matrix(q, db, rc), radius, count, first0, mask_words)


def greedy_pick_ref(close, first, k, count, cap):
    """svdd_greedy_pick on an arbitrary bit matrix close [T, T] bool (only j > i of row i matters) and first [T] (INT32_MAX: none)
    -> (rep_pick i32 [T], the block rows picked in order, the new count)."""
    T = close.shape[0]
    rep_pick, mine, count0 = np.full(T, -1, np.int32), np.empty(T, np.int64), count
    limit = min(k, cap)
    for i in range(T):
        if first is not None and first[i] != INT32_MAX:
            rep_pick[i] = first[i]
            continue
        sup = np.nonzero(close[mine[:count - count0], i])[0]                   # this block's picks so far that row i is close to
        if sup.size:
            rep_pick[i] = count0 + sup[0]
        elif count < limit:
            rep_pick[i] = count
            mine[count - count0] = i
            count += 1
    return rep_pick, mine[:count - count0].tolist(), count


def planted(N, L, F, max_sub, seed, copy_share=0.15, rc_share=0.25):
    """N rows in F planted families: a row is a random founder with 0 .. max_sub substitutions (a share of exact copies), a share
    of the rows reverse-complemented -> (x u8 [N, L], scores f32 [N] with many ties). Random rows alone would sit about 0.75 L
    apart, and nothing would ever be suppressed."""
    rng = np.random.default_rng(seed)
    founders = rng.integers(0, 4, (F, L))
    x = np.empty((N, L), np.int64)
    for i in range(N):
        row = founders[rng.integers(F)].copy()
        if rng.random() >= copy_share:
            ns = min(int(rng.integers(0, max_sub + 1)), L)
            pos = rng.choice(L, ns, replace=False)
            row[pos] = (row[pos] + rng.integers(1, 4, ns)) % 4
        if rng.random() < rc_share:
            row = 3 - row[::-1]
        x[i] = row
    scores = (rng.integers(0, max(2, N // 3), N) / 4.0).astype(np.float32)
    return x.astype(np.uint8), scores


# name -> (N, L, F, max_sub, min_dist, block_rows, seed): tests/test_select_cpu.py asserts on the reference alone that every one of
# these has 1 < picks < N, a row suppressed by a pick of its own block and one by a pick of an earlier block at these block_rows,
# with revcomp a row that is within the radius of its representative through the reverse strand only, and tied scores
CASES = {
    "odd": (257, 33, 8, 6, 5, 64, 1),
    "gosai": (300, 200, 12, 12, 10, 64, 2),
    "blocks": (1000, 200, 40, 12, 10, 256, 3),
    "word": (200, 16, 6, 2, 2, 32, 4),
    "long": (300, 1024, 10, 20, 16, 64, 5),
}


def case(name):
    N, L, F, max_sub, min_dist, T, seed = CASES[name]
    x, scores = planted(N, L, F, max_sub, seed)
    return x, scores, min_dist, T


def degenerate(name):
    """The cases the non-vacuity conditions cannot hold for -> (x, scores, min_dist)."""
    rng = np.random.default_rng(7)
    if name == "L1":
        return rng.integers(0, 4, (10, 1)).astype(np.uint8), rng.random(10).astype(np.float32), 1
    if name == "N1":
        return rng.integers(0, 4, (1, 40)).astype(np.uint8), np.zeros(1, np.float32), 3
    if name == "equal":
        return np.repeat(rng.integers(0, 4, (1, 50)), 20, 0).astype(np.uint8), rng.random(20).astype(np.float32), 4
    raise KeyError(name)


DEGENERATE = ("L1", "N1", "equal")
