"""The contract of diverse library selection under a minimum EDIT distance (svdd_amd.quality.select_diverse_edit)
restated in numpy: the distances are tests/edit_ref.py's Wagner-Fischer table (nothing bit-parallel), the walk and the property
check are tests/select_ref.py's with a precomputed distance matrix in place of the Hamming distance, and the kernel references
(within_of, greedy_pick_ref) are select_ref's own, which take any distance or bit matrix. Also the planted data with indels and
shifts and the case table that tests/test_select_edit_cpu.py and tests/test_select_edit_gpu.py share. Nothing here imports the
package."""
import functools
import hashlib
import os

import numpy as np

from tests import select_ref as S
from tests.edit_ref import edit_matrix

INT32_MAX = S.INT32_MAX


def distance_matrix(q, db, rc=False):
    """q [B, Lq], db [N, Ld] -> int64 [B, N]: the Levenshtein distance, with rc the smaller of that and the distance of rc(q_i)."""
    q, db = np.asarray(q).astype(np.int64), np.asarray(db).astype(np.int64)
    d = edit_matrix(q, db)
    return np.minimum(d, edit_matrix(S.revcomp(q), db)) if rc else d


def hamming_matrix(q, db, rc=False):
    """The same pairs by Hamming distance (select_ref.distance_matrix): what the edit distance is compared with."""
    return S.distance_matrix(q, db, rc)


def select_of(D, scores=None, k=None, min_dist=1):
    """select_ref.select_ref on a precomputed distance matrix D [N, N] -> (picked i64 [P], rep i64 [N], rep_dist i32 [N])."""
    N = D.shape[0]
    k = N if k is None else min(k, N)
    picked, rep, rep_dist = [], np.full(N, -1, np.int64), np.full(N, -1, np.int32)
    for i in S.order_of(scores, N):
        d = D[i, picked] if picked else np.zeros(0, np.int64)
        close = np.nonzero(d < min_dist)[0]
        if close.size:
            rep[i], rep_dist[i] = picked[close[0]], d[close[0]]
        elif len(picked) < k:
            picked.append(int(i))
            rep[i], rep_dist[i] = i, 0
    return np.asarray(picked, np.int64), rep, rep_dist


def check_selection(D, scores, k, min_dist, picked, rep, rep_dist):
    """select_ref.check_selection on a precomputed distance matrix: the properties of a selection, checked without the walk."""
    N = D.shape[0]
    kk = N if k is None else min(k, N)
    rank = np.empty(N, np.int64)
    rank[S.order_of(scores, N)] = np.arange(N)
    assert len(picked) <= kk and len(set(picked.tolist())) == len(picked)
    assert (np.diff(rank[picked]) > 0).all()
    for n, p in enumerate(picked):
        assert (D[p, picked[:n]] >= min_dist).all()
        assert rep[p] == p and rep_dist[p] == 0
    is_pick = np.zeros(N, bool)
    is_pick[picked] = True
    for i in np.nonzero(~is_pick)[0]:
        d = D[i, picked]
        close = np.nonzero(d < min_dist)[0]
        if close.size:
            assert rep[i] == picked[close[0]] and rep_dist[i] == d[close[0]]
            assert rank[picked[close[0]]] < rank[i]                           # not picked although it came before that pick: impossible
        else:
            assert len(picked) == kk and rep[i] == -1 and rep_dist[i] == -1


def planted_indel(N, L, F, max_edit, seed, copy_share=0.15, rc_share=0.25, shift_share=0.2):
    """N rows in F planted families -> (x u8 [N, L], scores f32 [N] with many ties). A row is a random founder that is an exact copy
    (copy_share), a pure shift by 1 .. 3 at either end with the freed positions drawn at random (shift_share), or carries
    0 .. max_edit random edits, each a substitution, an insertion or a deletion at a random position, and is then cut or padded
    with random tokens back to L; a share of the rows is reverse-complemented."""
    rng = np.random.default_rng(seed)
    founders = rng.integers(0, 4, (F, L))
    x = np.empty((N, L), np.int64)
    for i in range(N):
        row = founders[rng.integers(F)].copy()
        u = rng.random()
        if u < copy_share:
            pass
        elif u < copy_share + shift_share:
            s = min(int(rng.integers(1, 4)), L)
            fill = rng.integers(0, 4, s)
            row = np.concatenate([row[s:], fill]) if rng.random() < 0.5 else np.concatenate([fill, row[:L - s]])
        else:
            seq = row.tolist()
            for _ in range(int(rng.integers(0, max_edit + 1))):
                kind = int(rng.integers(3))
                if kind == 0 and seq:
                    pos = int(rng.integers(len(seq)))
                    seq[pos] = (seq[pos] + int(rng.integers(1, 4))) % 4
                elif kind == 1:
                    seq.insert(int(rng.integers(len(seq) + 1)), int(rng.integers(4)))
                elif seq:
                    del seq[int(rng.integers(len(seq)))]
            seq = seq[:L] + rng.integers(0, 4, max(0, L - len(seq))).tolist()
            row = np.asarray(seq, np.int64)
        if rng.random() < rc_share:
            row = 3 - row[::-1]
        x[i] = row
    scores = (rng.integers(0, max(2, N // 3), N) / 4.0).astype(np.float32)
    return x.astype(np.uint8), scores


# name -> (N, L, F, max_edit, min_dist, block_rows, seed): tests/test_select_edit_cpu.py asserts on the reference alone that every
# one of these has 1 < picks < N, a row suppressed by a pick of its own block and one by a pick of an earlier block, a suppressed
# row that is at least min_dist from its representative by HAMMING distance (represented through an indel only), with revcomp a row
# within the radius through the reverse strand only, pairs at exactly min_dist - 1 and min_dist, other picks than the Hamming
# selection's, and tied scores. Small N at long L: the numpy table costs N^2 L^2.
CASES = {
    "odd": (257, 33, 8, 4, 5, 64, 1),
    "word": (200, 16, 6, 2, 3, 32, 4),
    "planes": (260, 65, 8, 5, 6, 64, 6),
    "gosai": (100, 200, 5, 8, 10, 32, 2),
    "wt7": (64, 224, 4, 8, 10, 16, 7),
    "wt8": (64, 225, 4, 8, 10, 16, 8),
    "long": (24, 1024, 2, 12, 16, 8, 10),       # seeds 5 and 9 have no (row, pick) pair at exactly min_dist - 1
}


def case(name):
    N, L, F, max_edit, min_dist, T, seed = CASES[name]
    x, scores = planted_indel(N, L, F, max_edit, seed)
    return x, scores, min_dist, T


@functools.lru_cache(maxsize=None)
def case_distances(name, rc):
    """The case's distance matrix D [N, N] (the slow part: computed once per process and shared; do not write to it)."""
    x = (case(name) if name in CASES else S.degenerate(name))[0]
    D = distance_matrix(x, x, rc)
    D.setflags(write=False)
    return D


# ------------------------------------------------------------------------------ the data of the raw kernel tests ----
# Every class of plane words (1, 2, 4, 7, 8, 16, 32) and every edge of a 32-bit plane word and of a 16-token packed word.
KERNEL_LS = (1, 16, 17, 32, 33, 64, 65, 128, 129, 200, 224, 225, 257, 1024)
SIZES = ((1, 1), (63, 65), (64, 64), (65, 63), (257, 257), (1, 257), (257, 1))       # (B, N) at L <= 65: select_ref's list
LONG_SIZES = ((65, 63), (1, 130))                                                    # at L >= 128: the numpy table costs B N L^2
GOLDEN_MIN_L = 64                  # from here on the tables are recorded (tests/golden/make_golden_select_edit.py): minutes of numpy
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g41_select_edit.npz")


def kernel_sizes(L):
    return SIZES if L <= 65 else LONG_SIZES


def _nominal_radius(L):
    return min(max(1, L // 8), L - 1)


@functools.lru_cache(maxsize=None)
def mid_radius(L):
    """About L / 8: the radius at which the planted rows have hits, near misses and hits that Hamming distance does not see. From
    L = 16 on it is the value nearest to L / 8 at which the tables of the L's cases hold a pair at exactly r and one at exactly
    r + 1 edits, on one strand and on both: the comparison d <= radius is then exercised from both sides. (It is read off the
    reference's tables, never off the kernel.)"""
    want = _nominal_radius(L)
    if L < 16:
        return want
    tables = [kernel_case(L, si)[2] for si in range(len(kernel_sizes(L)))]
    has = lambda v: all(any((D[rc] == v).any() for D in tables) for rc in (False, True))      # noqa: E731
    for delta in range(want):
        for r in (want - delta, want + delta):
            if 1 <= r <= L - 2 and has(r) and has(r + 1):
                return r
    raise AssertionError(f"L = {L}: no radius near {want} with pairs at r and r + 1")


def kernel_rows(L, si):
    """Queries and database of the (B, N) = kernel_sizes(L)[si] case: planted rows over the SAME three founders on both sides,
    with edit counts whose sums straddle L / 8 -> (xq u8 [B, L], xdb u8 [N, L])."""
    B, N = kernel_sizes(L)[si]
    max_edit = 2 * _nominal_radius(L) // 3 + 1
    xq = planted_indel(B, L, 3, max_edit, 100 + si, copy_share=0.2, rc_share=0.3, shift_share=0.25)[0]
    xdb = planted_indel(N, L, 3, max_edit, 100 + si, copy_share=0.2, rc_share=0.3, shift_share=0.25)[0][::-1].copy()
    return xq, xdb


@functools.lru_cache(maxsize=None)
def kernel_case(L, si):
    """-> (xq, xdb, {False: D one strand, True: D both strands}) of kernel_rows(L, si); computed once per process, recorded for
    L >= GOLDEN_MIN_L. Do not write to them."""
    if L >= GOLDEN_MIN_L:
        z = np.load(GOLDEN)
        xq, xdb, D = z[f"xq_{L}_{si}"], z[f"xdb_{L}_{si}"], {rc: z[f"d{int(rc)}_{L}_{si}"].astype(np.int64) for rc in (False, True)}
    else:
        xq, xdb = kernel_rows(L, si)
        D = {rc: distance_matrix(xq, xdb, rc) for rc in (False, True)}
    for a in (xq, xdb, D[False], D[True]):
        a.setflags(write=False)
    return xq, xdb, D


def kernel_case_is_not_vacuous(L):
    """What the mid radius of the L's cases must exercise (L >= 16), over all its sizes together: a hit that Hamming distance does
    not see, a pair at exactly the radius and one at exactly radius + 1, a hit through the reverse strand only."""
    r = mid_radius(L)
    seen = np.zeros(4, bool)
    for si in range(len(kernel_sizes(L))):
        xq, xdb, D = kernel_case(L, si)
        seen |= [((D[False] <= r) & (S.distance_matrix(xq, xdb) > r)).any(), (D[True] == r).any() or (D[False] == r).any(),
                 (D[True] == r + 1).any() or (D[False] == r + 1).any(), ((D[True] <= r) & (D[False] > r)).any()]
    return seen.tolist()


# many segments: B = 260 queries of L = 16 against N = 20,000 rows with planted copies and shifts of the queries, radius 2
SEG_B, SEG_N, SEG_L, SEG_RADIUS = 260, 20000, 16, 2


def segment_rows():
    rng = np.random.default_rng(11)
    xq, xdb = rng.integers(0, 4, (SEG_B, SEG_L)).astype(np.uint8), rng.integers(0, 4, (SEG_N, SEG_L)).astype(np.uint8)
    at, src = rng.integers(0, SEG_N, 3000), rng.integers(0, SEG_B, 3000)
    xdb[at[:1000]] = xq[src[:1000]]                                                              # exact copies of the queries
    xdb[at[1000:2000], :-1] = xq[src[1000:2000], 1:]                                             # shifted by one: 2 edits at most
    xdb[at[2000:], 2:] = xq[src[2000:], :-2]                                                     # shifted by two: 4 edits at most
    return xq, xdb


def segment_hits(xq, xdb, chunk=1000):
    """bool [B, N]: the pairs within SEG_RADIUS, the table computed in database chunks."""
    return np.concatenate([edit_matrix(xq, xdb[c:c + chunk]) <= SEG_RADIUS for c in range(0, xdb.shape[0], chunk)], 1)


@functools.lru_cache(maxsize=None)
def segment_case():
    """-> (xq, xdb, hits bool [B, N]) with the hits as recorded in the golden file (40 s of numpy)."""
    z = np.load(GOLDEN)
    xq, xdb = segment_rows()
    hits = np.zeros((SEG_B, SEG_N), bool)
    hits[z["seg_hit_i"], z["seg_hit_j"]] = True
    assert z["seg_xq"].tobytes() == xq.tobytes() and z["seg_xdb_sha1"].item() == hashlib.sha1(xdb.tobytes()).hexdigest()
    return xq, xdb, hits
