"""Quality of a decoded batch AS A SET: what the reference reports after every sampling run
(diffusion_gosai.py on_validation_epoch_end: cal_kmer_pearsonr, cal_wasserstein_distance, oracle.get_wasserstein_dist) plus the two
standard companions of a reward table that it does not have, diversity and novelty.

  kmer_counts / kmer_pearsonr      k-mer spectrum on the device (svdd_kmer_counts), Pearson r by the reference's compare_kmer rule
  pack_tokens / hamming_nn / pairwise_hamming_hist
                                    Hamming distances on 2-bit-packed rows (svdd_pack_tokens, svdd_hamming_nn): exact integers,
                                    independent of every chunking
  edit_nn / pairwise_edit_hist / edit_quality
                                    Levenshtein distances on the same packed rows (svdd_edit_nn): the near copies that
                                    Hamming distance cannot see (a shifted training row)
  select_diverse / library_quality  greedy selection under a minimum Hamming distance (svdd_within, svdd_greedy_pick): the
                                    best rows that are no near copies of each other, and the families of the set
  select_diverse_edit / library_quality_edit / edit_distance
                                    the same selection under a minimum EDIT distance (svdd_edit_within, svdd_edit_pairs):
                                    a design and its shifted copy are one family; and the row-wise Levenshtein distance
  wasserstein_1d / frechet_distance host-level float64 (torch), no kernel
  sample_quality                    the flat report

Token inputs are [N, L] integer tensors (any integer dtype; a CPU tensor or a numpy array is checked on the host and moved to the
GPU). The kernels have no CPU fallback."""
import collections
import math

import numpy as np
import torch

from . import ops
from .ops import SvddError

HAMMING_CHUNK_ROWS = 1 << 20             # database rows per svdd_hamming_nn call (any value gives the same result)
EDIT_CHUNK_ROWS = 1 << 20                # database rows per svdd_edit_nn call (likewise)
KMER_CHUNK_ROWS = 1 << 22
SELECT_BLOCK_ROWS = 4096                 # rows per block of select_diverse's walk (likewise; measured in profiles/select_time.txt)
SELECT_EDIT_BLOCK_ROWS = 4096            # ... of select_diverse_edit's (likewise; measured in profiles/select_edit_time.txt)


def _checked(x, name, max_token):
    """Shape and dtype of a token set, and for host data its values (device data: the kernels flag them) -> an integer tensor."""
    if isinstance(x, np.ndarray):
        if x.dtype.kind not in "iu":
            raise ValueError(f"{name} must hold integer tokens, got {x.dtype}")
        x = torch.from_numpy(np.ascontiguousarray(x).astype(np.int64, copy=False))
    if not isinstance(x, torch.Tensor) or x.dtype not in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64):
        raise ValueError(f"{name} must be an integer tensor of tokens, got {getattr(x, 'dtype', type(x))}")
    if x.dim() != 2 or x.numel() == 0:
        raise ValueError(f"{name} must be a non-empty [N, L] tensor, got {tuple(x.shape)}")
    if not x.is_cuda and (int(x.min()) < 0 or int(x.max()) > max_token):
        raise ValueError(f"{name} holds a token outside 0 .. {max_token}")
    return x


def _on_device(x, name):
    """A checked token set -> u8 [N, L] contiguous on the GPU."""
    if not x.is_cuda:
        if not torch.cuda.is_available():
            raise SvddError(f"{name}: the quality kernels run on the GPU (the SVDD hot path has no CPU fallback)")
        x = x.to(torch.uint8).cuda()
    elif x.dtype != torch.uint8:
        x = torch.where((x < 0) | (x > 255), torch.full_like(x, 255), x).to(torch.uint8)     # out of range stays out of range
    return x.contiguous()


def _tokens(x, name, max_token):
    return _on_device(_checked(x, name, max_token), name)


def _chunk_rows(chunk_rows, default):
    if chunk_rows is None:
        return default
    if not isinstance(chunk_rows, int) or isinstance(chunk_rows, bool) or chunk_rows <= 0:
        raise ValueError(f"chunk_rows = {chunk_rows!r}: expected a positive int or None")
    return chunk_rows


def _check_k(k):
    if not isinstance(k, int) or isinstance(k, bool) or not 1 <= k <= ops.KMER_MAX_K:
        raise ValueError(f"k = {k!r}: expected an int in 1 .. {ops.KMER_MAX_K}")


# ----------------------------------------------------------------------------------------------------- k-mer spectra ----
def kmer_counts(x, k=3, chunk_rows=None):
    """-> (counts i64 [4^k] on the device, skipped int). Bin = the lexicographic rank of the k-mer's ACGT string (reference
    oracle.count_kmers' dictionary as a vector); a window that holds a token > 3 (MASK) is not counted but counted in skipped.
    chunk_rows: rows per launch (the counts are integers: every chunking gives the same result)."""
    _check_k(k)
    rows = _chunk_rows(chunk_rows, KMER_CHUNK_ROWS)
    x = _tokens(x, "x", 255)
    counts = torch.zeros(4 ** k, dtype=torch.int64, device=x.device)
    skipped = torch.zeros(1, dtype=torch.int64, device=x.device)
    for r0 in range(0, x.shape[0], rows):
        ops.kmer_counts(x[r0:r0 + rows], k, counts, skipped)
    return counts, int(skipped[0])


def _pearson_union(c1, c2):
    """Pearson r of two count vectors over the bins that are non-zero in either (float64 on the host); NaN when fewer than two
    bins are left or a side has no variance."""
    keep = (c1 != 0) | (c2 != 0)
    a, b = c1[keep].double(), c2[keep].double()
    if a.numel() < 2:
        return float("nan")
    a, b = a - a.mean(), b - b.mean()
    den = math.sqrt(float((a * a).sum()) * float((b * b).sum()))
    return float((a * b).sum()) / den if den > 0 else float("nan")


def _ref_counts(ref, k, name="ref"):
    """ref: tokens [N', L'] or a ready count vector [4^k] -> i64 [4^k] on the host."""
    if isinstance(ref, np.ndarray):
        ref = torch.from_numpy(np.ascontiguousarray(ref))
    if isinstance(ref, torch.Tensor) and ref.dim() == 1:
        if ref.numel() != 4 ** k or ref.dtype.is_floating_point and bool((ref != ref.round()).any()):
            raise ValueError(f"{name}: a count vector must hold 4^k = {4 ** k} integers, got {tuple(ref.shape)} {ref.dtype}")
        return ref.detach().cpu().to(torch.int64)
    return kmer_counts(ref, k)[0].cpu()


def kmer_pearsonr(x, ref, k=3):
    """Pearson correlation of the k-mer spectra of x and ref (tokens [N', L'] or a count vector [4^k]) by the reference's
    Diffusion.compare_kmer rule: over the union of the k-mers present in either set; a bin that is zero in both is left out.
    The reference scales one side by n2 / n1 first: a positive factor, which does not change r, so it is skipped.
    Float64 on the host from the exact counts. < 2 bins in the union or zero variance on a side: NaN."""
    _check_k(k)
    return _pearson_union(kmer_counts(x, k)[0].cpu(), _ref_counts(ref, k))


# ------------------------------------------------------------------------------------------------- Hamming distances ----
def pack_tokens(x):
    """x [N, L] tokens 0..3, L <= 1024 -> int32 [N, ceil(L / 16)]: 2 bits per token, 16 per word. Raises on a token > 3."""
    x = _checked(x, "x", 3)
    if x.shape[1] > ops.PACK_MAX_L:
        raise ValueError(f"L = {x.shape[1]} > {ops.PACK_MAX_L}")
    return ops.pack_tokens(_on_device(x, "x"))


def _pair(x, db):
    x = _checked(x, "x", 3)
    xd = None if db is None else _checked(db, "db", 3)
    if xd is not None and xd.shape[1] != x.shape[1]:
        raise ValueError(f"x and db must have one length, got {x.shape[1]} and {xd.shape[1]}")
    if x.shape[1] > ops.PACK_MAX_L:
        raise ValueError(f"L = {x.shape[1]} > {ops.PACK_MAX_L}")
    return _on_device(x, "x"), None if xd is None else _on_device(xd, "db")


def _hamming(x, db, chunk_rows, want_key, want_hist):
    """-> (nn_key i64 [B] | None, hist i64 [L + 1] | None) of x against db (None: x against itself without the diagonal)."""
    rows = _chunk_rows(chunk_rows, HAMMING_CHUNK_ROWS)
    x, xd = _pair(x, db)
    B, L = x.shape
    err = torch.zeros(1, dtype=torch.int32, device=x.device)
    q = ops.pack_tokens(x, err=err)
    key = torch.full((B,), ops.NN_KEY_INIT, dtype=torch.int64, device=x.device) if want_key else None
    hist = torch.zeros(L + 1, dtype=torch.int64, device=x.device) if want_hist else None
    src = x if xd is None else xd
    for r0 in range(0, src.shape[0], rows):
        d = q[r0:r0 + rows] if xd is None else ops.pack_tokens(xd[r0:r0 + rows], err=err)
        ops.hamming_nn(q, d, L, key, hist, db_base=r0, exclude_diag=xd is None)
    ops.check_pack_err(err)
    return key, hist


def hamming_nn(x, db=None, chunk_rows=None):
    """Nearest neighbour of every row of x in db by Hamming distance -> (dist i32 [B], idx i64 [B]); among equally near rows the
    lowest index. db None: x against itself with the diagonal excluded (a one-row set gives (-1, -1)). chunk_rows: database rows
    per launch (every value gives the same result)."""
    return ops.nn_decode(_hamming(x, db, chunk_rows, True, False)[0])


def pairwise_hamming_hist(x, db=None):
    """i64 [L + 1]: the number of pairs (row of x, row of db) at each Hamming distance; db None: the ordered pairs i != j of x."""
    return _hamming(x, db, None, False, True)[1]


# ---------------------------------------------------------------------------------------------------- edit distances ----
def _check_cap(cap, Lq, Ld, name="cap"):
    if cap is None:
        return max(Lq, Ld)
    if not isinstance(cap, int) or isinstance(cap, bool) or not 0 <= cap <= max(Lq, Ld):
        raise ValueError(f"{name} = {cap!r}: expected an int in 0 .. max(Lq, Ld) = {max(Lq, Ld)} or None")
    return cap


def _edit(x, db, cap, chunk_rows, want_key, want_hist, seed_hamming=True):
    """-> (nn_key i64 [B] | None, hist i64 [cap + 2] | None) of x against db (None: x against itself without the diagonal) by
    Levenshtein distance. The two sets may have different lengths."""
    rows = _chunk_rows(chunk_rows, EDIT_CHUNK_ROWS)
    x = _checked(x, "x", 3)
    xd = None if db is None else _checked(db, "db", 3)
    Lq, Ld = x.shape[1], x.shape[1] if xd is None else xd.shape[1]
    if max(Lq, Ld) > ops.PACK_MAX_L:
        raise ValueError(f"L = {max(Lq, Ld)} > {ops.PACK_MAX_L}")
    cap = _check_cap(cap, Lq, Ld)
    x, xd = _on_device(x, "x"), None if xd is None else _on_device(xd, "db")
    B = x.shape[0]
    err = torch.zeros(1, dtype=torch.int32, device=x.device)
    q = ops.pack_tokens(x, err=err)
    src = x if xd is None else xd
    chunks = [(r0, q[r0:r0 + rows] if xd is None else ops.pack_tokens(xd[r0:r0 + rows], err=err)) for r0 in range(0, src.shape[0], rows)]
    key = torch.full((B,), ops.NN_KEY_INIT, dtype=torch.int64, device=x.device) if want_key else None
    hist = torch.zeros(cap + 2, dtype=torch.int64, device=x.device) if want_hist else None
    if want_key and not want_hist and seed_hamming and Lq == Ld:
        # the Hamming neighbour is an upper bound (edit distance <= Hamming distance of the same pair): a seed within cap lets the
        # edit pass leave every pair that cannot beat it
        seed = torch.full_like(key, ops.NN_KEY_INIT)
        for r0, d in chunks:
            ops.hamming_nn(q, d, Lq, seed, None, db_base=r0, exclude_diag=xd is None)
        key = torch.where((seed != ops.NN_KEY_INIT) & ((seed >> 32) <= cap), seed, key)
    for r0, d in chunks:
        ops.edit_nn(q, d, Lq, Ld, cap, key, hist, db_base=r0, exclude_diag=xd is None)
    ops.check_pack_err(err)
    return key, hist


def edit_nn(x, db=None, cap=None, chunk_rows=None, seed_hamming=True):
    """Nearest neighbour of every row of x in db by Levenshtein distance (substitution, insertion, deletion: 1 each; global) within
    cap edits -> (dist i32 [B], idx i64 [B]); among equally near rows the lowest index, (-1, -1) where no row is within cap.
    db None: x against itself with the diagonal excluded. cap None: max(Lq, Ld), so every row gets an answer. x and db may have
    different lengths. chunk_rows: database rows per launch. seed_hamming (equal lengths): start from one Hamming pass, whose
    neighbour bounds the edit distance from above. Neither changes the result."""
    return ops.nn_decode(_edit(x, db, cap, chunk_rows, True, False, seed_hamming)[0])


def pairwise_edit_hist(x, db=None, cap=None):
    """i64 [cap + 2]: the number of pairs (row of x, row of db) at each Levenshtein distance 0 .. cap, and in the last bin the pairs
    beyond cap; db None: the ordered pairs i != j of x. cap None: max(Lq, Ld) (the last bin is then 0)."""
    return _edit(x, db, cap, None, False, True)[1]


def edit_quality(x, edit_cap, train=None):
    """The near-copy report sample_quality's Hamming keys cannot give (a training row shifted by three bases is 6 edits away and
    about 0.75 L by Hamming) -> a flat dict, k = edit_cap:
      edit_near_batch_fraction   the share of designs with ANOTHER design within k edits
      edit_near_train_fraction / edit_near_train_min   with train [N, L']: the share of designs with a training row within k
                                 edits, and the smallest such distance (-1 if none)
      hamming_missed_fraction    with train of the designs' length: the share of designs with a training row within k edits whose
                                 nearest training row by Hamming is farther than k (the designs the Hamming report calls novel)"""
    x = _checked(x, "x", 3)
    train = None if train is None else _checked(train, "train", 3)
    B, L = x.shape
    if edit_cap is None or _check_cap(edit_cap, L, L if train is None else train.shape[1], "edit_cap") != edit_cap:
        raise ValueError("edit_cap = None: expected an int in 0 .. max(Lq, Ld)")
    x = _on_device(x, "x")
    out = {}
    dist, _ = ops.nn_decode(_edit(x, None, min(edit_cap, L), None, True, False)[0])      # two rows of length L: at most L edits
    out["edit_near_batch_fraction"] = int((dist >= 0).sum()) / B
    if train is not None:
        train = _on_device(train, "train")
        dist, _ = ops.nn_decode(_edit(x, train, edit_cap, None, True, False)[0])
        near = dist >= 0
        out["edit_near_train_fraction"] = int(near.sum()) / B
        out["edit_near_train_min"] = int(dist[near].min()) if bool(near.any()) else -1
        if train.shape[1] == L:
            hd, _ = hamming_nn(x, train)
            out["hamming_missed_fraction"] = int((near & (hd > edit_cap)).sum()) / B
    return out


# ------------------------------------------------------------------------------------------- diverse library selection ----
Selection = collections.namedtuple("Selection", ["picked", "rep", "rep_dist"])


def _check_select(x, scores, k, min_dist, block_rows):
    """The host-side checks of select_diverse, before anything is launched -> (tokens, scores | None, k | None, rows per block)."""
    x = _checked(x, "x", 3)
    N, L = x.shape
    if L > ops.PACK_MAX_L:
        raise ValueError(f"L = {L} > {ops.PACK_MAX_L}")
    if k is not None and (not isinstance(k, int) or isinstance(k, bool) or k < 1):
        raise ValueError(f"k = {k!r}: expected an int >= 1 or None")
    if not isinstance(min_dist, int) or isinstance(min_dist, bool) or not 1 <= min_dist <= L:
        raise ValueError(f"min_dist = {min_dist!r}: expected an int in 1 .. L = {L}")
    if block_rows is not None and (not isinstance(block_rows, int) or isinstance(block_rows, bool)
                                   or not 1 <= block_rows <= ops.PICK_MAX_ROWS):
        raise ValueError(f"block_rows = {block_rows!r}: expected an int in 1 .. {ops.PICK_MAX_ROWS} or None")
    if scores is not None:
        if isinstance(scores, np.ndarray):
            scores = torch.from_numpy(np.ascontiguousarray(scores))
        if not isinstance(scores, torch.Tensor) or not scores.dtype.is_floating_point or tuple(scores.shape) != (N,):
            raise ValueError(f"scores must be a float tensor [{N}] or None, got {getattr(scores, 'dtype', type(scores))} "
                             f"{tuple(getattr(scores, 'shape', ()))}")
        if bool(torch.isnan(scores).any()):
            raise ValueError("scores holds a NaN: the order of the walk would be undefined")
    return x, scores, k, SELECT_BLOCK_ROWS if block_rows is None else block_rows


def _revcomp(x):
    return (3 - x).flip(1)


def _greedy_walk(x, scores, k, T, hits_of):
    """The walk that both metrics share: rank the rows, pack them, and per block of T rows in rank order mark the rows that an
    earlier block's pick settles (`first`), build the block's own bit matrix, and let svdd_greedy_pick walk it.
    hits_of(order, rows, err), rows = the packed rows in rank order -> hits(r0, r1, db, **outputs): the metric's within-radius
    kernel with the ranked rows r0 .. r1 as queries (db_count / first / mask as ops.within's).
    -> (packed rows in the GIVEN order, picked i64 [P], rep i64 [N])."""
    N, L = x.shape
    dev = x.device
    order = torch.arange(N, device=dev) if scores is None else torch.sort(scores.to(dev), descending=True, stable=True).indices
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    packed = ops.pack_tokens(x, err=err)
    rows = packed[order].contiguous()
    hits = hits_of(order, rows, err)
    cap = N if k is None else min(k, N)
    W = rows.shape[1]
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    reps = torch.empty((cap, W), dtype=torch.int32, device=dev)
    picked_rank = torch.empty(cap, dtype=torch.int32, device=dev)
    first = torch.full((N,), ops.FIRST_INIT, dtype=torch.int32, device=dev)
    rep_pick = torch.empty(N, dtype=torch.int32, device=dev)
    mask = torch.empty((min(T, N), (min(T, N) + 31) // 32), dtype=torch.int32, device=dev)
    for r0 in range(0, N, T):                                     # no host synchronisation in here: the number of picks is `count`
        r1 = min(r0 + T, N)
        blk = rows[r0:r1]
        if r0:
            hits(r0, r1, reps[:min(cap, r0)], db_count=count, first=first[r0:r1])
        hits(r0, r1, blk, mask=mask[:r1 - r0])
        ops.greedy_pick(mask[:r1 - r0], first[r0:r1] if r0 else None, blk, L, r0, cap, count, reps, picked_rank, rep_pick[r0:r1])
    ops.check_pack_err(err)
    picked = order[picked_rank[:int(count[0])].long()]
    rep = torch.empty(N, dtype=torch.int64, device=dev)
    rep[order] = torch.where(rep_pick >= 0, picked[rep_pick.clamp(min=0).long()], torch.full_like(rep_pick, -1, dtype=torch.int64))
    return packed, picked, rep


def select_diverse(x, scores=None, k=None, min_dist=1, revcomp=False, block_rows=None):
    """Greedy selection under a minimum distance: walk the rows of x [N, L] (tokens 0..3) from the highest score down
    (equal scores: the lower index first; scores None: the given order) and pick a row when it is at least min_dist (1 .. L) away
    from every row picked so far, until k rows are picked (None: no limit). The distance is the Hamming distance; with revcomp the
    smaller of that and the distance to the reverse complement. -> Selection(picked, rep, rep_dist) on the device:
      picked   i64 [P]  the picked rows in pick order
      rep      i64 [N]  a row's representative: itself if it is picked, else the EARLIEST pick closer than min_dist, else -1 (a
                        row that is far from every pick and came when k picks existed; never with k None)
      rep_dist i32 [N]  the distance to the representative (0 for a pick, -1 where rep is -1)
    min_dist = 1 removes exact duplicates. The first k picks of a run without limit are the run with k (the prefix property).
    block_rows (1 .. 4096): the rows per block of the walk, a tuning knob only: every value gives the same result."""
    x, scores, k, T = _check_select(x, scores, k, min_dist, block_rows)
    x = _on_device(x, "x")
    N, L = x.shape
    dev = x.device

    def hits_of(order, rows, err):
        rows_rc = ops.pack_tokens(_revcomp(x).contiguous(), err=err)[order].contiguous() if revcomp else None
        return lambda r0, r1, db, **out: ops.within(rows[r0:r1], db, L, min_dist - 1,
                                                    q_rc=None if rows_rc is None else rows_rc[r0:r1], **out)
    _, picked, rep = _greedy_walk(x, scores, k, T, hits_of)
    # a row against its ONE representative on the unpacked tokens: O(N L), not hot
    rep_dist = torch.full((N,), -1, dtype=torch.int32, device=dev)
    for c0 in range(0, N, 1 << 16):
        r = rep[c0:c0 + (1 << 16)]
        a, b = x[c0:c0 + (1 << 16)], x[r.clamp(min=0)]
        d = (a != b).sum(1)
        if revcomp:
            d = torch.minimum(d, (_revcomp(a) != b).sum(1))
        rep_dist[c0:c0 + (1 << 16)] = torch.where(r >= 0, d, torch.full_like(d, -1)).to(torch.int32)
    return Selection(picked, rep, rep_dist)


def select_diverse_edit(x, scores=None, k=None, min_dist=1, revcomp=False, block_rows=None):
    """select_diverse under a minimum EDIT distance: the same walk, the same Selection(picked, rep, rep_dist), the same
    tie rules and prefix property, with the Levenshtein distance (substitution, insertion, deletion: 1 each; global) in place of
    the Hamming distance; with revcomp the smaller of that and the edit distance to the reverse complement. min_dist is 1 .. L
    edits: a row and its copy shifted by one base are 2 edits apart, and 0.75 L apart for select_diverse. rep_dist is the edit
    distance to the representative. min_dist = 1 is select_diverse's (distance 0 means equal rows). block_rows (1 .. 4096; None:
    SELECT_EDIT_BLOCK_ROWS): a tuning knob only."""
    x, scores, k, T = _check_select(x, scores, k, min_dist, block_rows)
    if block_rows is None:
        T = SELECT_EDIT_BLOCK_ROWS
    x = _on_device(x, "x")
    N, L = x.shape

    def hits_of(order, rows, err):
        return lambda r0, r1, db, **out: ops.edit_within(rows[r0:r1], db, L, min_dist - 1, both_strands=revcomp, **out)
    packed, picked, rep = _greedy_walk(x, scores, k, T, hits_of)
    # a row against its ONE representative: N pairs (svdd_edit_pairs), -1 where there is none
    rep_dist = ops.edit_pairs(packed, packed, rep.to(torch.int32), L, L, L, both_strands=revcomp)
    return Selection(picked, rep, rep_dist)


def _exact_mean(v):
    """The correctly rounded mean of a float64 vector (math.fsum: independent of the order); NaN where +inf meets -inf."""
    try:
        return math.fsum(v.tolist()) / v.numel()
    except (ValueError, OverflowError):
        return float("nan")


def edit_distance(a, b, cap=None, revcomp=False):
    """Row i of a [B, La] against row i of b [B, Lb] (tokens 0..3; the two lengths may differ) -> int32 [B] on the device: the
    Levenshtein distance (substitution, insertion, deletion: 1 each; global), with revcomp the smaller of that and the distance
    of a's reverse complement; -1 where it exceeds cap (0 .. max(La, Lb); None: no limit)."""
    a, b = _checked(a, "a", 3), _checked(b, "b", 3)
    if a.shape[0] != b.shape[0]:
        raise ValueError(f"a and b must have one number of rows, got {a.shape[0]} and {b.shape[0]}")
    La, Lb = a.shape[1], b.shape[1]
    if max(La, Lb) > ops.PACK_MAX_L:
        raise ValueError(f"L = {max(La, Lb)} > {ops.PACK_MAX_L}")
    cap = _check_cap(cap, La, Lb)
    a, b = _on_device(a, "a"), _on_device(b, "b")
    err = torch.zeros(1, dtype=torch.int32, device=a.device)
    q, d = ops.pack_tokens(a, err=err), ops.pack_tokens(b, err=err)
    dist = ops.edit_pairs(q, d, torch.arange(a.shape[0], dtype=torch.int32, device=a.device), La, Lb, cap, both_strands=revcomp)
    ops.check_pack_err(err)
    return dist


def _library(x, scores, k, min_dist, revcomp, select=select_diverse):
    """One run of `select` without limit -> (its Selection, scores on the device, the report of library_quality)."""
    if not isinstance(k, int) or isinstance(k, bool) or k < 1:
        raise ValueError(f"k = {k!r}: expected an int >= 1")
    if scores is None:
        raise ValueError("scores = None: a library is chosen by score")
    sel = select(x, scores, None, min_dist, revcomp)
    picked, rep = sel.picked, sel.rep
    N, P = rep.shape[0], picked.shape[0]
    s = (torch.from_numpy(np.ascontiguousarray(scores)) if isinstance(scores, np.ndarray) else scores).to(picked.device).double()
    n = min(k, P)
    pick_no = torch.full((N,), -1, dtype=torch.int64, device=picked.device)
    pick_no[picked] = torch.arange(P, device=picked.device)
    rep_no = pick_no[rep]                                         # k None: every row has a representative
    lib = s[picked[:n]]
    report = {
        "library_size": n,
        "library_score_mean": _exact_mean(lib),
        "library_score_min": float(lib.min()),
        "topk_score_mean": _exact_mean(s.sort(descending=True).values[:n]),
        "families": P,
        "largest_family_fraction": int(torch.bincount(rep_no, minlength=P).max()) / N,
        "library_family_coverage": int((rep_no < n).sum()) / N,
    }
    return sel, s, report


def library_quality(x, scores, k, min_dist, revcomp=False):
    """What a library of k designs chosen by select_diverse(x, scores, k, min_dist, revcomp) is worth -> a flat dict, from ONE run
    without limit (its first k picks are the library, by the prefix property):
      library_size              min(k, families)
      library_score_mean / library_score_min   of the library's rows
      topk_score_mean           the mean of the same number of rows taken by score alone: the price of diversity is the difference
      families                  the picks of the run without limit: the distinct families the set holds at this min_dist
      largest_family_fraction   the share of rows represented by the largest family's pick
      library_family_coverage   the share of rows whose representative is in the library"""
    return _library(x, scores, k, min_dist, revcomp)[2]


def library_quality_edit(x, scores, k, min_dist, revcomp=False):
    """library_quality of a library chosen by select_diverse_edit(x, scores, k, min_dist, revcomp): the same seven keys from ONE
    run without limit, families and coverage counted by edit distance (a design and its shifted copy are one family)."""
    return _library(x, scores, k, min_dist, revcomp, select_diverse_edit)[2]


# ------------------------------------------------------------------------------------------ host-level float64 rules ----
def _f64(a):
    if isinstance(a, np.ndarray):
        a = torch.from_numpy(np.ascontiguousarray(a))
    if not isinstance(a, torch.Tensor):
        a = torch.as_tensor(a)
    return a.detach().to(torch.float64).cpu()                    # host-level: these samples are small


def wasserstein_1d(a, b):
    """The 1-D Wasserstein-1 distance of two samples (any sizes): the integral of |F_a - F_b| over the merged support, float64;
    the quantity scipy.stats.wasserstein_distance returns (reference cal_wasserstein_distance). An empty side gives NaN."""
    a, b = _f64(a).reshape(-1), _f64(b).reshape(-1)
    if a.numel() == 0 or b.numel() == 0:
        return float("nan")
    a, b = a.sort().values, b.sort().values
    allv = torch.cat([a, b]).sort().values
    fa = torch.searchsorted(a, allv[:-1], right=True).double() / a.numel()
    fb = torch.searchsorted(b, allv[:-1], right=True).double() / b.numel()
    return float(((fa - fb).abs() * (allv[1:] - allv[:-1])).sum())


def _cov(e):
    return torch.atleast_2d(torch.cov(e.T))


def frechet_distance(e1, e2):
    """|mu1 - mu2|^2 + tr(S1 + S2 - 2 (S1 S2)^(1/2)) of two embedding sets [n, D] in float64 (reference oracle.get_wasserstein_dist).
    tr (S1 S2)^(1/2) = the sum of the square roots of the eigenvalues of S1 S2 (real parts, negatives clamped at 0). NaN or empty
    input returns NaN, as the reference does."""
    e1, e2 = _f64(e1), _f64(e2)
    if e1.numel() == 0 or e2.numel() == 0 or bool(torch.isnan(e1).any()) or bool(torch.isnan(e2).any()):
        return float("nan")
    if e1.dim() != 2 or e2.dim() != 2 or e1.shape[1] != e2.shape[1]:
        raise ValueError(f"embeddings must be [n, D] with one D, got {tuple(e1.shape)} and {tuple(e2.shape)}")
    s1, s2 = _cov(e1), _cov(e2)
    ev = torch.linalg.eigvals(s1 @ s2).real.clamp(min=0.0)
    return float(((e1.mean(0) - e2.mean(0)) ** 2).sum() + torch.trace(s1) + torch.trace(s2) - 2.0 * ev.sqrt().sum())


def _median(v):
    return float(torch.quantile(v.double(), 0.5)) if v.numel() else float("nan")


# -------------------------------------------------------------------------------------------------------- the report ----
def sample_quality(x, refs=None, train=None, k=3, scores=None, ref_scores=None):
    """A flat dict of set-level metrics of the designs x [B, L] (tokens 0..3):
      kmer_pearsonr_<name>   for every set of refs {name: tokens [N', L'] or counts [4^k]}
      diversity_mean         mean Hamming distance over the pairs i != j of the batch (NaN for one row)
      diversity_nn_median    median distance of a row to its nearest OTHER row
      unique_fraction        distinct rows / rows: the rows whose nearest other row is at distance > 0, plus one representative
                             (the lowest index) of every group of duplicates
      novelty_nn_median / novelty_nn_min / memorised_fraction   with train [N, L]: the distance to the nearest training row, and
                             the share of designs that ARE a training row (distance 0)
      ws_scores_<name>       with scores [B] and ref_scores {name: [n]}: the 1-D Wasserstein distance of the two score samples
    Diversity and novelty are not in the reference."""
    _check_k(k)
    x = _tokens(x, "x", 3)
    B, L = x.shape
    out = {}
    if refs:
        cx = kmer_counts(x, k)[0].cpu()
        for name, ref in refs.items():
            out[f"kmer_pearsonr_{name}"] = _pearson_union(cx, _ref_counts(ref, k, name))
    key, hist = _hamming(x, None, None, True, True)
    dist, idx = ops.nn_decode(key)
    hist = hist.cpu()
    pairs = int(hist.sum())
    out["diversity_mean"] = float((hist * torch.arange(L + 1)).sum()) / pairs if pairs else float("nan")
    out["diversity_nn_median"] = _median(dist) if B > 1 else float("nan")
    first = torch.arange(B, device=x.device)
    out["unique_fraction"] = int(((dist != 0) | (idx > first)).sum()) / B
    if train is not None:
        dist, _ = hamming_nn(x, train)
        out["novelty_nn_median"], out["novelty_nn_min"] = _median(dist), int(dist.min())
        out["memorised_fraction"] = int((dist == 0).sum()) / B
    if scores is not None and ref_scores is not None:
        for name, rs in ref_scores.items():
            out[f"ws_scores_{name}"] = wasserstein_1d(scores, rs)
    return out
