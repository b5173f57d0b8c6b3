"""Plain numpy restatement of svdd_edit_nn, written from the contract in include/svdd_hip.h, and of
svdd_amd.quality.edit_quality. The Levenshtein table is filled column by column (Wagner-Fischer) for all pairs at once; inside a
column new[i] = min(t[i], new[i - 1] + 1) is the running minimum of t - i, plus i. Nothing bit-parallel: this is what the kernel and
the module are compared with."""
import numpy as np

from tests.quality_ref import ALL_ONES, hamming_nn_ref, nn_decode_ref


def edit_matrix(xq, xdb):
    """[B, N] Levenshtein distances of unpacked rows (substitution, insertion, deletion: 1 each; global)."""
    xq, xdb = np.asarray(xq), np.asarray(xdb)
    (B, m), (N, n) = xq.shape, xdb.shape
    ar = np.arange(m + 1, dtype=np.int64)
    col = np.broadcast_to(ar, (B, N, m + 1)).copy()                       # column 0: D[i][0] = i
    for j in range(n):
        differ = xq[:, None, :] != xdb[None, :, j, None]                  # [B, N, m]
        t = np.empty_like(col)
        t[..., 0] = j + 1                                                 # D[0][j + 1]
        t[..., 1:] = np.minimum(col[..., :-1] + differ, col[..., 1:] + 1)  # diagonal, left
        col = np.minimum.accumulate(t - ar, axis=-1) + ar                 # ... and the cell above, all the way down
    return col[..., m]


def _pairs(xq, xdb, cap, q_base, db_base, exclude_diag, d):
    d = edit_matrix(xq, xdb) if d is None else d
    B, N = d.shape
    keep = np.ones((B, N), bool)
    if exclude_diag:
        keep = (q_base + np.arange(B))[:, None] != (db_base + np.arange(N))[None, :]
    return d, keep, keep & (d <= cap)


def edit_nn_ref(xq, xdb, cap, q_base=0, db_base=0, exclude_diag=False, nn_key=None, hist=None, d=None):
    """svdd_edit_nn on UNPACKED rows -> (nn_key u64 [B], hist i64 [cap + 2]), both continued from what is passed in.
    d: edit_matrix(xq, xdb) where the caller has it already (the table is the slow part)."""
    d, keep, near = _pairs(xq, xdb, cap, q_base, db_base, exclude_diag, d)
    B, N = d.shape
    key = np.full(B, ALL_ONES, np.uint64) if nn_key is None else np.array(nn_key, np.uint64)
    hist = np.zeros(cap + 2, np.int64) if hist is None else np.array(hist, np.int64)
    hist[:cap + 1] += np.bincount(d[near], minlength=cap + 1)
    hist[cap + 1] += int((keep & ~near).sum())
    cand = (d.astype(np.uint64) << np.uint64(32)) | (db_base + np.arange(N)).astype(np.uint64)[None, :]
    cand = np.where(near, cand, ALL_ONES)
    return np.minimum(key, cand.min(axis=1)), hist


def edit_hist_ref(xq, xdb, cap, exclude_diag=False, d=None):
    return edit_nn_ref(xq, xdb, cap, exclude_diag=exclude_diag, d=d)[1]


def edit_quality_ref(x, edit_cap, train=None):
    """svdd_amd.quality.edit_quality from the restatements above."""
    x = np.asarray(x)
    out = {}
    dist, _ = nn_decode_ref(edit_nn_ref(x, x, edit_cap, exclude_diag=True)[0])
    out["edit_near_batch_fraction"] = float((dist >= 0).mean())
    if train is not None:
        train = np.asarray(train)
        dist, _ = nn_decode_ref(edit_nn_ref(x, train, edit_cap)[0])
        near = dist >= 0
        out["edit_near_train_fraction"] = float(near.mean())
        out["edit_near_train_min"] = int(dist[near].min()) if near.any() else -1
        if train.shape[1] == x.shape[1]:
            hd, _ = nn_decode_ref(hamming_nn_ref(x, train)[0])
            out["hamming_missed_fraction"] = float((near & (hd > edit_cap)).mean())
    return out
