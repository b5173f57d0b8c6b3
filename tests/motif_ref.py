"""numpy restatements of svdd_amd.motifs and svdd_motif_scan, written from the contracts in include/svdd_hip.h and
the module's docstrings: integerisation of a position-frequency matrix, the threshold by dynamic programming and by brute force
over all 4^w strings, the scan (per-window scores on both strands, hits, rows hit, per-row hits, the best window by the tie rules)
and rank-average Spearman. Plain loops and dictionaries: nothing here shares code with the module."""
import functools
import itertools
import math

import numpy as np

INT32_MIN = -(1 << 31)


def integerise_ref(pfm, nsites=20.0, bg=(0.25,) * 4, pseudocount=0.1, scale=100):
    """[w, 4] frequencies or counts -> int [w, 4]: rint(log2(p / bg) scale), p = (f nsites + pseudocount bg) / (nsites + pseudocount)."""
    out = []
    for row in np.asarray(pfm, np.float64):
        s = float(sum(row))
        out.append([int(np.rint(math.log2(((row[t] / s) * nsites + pseudocount * bg[t]) / (nsites + pseudocount) / bg[t]) * scale))
                    for t in range(4)])
    return np.array(out, np.int64)


def distribution_ref(pwm, bg=(0.25,) * 4):
    """{score: probability} of a random w-mer under the i.i.d. background, column by column (float64)."""
    dist = {0: 1.0}
    for col in np.asarray(pwm, np.int64):
        new = {}
        for t in range(4):
            for s, pr in dist.items():
                new[s + int(col[t])] = new.get(s + int(col[t]), 0.0) + pr * bg[t]
        dist = new
    return dist


def _threshold_from(dist, pvalue):
    """The smallest attainable score with tail <= pvalue, else max + 1; also the relative distance of the nearest tail to pvalue."""
    scores = sorted((s for s, pr in dist.items() if pr > 0), reverse=True)
    best, gap, tail = scores[0] + 1, float("inf"), 0.0
    for t in scores:                                  # from the top: the tail grows from its smallest terms
        tail += dist[t]
        gap = min(gap, abs(tail - pvalue) / pvalue)
        if tail <= pvalue:
            best = t
    return best, gap


def threshold_dp_ref(pwm, pvalue, bg=(0.25,) * 4):
    return _threshold_from(distribution_ref(pwm, bg), pvalue)[0]


@functools.lru_cache(maxsize=None)
def _brute_distribution(pwm_bytes, w, bg):
    pwm = np.frombuffer(pwm_bytes, np.int64).reshape(w, 4)
    terms = {}
    for s in itertools.product(range(4), repeat=w):
        score = int(sum(pwm[i, t] for i, t in enumerate(s)))
        terms.setdefault(score, []).append(math.prod(bg[t] for t in s))
    return {s: math.fsum(v) for s, v in terms.items()}


def threshold_brute_ref(pwm, pvalue, bg=(0.25,) * 4):
    """By enumerating all 4^w strings: every score's probability is the fsum of its strings' -> (threshold, the smallest relative
    distance |tail - pvalue| / pvalue over the attainable scores)."""
    pwm = np.ascontiguousarray(pwm, np.int64)
    return _threshold_from(_brute_distribution(pwm.tobytes(), pwm.shape[0], tuple(bg)), pvalue)


def window_scores_ref(x, pwm, w):
    """x [N, L] tokens, pwm [>= w, 4] -> (S+ [N, L - w + 1], S- [N, L - w + 1]) int64; S-[n, p] = sum_i pwm[w - 1 - i, 3 - x[n, p + i]]."""
    x = np.asarray(x, np.int64)
    N, L = x.shape
    nw = max(L - w + 1, 0)
    f, r = np.zeros((N, nw), np.int64), np.zeros((N, nw), np.int64)
    pwm = np.asarray(pwm, np.int64)
    for i in range(w):
        if nw:
            f += pwm[i][x[:, i:i + nw]]
            r += pwm[w - 1 - i][3 - x[:, i:i + nw]]
    return f, r


def scan_ref(x, mset, both=True):
    """-> dict: hits i64 [M], rows_hit i64 [M], row_hits i32 [N, M], best_score / best_start i32 [N, M], best_strand i8 [N, M]
    (highest score; then the lowest start; then forward (0) before reverse (1); no window: INT32_MIN, -1, -1), plus
    any_nonhit bool [M]: some window of some strand is below the threshold."""
    x = np.asarray(x)
    N, M = x.shape[0], len(mset.width)
    out = dict(hits=np.zeros(M, np.int64), rows_hit=np.zeros(M, np.int64), row_hits=np.zeros((N, M), np.int32),
               best_score=np.full((N, M), INT32_MIN, np.int64), best_start=np.full((N, M), -1, np.int32),
               best_strand=np.full((N, M), -1, np.int8), any_nonhit=np.zeros(M, bool))
    for m in range(M):
        w, thr = int(mset.width[m]), int(mset.threshold[m])
        f, r = window_scores_ref(x, mset.pwm[m], w)
        if f.shape[1] == 0:
            continue
        hit = (f >= thr).astype(np.int64) + ((r >= thr).astype(np.int64) if both else 0)
        out["row_hits"][:, m] = hit.sum(1)
        out["any_nonhit"][m] = bool((f < thr).any() or (both and (r < thr).any()))
        # candidates in the order of the tie rule: start ascending, forward before reverse; argmax takes the first maximum
        cand = np.stack([f, r], 2).reshape(N, -1) if both else f
        j = cand.argmax(1)
        out["best_score"][:, m] = cand[np.arange(N), j]
        out["best_start"][:, m] = j // 2 if both else j
        out["best_strand"][:, m] = j % 2 if both else 0
    out["hits"] = out["row_hits"].astype(np.int64).sum(0)
    out["rows_hit"] = (out["row_hits"] > 0).sum(0).astype(np.int64)
    out["best_score"] = out["best_score"].astype(np.int32)
    return out


def best_key_ref(score, start, strand):
    """The entry's i64 key of a best window (include/svdd_hip.h): (u32(score) ^ 0x80000000) << 32 | u32(~(2 start + strand)); no
    window (start -1): 0. -> uint64 array."""
    score, start, strand = (np.asarray(a, np.int64) for a in (score, start, strand))
    hi = ((score & 0xFFFFFFFF) ^ 0x80000000).astype(np.uint64)
    lo = (~(2 * start + strand) & 0xFFFFFFFF).astype(np.uint64)
    return np.where(start < 0, np.uint64(0), (hi << np.uint64(32)) | lo)


def revcomp(x):
    return 3 - np.asarray(x)[..., ::-1]


def rank_average_ref(a):
    a = [float(v) for v in a]
    return [sum(1 for u in a if u < v) + (sum(1 for u in a if u == v) + 1) / 2.0 for v in a]


def pearson_ref(a, b):
    a, b = [float(v) for v in a], [float(v) for v in b]
    if len(a) < 2:
        return float("nan")
    ma, mb = math.fsum(a) / len(a), math.fsum(b) / len(b)
    sab = math.fsum((u - ma) * (v - mb) for u, v in zip(a, b))
    den = math.sqrt(math.fsum((u - ma) ** 2 for u in a) * math.fsum((v - mb) ** 2 for v in b))
    return sab / den if den > 0 else float("nan")


def spearman_ref(a, b):
    if len(a) < 2:
        return float("nan")
    return pearson_ref(rank_average_ref(a), rank_average_ref(b))


def motif_report_ref(x, mset, refs):
    """BaseModel.evaluate_motifs' dict from the restatement."""
    c = scan_ref(x, mset)
    freq = c["rows_hit"] / x.shape[0]
    out = {}
    for name, ref in refs.items():
        ref = np.asarray(ref)
        fr = ref if ref.ndim == 1 else scan_ref(ref, mset)["rows_hit"] / ref.shape[0]
        out[f"motif_spearman_{name}"] = spearman_ref(freq, fr)
    out["motifs_per_row_mean"] = int(c["hits"].sum()) / x.shape[0]
    out["motifs_reachable"] = int((mset.threshold.astype(np.int64) <= mset.max_score).sum())
    return out
