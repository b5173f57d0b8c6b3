"""Host restatement of in-silico mutagenesis and ISM-driven directed evolution: plain loops, no device code.

  mutants_ref(x, positions)                       the mutants in the order of the reference's ISMDataset(..., drop_ref=True): sequence,
                                                  then position, then allele in ACGT order with the row's own base skipped
  fold_ref(...)                                   one chunk of scores into the table and the running best (svdd_ism_fold's rule)
  ism_ref(x, positions, score_fn)                 the [B, P, 4] table; the entry of a row's own base is the row's own score
  apply_ref(...)                                  one iteration's boundary (svdd_evolve_apply's rule)
  evolve_ref(x, positions, score_fn, max_iter, stop)

score_fn(tokens uint8 [n, L]) -> float32 [n]. The rules, as the issue states them:
  pick    a row's best mutant in (position, allele) order; a mutant replaces the running best only if its score is STRICTLY
          greater (the first wins a tie, like pandas idxmax); a NaN never wins; the running best starts at (-inf, -1, -1), so a
          row whose mutants all score NaN or -inf has no pick.
  global  every live row takes its pick whether or not it improves on the row's score; m = max of the picks' scores; if
          m > best_so_far then best_so_far = m, otherwise the run stops and NO row changes; the iteration is in the trace.
          best_so_far starts at the maximum of the inputs' scores (the reference's iteration 0).
  row     a row takes its pick only if it strictly beats the row's score, otherwise it is dead for good; the run stops in the
          iteration in which no row moved.
  best    x_best / score_best: the highest-scoring state along the row's trajectory, the first occurrence among equals.
"""
import numpy as np

NEG_INF = np.float32(-np.inf)


def alleles_of(ref):
    """The three bases that are not `ref`, ascending (k = 0, 1, 2)."""
    return [a for a in range(4) if a != ref]


def mutants_ref(x, positions, live=None):
    """x uint8 [B, L] -> uint8 [B, 3P, L]; a row with live[b] == 0, or a parent token > 3 at the position, gives exact copies."""
    x = np.asarray(x, dtype=np.uint8)
    B, L = x.shape
    P = len(positions)
    out = np.empty((B, 3 * P, L), dtype=np.uint8)
    for b in range(B):
        for j, pos in enumerate(positions):
            for k in range(3):
                row = x[b].copy()
                ref = int(x[b, pos])
                if ref <= 3 and (live is None or live[b]):
                    row[pos] = alleles_of(ref)[k]
                out[b, 3 * j + k] = row
    return out


def onehot_ref(tok):
    tok = np.asarray(tok)
    return (tok[..., None] == np.arange(4)).astype(np.float32)            # a token > 3: a zero row


def fold_ref(scores, parent_score, x, positions, p0, Pc, ism, best, live=None):
    """scores float32 [B, 3 Pc] of the mutants of positions[p0 : p0 + Pc]; ism [B, P, 4] or None and best = (score [B], pos [B],
    allele [B]) or None are updated in place. The chunk with p0 == 0 starts the running best."""
    B = x.shape[0]
    for b in range(B):
        if best is not None and p0 == 0:
            best[0][b], best[1][b], best[2][b] = NEG_INF, -1, -1
        for j in range(Pc):
            pos = positions[p0 + j]
            ref = int(x[b, pos])
            if ism is not None:
                ism[b, p0 + j, :] = parent_score[b]
            if ref > 3:
                continue
            for k, a in enumerate(alleles_of(ref)):
                s = np.float32(scores[b, 3 * j + k])
                if ism is not None:
                    ism[b, p0 + j, a] = s
                if best is not None and (live is None or live[b]) and s > best[0][b]:       # NaN > anything is False
                    best[0][b], best[1][b], best[2][b] = s, pos, a


def new_best(B):
    return np.full(B, NEG_INF, np.float32), np.full(B, -1, np.int32), np.full(B, -1, np.int32)


def ism_ref(x, positions, score_fn):
    x = np.asarray(x, dtype=np.uint8)
    B, L = x.shape
    P = len(positions)
    parent = np.asarray(score_fn(x), dtype=np.float32)
    scores = np.asarray(score_fn(mutants_ref(x, positions).reshape(B * 3 * P, L)), dtype=np.float32).reshape(B, 3 * P)
    ism = np.empty((B, P, 4), np.float32)
    fold_ref(scores, parent, x, positions, 0, P, ism, None)
    return ism


def apply_ref(best, stop, x, score_cur, live, state, x_best, score_best):
    """One boundary; everything updated in place; state = {"best_so_far": float32, "stopped": bool}.
    -> the trace row (position [B], allele [B], score [B], taken [B]) or None when the run was already stopped."""
    if state["stopped"]:
        return None
    B, L = x.shape
    bs, bp, ba = best
    valid = [bool((live is None or live[b]) and 0 <= bp[b] < L and 0 <= ba[b] <= 3) for b in range(B)]
    if stop == "global":
        m = NEG_INF
        for b in range(B):
            if valid[b] and bs[b] > m:
                m = bs[b]
        go = bool(m > state["best_so_far"])
        if go:
            state["best_so_far"] = m
        else:
            state["stopped"] = True
        take = [valid[b] and go for b in range(B)]
    elif stop == "row":
        take = [valid[b] and bool(bs[b] > score_cur[b]) for b in range(B)]
        if not any(take):
            state["stopped"] = True
    else:
        raise ValueError(stop)
    tr = (np.full(B, -1, np.int32), np.full(B, -1, np.int32), np.empty(B, np.float32), np.zeros(B, np.uint8))
    for b in range(B):
        tr[2][b] = bs[b] if valid[b] else score_cur[b]
        if valid[b]:
            tr[0][b], tr[1][b] = bp[b], ba[b]
        if take[b]:
            tr[3][b] = 1
            x[b, bp[b]] = ba[b]
            score_cur[b] = bs[b]
            if score_cur[b] > score_best[b]:
                x_best[b] = x[b]
                score_best[b] = score_cur[b]
        elif stop == "row" and live[b]:
            live[b] = 0
    return tr


def evolve_ref(x, positions, score_fn, max_iter, stop):
    """-> (x_best uint8 [B, L], score_best float32 [B], trace dict as Diffusion.evolve's, numpy)."""
    x = np.array(x, dtype=np.uint8)
    B, L = x.shape
    P = len(positions)
    score_cur = np.array(score_fn(x), dtype=np.float32)
    x_best, score_best = x.copy(), score_cur.copy()
    m0 = NEG_INF
    for s in score_cur:
        if s > m0:
            m0 = s
    state = {"best_so_far": m0, "stopped": False}
    live = np.ones(B, np.uint8) if stop == "row" else None
    if stop not in ("global", "row"):
        raise ValueError(stop)
    rows, scores_tr = [], [score_cur.copy()]
    for _ in range(max_iter):
        cand = mutants_ref(x, positions, live)
        scores = np.asarray(score_fn(cand.reshape(B * 3 * P, L)), dtype=np.float32).reshape(B, 3 * P)
        best = new_best(B)
        fold_ref(scores, score_cur, x, positions, 0, P, None, best, live)
        tr = apply_ref(best, stop, x, score_cur, live, state, x_best, score_best)
        rows.append(tr)
        scores_tr.append(tr[2])
        if state["stopped"]:
            break
    n = len(rows)
    trace = {"iters": n,
             "position": np.stack([r[0] for r in rows]) if n else np.zeros((0, B), np.int32),
             "allele": np.stack([r[1] for r in rows]) if n else np.zeros((0, B), np.int32),
             "taken": np.stack([r[3] for r in rows]) if n else np.zeros((0, B), np.uint8),
             "score": np.stack(scores_tr)}
    return x_best, score_best, trace
