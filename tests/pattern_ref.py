"""Host restatement of pattern scanning and pattern-driven directed evolution: plain loops, no device code.

  mutants_ref(x, positions, patterns)             the mutants in the restated order of grelu's MotifScanDataset: sequence, then start
                                                  position, then pattern (the pattern index runs fastest); a REPLACEMENT of
                                                  x[b, pos : pos + w] by the pattern, the length stays L
  fold_ref(scores, parent, ...)                   one chunk of scores into the table and the running best (svdd_pattern_fold's rule)
  table_ref(x, positions, patterns, score_fn)     the [B, P, K] table; a mutant that equals its parent has the parent's score
  apply_ref(...)                                  one iteration's boundary (svdd_pattern_apply's rule)
  evolve_patterns_ref(score_fn, x, patterns, positions, max_iter, stop)

score_fn(tokens uint8 [n, L]) -> float32 [n]. patterns: a list of token sequences over 0..3, widths 1..32. The rules:
  pick    a row's best mutant in (position, pattern) order; an entry replaces the running best only if its score is STRICTLY
          greater (the first wins a tie, the running best of earlier chunks wins a tie); a NaN never wins; the running best starts at
          (-inf, -1, -1), so a row whose entries all score NaN has no pick. best_pos is the INDEX into positions.
  copy    a mutant that equals its parent is a legitimate entry: its score is the parent's score (it is not scored again).
  global  every live row takes its pick, which may be a no-op whose score is the row's own; m = max of the picks' scores; if
          m > best_so_far then best_so_far = m, otherwise the run stops and NO row changes; the iteration is in the trace.
  row     a row takes its pick only if it strictly beats the row's score, otherwise it is dead for good.
  best    x_best / score_best: the highest-scoring state along the row's trajectory, the first occurrence among equals.
"""
import numpy as np

NEG_INF = np.float32(-np.inf)
MAX_WIDTH = 32


def _ok(x_row, pos, pat):
    """The conditions under which the kernel writes a mutant and not a copy."""
    w = len(pat)
    return (1 <= w <= MAX_WIDTH and 0 <= pos and pos + w <= len(x_row) and (np.asarray(x_row) <= 3).all()
            and all(0 <= int(t) <= 3 for t in pat))


def mutants_ref(x, positions, patterns, live=None):
    """x uint8 [B, L] -> uint8 [B, P K, L]; a dead row, a parent row with a token > 3, a pattern with one, or a window that leaves
    the row gives exact copies."""
    x = np.asarray(x, dtype=np.uint8)
    B, L = x.shape
    P, K = len(positions), len(patterns)
    out = np.empty((B, P * K, L), dtype=np.uint8)
    for b in range(B):
        for j, pos in enumerate(positions):
            for k, pat in enumerate(patterns):
                row = x[b].copy()
                if (live is None or live[b]) and _ok(x[b], pos, pat):
                    row[pos:pos + len(pat)] = np.asarray(pat, np.uint8)
                out[b, j * K + k] = row
    return out


def onehot_ref(tok):
    tok = np.asarray(tok)
    return (tok[..., None] == np.arange(4)).astype(np.float32)            # a token > 3: a zero row


def new_best(B):
    return np.full(B, NEG_INF, np.float32), np.full(B, -1, np.int32), np.full(B, -1, np.int32)


def fold_ref(scores, parent, K, p0, Pc, table, best, live=None, slot=None):
    """scores float32 [B, Pc K] of the mutants of positions[p0 : p0 + Pc] (with slot int32 [B, Pc K]: entry i has scores.flat[slot[i]],
    or parent[b] where slot[i] < 0); table [B, P, K] or None and best = (score [B], position index [B], pattern [B]) or None are
    updated in place. The chunk with p0 == 0 starts the running best."""
    B = len(parent)
    flat = np.asarray(scores, np.float32).reshape(-1)
    for b in range(B):
        if best is not None and p0 == 0:
            best[0][b], best[1][b], best[2][b] = NEG_INF, -1, -1
        for j in range(Pc):
            for k in range(K):
                i = (b * Pc + j) * K + k
                if slot is None:
                    s = flat[i]
                else:
                    s = flat[slot.reshape(-1)[i]] if slot.reshape(-1)[i] >= 0 else np.float32(parent[b])
                if table is not None:
                    table[b, p0 + j, k] = s
                if best is not None and (live is None or live[b]) and s > best[0][b]:       # NaN > anything is False
                    best[0][b], best[1][b], best[2][b] = s, p0 + j, k


def _scores_with_copies(score_fn, x, cand, parent, whole_batch=False, K=None, chunk=None):
    """score_fn on the mutants that differ from their parent; a copy has its parent's score. whole_batch: score_fn is asked about
    whole batches of mutants, the copies included, and the copies' answers are dropped (for a scorer whose bits may depend on the
    batch it is given: the engine's whole-mutant route forms exactly these batches) — all mutants at once, or with chunk (and K)
    one batch per `chunk` positions, rows in (sequence, position, pattern) order, the last batch possibly shorter."""
    B, M, L = cand.shape
    differs = (cand != x[:, None, :]).any(-1)
    out = np.repeat(np.asarray(parent, np.float32)[:, None], M, 1)
    if whole_batch:
        step = M if chunk is None else chunk * K
        for m0 in range(0, M, step):
            sub = np.ascontiguousarray(cand[:, m0:m0 + step])
            sc = np.asarray(score_fn(sub.reshape(-1, L)), dtype=np.float32).reshape(B, -1)
            out[:, m0:m0 + step][differs[:, m0:m0 + step]] = sc[differs[:, m0:m0 + step]]
    elif differs.any():
        out[differs] = np.asarray(score_fn(cand[differs]), dtype=np.float32)
    return out


def table_ref(x, positions, patterns, score_fn, whole_batch=False, chunk=None):
    x = np.asarray(x, dtype=np.uint8)
    B = x.shape[0]
    P, K = len(positions), len(patterns)
    parent = np.asarray(score_fn(x), dtype=np.float32)
    scores = _scores_with_copies(score_fn, x, mutants_ref(x, positions, patterns), parent, whole_batch, K, chunk)
    table = np.empty((B, P, K), np.float32)
    fold_ref(scores, parent, K, 0, P, table, None)
    return table


def apply_ref(best, positions, patterns, stop, x, score_cur, live, state, x_best, score_best):
    """One boundary; everything updated in place; state = {"best_so_far": float32, "stopped": bool}.
    -> the trace row (start position [B], pattern [B], score [B], taken [B]) or None when the run was already stopped."""
    if state["stopped"]:
        return None
    B, L = x.shape
    P, K = len(positions), len(patterns)
    bs, bp, bk = best

    def valid_of(b):
        if not ((live is None or live[b]) and 0 <= bp[b] < P and 0 <= bk[b] < K):
            return False
        pos, w = positions[bp[b]], len(patterns[bk[b]])
        return 1 <= w <= MAX_WIDTH and pos >= 0 and pos + w <= L
    valid = [valid_of(b) for b in range(B)]
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
            tr[0][b], tr[1][b] = positions[bp[b]], bk[b]
        if take[b]:
            tr[3][b] = 1
            pat = np.asarray(patterns[bk[b]], np.uint8)
            x[b, positions[bp[b]]:positions[bp[b]] + len(pat)] = pat
            score_cur[b] = bs[b]
            if score_cur[b] > score_best[b]:
                x_best[b] = x[b]
                score_best[b] = score_cur[b]
        elif stop == "row" and live[b]:
            live[b] = 0
    return tr


def evolve_patterns_ref(score_fn, x, patterns, positions=None, max_iter=10, stop="global", whole_batch=False, chunk=None):
    """-> (x_best uint8 [B, L], score_best float32 [B], trace dict as Diffusion.evolve_patterns', numpy)."""
    x = np.array(x, dtype=np.uint8)
    B, L = x.shape
    K = len(patterns)
    if positions is None:
        positions = list(range(L - max(len(p) for p in patterns) + 1))
    P = len(positions)
    if stop not in ("global", "row"):
        raise ValueError(stop)
    score_cur = np.array(score_fn(x), dtype=np.float32)
    x_best, score_best = x.copy(), score_cur.copy()
    m0 = NEG_INF
    for s in score_cur:
        if s > m0:
            m0 = s
    state = {"best_so_far": m0, "stopped": False}
    live = np.ones(B, np.uint8) if stop == "row" else None
    rows, scores_tr = [], [score_cur.copy()]
    for _ in range(max_iter):
        cand = mutants_ref(x, positions, patterns, live)
        scores = _scores_with_copies(score_fn, x, cand, score_cur, whole_batch, K, chunk)
        best = new_best(B)
        fold_ref(scores, score_cur, K, 0, P, None, best, live)
        tr = apply_ref(best, positions, patterns, stop, x, score_cur, live, state, x_best, score_best)
        rows.append(tr)
        scores_tr.append(tr[2])
        if state["stopped"]:
            break
    n = len(rows)
    trace = {"iters": n,
             "position": np.stack([r[0] for r in rows]) if n else np.zeros((0, B), np.int32),
             "pattern": np.stack([r[1] for r in rows]) if n else np.zeros((0, B), np.int32),
             "taken": np.stack([r[3] for r in rows]) if n else np.zeros((0, B), np.uint8),
             "score": np.stack(scores_tr)}
    return x_best, score_best, trace
