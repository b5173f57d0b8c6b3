"""Float64 restatements and shared set-up for the tests of the Enformer-shaped value trunk (svdd_amd/enformer_value.py,
svdd_amd/fused_trunk.py, csrc/svdd_trunk.hip). Not a test module: imported by the CPU and GPU trunk tests."""
import numpy as np
import torch

from svdd_amd.enformer_value import _relative_shift


def _bn_stats(m, g):
    m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.1)
    m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
    m.weight.copy_(1.0 + 0.2 * torch.randn(m.num_features, generator=g))
    m.bias.copy_(0.1 * torch.randn(m.num_features, generator=g))


def _pool_logits(tower, g):
    for blk in tower.blocks:
        pw = blk[1].pool.to_attn_logits.weight
        pw.add_((torch.randn(pw.shape, generator=g) * 0.05).to(pw.device))


def randomise(emb, head, seed):
    """Non-trivial BatchNorm statistics, attention output projections (zero at init) and pooling logits."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    with torch.no_grad():
        for m in emb.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                _bn_stats(m, g)
        for blk in emb.transformer_tower:
            w = blk.mha.to_out.weight
            w.copy_(torch.randn(w.shape, generator=g) * (w.shape[1] ** -0.5))
            blk.mha.to_out.bias.copy_(torch.randn(w.shape[0], generator=g) * 0.05)
        _pool_logits(emb.conv_tower, g)


def randomise_tower(tower, seed):
    """The conv-tower part of `randomise` for an EnformerConvTower on its own: BatchNorm statistics and pooling logits."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    with torch.no_grad():
        for m in tower.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                _bn_stats(m, g)
        _pool_logits(tower, g)


def attn_small_ref(qkv, rel_k, content_bias, pos_bias, n, T, heads, dk, dv):
    """What svdd_trunk_attn_small computes, in the dtype of its inputs: qkv [n T, heads (2 dk + dv)] = [q | k | v], rel_k
    [heads, 2 T - 1, dk], biases [heads, dk] -> [n T, heads dv]. The relative shift is the module's own."""
    nq = heads * dk
    q = qkv[:, :nq].reshape(n, T, heads, dk).transpose(1, 2) * dk ** -0.5
    k = qkv[:, nq:2 * nq].reshape(n, T, heads, dk).transpose(1, 2)
    v = qkv[:, 2 * nq:].reshape(n, T, heads, dv).transpose(1, 2)
    cb, pb = content_bias.reshape(1, heads, 1, dk), pos_bias.reshape(1, heads, 1, dk)
    rel = _relative_shift(torch.einsum("bhid,hjd->bhij", q + pb, rel_k))
    logits = torch.matmul(q + cb, k.transpose(-1, -2)) + rel
    return torch.matmul(torch.softmax(logits, dim=-1), v).transpose(1, 2).reshape(n * T, heads * dv)


def gelu(x):
    return x * torch.sigmoid(1.702 * x)


def act(x, a):
    return x if a == 0 else torch.relu(x) if a == 1 else gelu(x)


# ---- first levels shared between a candidate and its parent (csrc/svdd_trunk.hip: svdd_trunk_windows, svdd_trunk_stem_unfold_win,
# svdd_trunk_attn_pool_win). Plain restatements of include/svdd_hip.h's words, and the one case table of the CPU and GPU tests.
def windows_ref(cand, parent, parent_idx, div, L, halo, depth, slots, count=None):
    """What svdd_trunk_windows writes: w0, wlen, seg as int32 [depth][n][slots]. Candidate c against row parent_idx[c] // div of
    `parent`, the positions that differ walked in ascending order. Level 0: one even-aligned window around each position, +- halo,
    clipped to the sequence; a window that touches the one before joins it, and once `slots` windows exist everything further joins
    the last. Level d + 1: every window halved, two rows more on each side (k = 5), even-aligned, clipped to the level; a window
    within 4 rows of the one before joins it. seg = wlen, + 4 context rows for d >= 1. Unused slots and c >= count: zeros."""
    n = len(cand)
    w0, wlen, seg = (np.zeros((depth, n, slots), dtype=np.int32) for _ in range(3))
    for c in range(n if count is None else min(n, count)):
        par = parent[parent_idx[c] // div]
        wins = []
        for p in range(L):
            if cand[c][p] == par[p]:
                continue
            lo, hi = max(0, p - halo) & ~1, min(L, (p + halo + 2) & ~1)
            if wins and (lo <= wins[-1][1] or len(wins) == slots):
                wins[-1][1] = max(wins[-1][1], hi)
            else:
                wins.append([lo, hi])
        Lc = L
        for d in range(depth):
            for j, (lo, hi) in enumerate(wins):
                w0[d, c, j], wlen[d, c, j], seg[d, c, j] = lo, hi - lo, hi - lo + (4 if d else 0)
            Lc //= 2                                               # (every level but the last shared one has an even length)
            nxt = []
            for lo, hi in wins:
                lo, hi = max(0, lo // 2 - 2) & ~1, min(Lc, (hi // 2 + 3) & ~1)
                if nxt and lo <= nxt[-1][1] + 4:
                    nxt[-1][1] = max(nxt[-1][1], hi)
                else:
                    nxt.append([lo, hi])
            wins = nxt
    return w0, wlen, seg


def reach_ref(changed, L, halo, depth):
    """Per level d < depth, the set of rows (of the level's length, ceil(L / 2^d)) that can differ from the parent's when the tokens
    at `changed` do — by brute force from what a row reads, no window in sight: a level-0 row p reads tokens p - halo .. p + halo,
    a pooled row i reads rows 2 i and 2 i + 1, a row of a level >= 1 reads pooled rows i - 2 .. i + 2."""
    rows = {r for r in range(L) if any(abs(r - p) <= halo for p in changed)}
    out, Lc = [rows], L
    for _ in range(1, depth):
        Lc = (Lc + 1) // 2
        pooled = {i for i in range(Lc) if 2 * i in rows or 2 * i + 1 in rows}
        rows = {i for i in range(Lc) if any(j in pooled for j in range(i - 2, i + 3))}
        out.append(rows)
    return out


def compact_offsets(seg, gap=0):
    """seg int [n][slots] -> (off int32 [n slots], total): the exclusive prefix sum the kernels are given; gap > 0 leaves that many
    rows free behind every used segment (an off the pooling kernel must honour slot by slot)."""
    s = np.asarray(seg, dtype=np.int64).reshape(-1)
    step = s + np.where(s > 0, gap, 0)
    off = np.cumsum(step) - step
    return off.astype(np.int32), int(step.sum())


def to_compact(dense, w0, wlen, off, in_halo, total, fill):
    """Dense per-sequence rows [n, L, C] (torch) -> the compact rows [total, C] the window kernels read: the segment of slot s
    starts at off[s], its window (rows w0[s] .. w0[s] + wlen[s] - 1 of sequence s // slots) in_halo rows further; every other row —
    the context rows of the segments and whatever lies between segments — holds `fill`."""
    n, slots = w0.shape
    out = torch.full((total, dense.shape[2]), fill, dtype=dense.dtype)
    for c in range(n):
        for j in range(slots):
            a, ln, o = int(w0[c, j]), int(wlen[c, j]), int(off[c * slots + j]) + in_halo
            out[o:o + ln] = dense[c, a:a + ln]
    return out


WIN_N, WIN_B, WIN_DIV, MASK = 24, 4, 6, 4
# (L, depth, slots, halo, count, permuted): every length x the depths its evenness allows (L = 30: level 1 has an odd length;
# 37 and 201: one level) x 1 / 2 / 4 slots; then halo 0 and 3, the live counts n // 3 and 0, and parent_idx permuted with div 1
WINDOW_CASES = [(L, depth, slots, 7, None, False)
                for L, depths in ((2, (1, 2)), (16, (1, 2, 3, 4)), (30, (1, 2)), (37, (1,)), (200, (1, 2, 3, 4)), (201, (1,)), (256, (1, 2, 3, 4)))
                for depth in depths for slots in (1, 2, 4)]
WINDOW_CASES += [(200, 3, 4, 0, None, False), (200, 3, 2, 3, None, False), (200, 4, 4, 7, WIN_N // 3, False), (30, 2, 2, 7, WIN_N // 3, False),
                 (256, 4, 2, 7, WIN_N // 3, False), (200, 2, 4, 7, 0, False), (200, 4, 4, 7, None, True), (16, 2, 1, 7, None, True)]


def window_case_id(case):
    L, depth, slots, halo, count, perm = case
    return f"L{L}d{depth}k{slots}h{halo}" + ("" if count is None else f"n{count}") + ("perm" if perm else "")


def _level0(p, L, halo):
    return max(0, p - halo) & ~1, min(L, (p + halo + 2) & ~1)


def _level1(p, L, halo):
    lo, hi = _level0(p, L, halo)
    return max(0, lo // 2 - 2) & ~1, min(L // 2, (hi // 2 + 3) & ~1)


def window_case_edits(L, halo, slots):
    """The changed positions of the WIN_N candidates of a case: none, either end, both, two adjacent, two whose level-0 windows
    just touch / just do not, two whose level-1 windows are 4 (joined) / 6 (apart) rows from each other, more positions than
    slots spread over the sequence, every position — then random sets. Where L is too short for a pair, the far end stands in."""
    a = min(L - 1, max(0, L // 5))
    first = lambda ok: next((p for p in range(a + 1, L) if ok(p)), L - 1)                        # noqa: E731
    last = lambda ok: next((p for p in range(L - 1, a, -1) if ok(p)), L - 1)                      # noqa: E731
    hi0, hi1 = _level0(a, L, halo)[1], _level1(a, L, halo)[1]
    edits = [[], [0], [L - 1], [0, L - 1], [L // 2, min(L - 1, L // 2 + 1)],
             [a, last(lambda p: _level0(p, L, halo)[0] == hi0)], [a, first(lambda p: _level0(p, L, halo)[0] > hi0)],
             [a, last(lambda p: _level1(p, L, halo)[0] == hi1 + 4)], [a, first(lambda p: _level1(p, L, halo)[0] == hi1 + 6)],
             sorted({int(round(k * (L - 1) / (slots + 1))) for k in range(slots + 2)}), list(range(L))]
    rng = np.random.default_rng(1000 * L + 10 * halo + slots)
    while len(edits) < WIN_N:
        k = int(rng.integers(1, 7))
        edits.append(sorted({int(p) for p in rng.integers(0, L, size=k)}))
    return [sorted(set(e)) for e in edits]


def window_case_tokens(case):
    """-> cand u8 [n, L], parent u8 [B, L], parent_idx int32 [n], div, edits: candidate c is its parent (row parent_idx[c] // div)
    with the tokens at edits[c] changed. Parent 3 is all MASK; the candidates of a parent are spread over the batch (c % 4), so
    parent_idx is no multiple of anything; permuted: 24 parents in shuffled order, div 1."""
    L, depth, slots, halo, count, perm = case
    rng = np.random.default_rng(7 * L + depth + 100 * slots)
    nb = WIN_N if perm else WIN_B
    parent = rng.integers(0, 5, size=(nb, L)).astype(np.uint8)
    parent[3] = MASK
    if perm:
        parent_idx, div = rng.permutation(WIN_N).astype(np.int32), 1
    else:
        parent_idx, div = np.array([(c % WIN_B) * WIN_DIV + c // WIN_B for c in range(WIN_N)], dtype=np.int32), WIN_DIV
    edits = window_case_edits(L, halo, slots)
    cand = parent[parent_idx // div].copy()
    for c, ps in enumerate(edits):
        for p in ps:
            cand[c, p] = (int(cand[c, p]) + 1 + p % 3) % 5 if cand[c, p] != MASK else p % 4
    return cand, parent, parent_idx, div, edits
