"""What tests/test_backbone_incr3_cpu.py and tests/test_backbone_incr3_gpu.py share: a numpy restatement of the work list of
svdd_backbone_incr3_f32 (the reach of a changed position from the dilations, the marked tiles per carried layer, the cut into items)
and the uniform unmasking model behind the estimate of how much of the carried layers a decode step marks."""
import numpy as np

TILES = 13                                        # row tiles of 16 in the 208-row planes


def reach(dil, depth):
    """reach[k - 1] of plane k = 1 .. depth: 4 + sum over i < k of 4 dil[i]."""
    return [4 + 4 * sum(dil[:k]) for k in range(1, depth + 1)]


def slots(max_item):
    return 13 if max_item == 1 else 7


def marked_tiles(changed, L, rc):
    """bool [13]: tile T holds a position within rc of a changed position (changed: 1-d int array)."""
    lo = 16 * np.arange(TILES)
    hi = np.minimum(lo + 15, L - 1)
    if len(changed) == 0:
        return np.zeros(TILES, dtype=bool)
    return ((changed[:, None] >= lo[None] - rc) & (changed[:, None] <= hi[None] + rc)).any(0) & (lo <= L - 1)


def expected_items(prev, new, L, dil, depth, max_item):
    """prev, new: [n][L] integer arrays -> (items [depth][n][slots] int32, masks [depth][n][13] bool): the marked tiles of every
    carried plane and their runs of adjacent tiles cut to at most max_item, first tile | tiles << 8, packed from slot 0, 0 = empty."""
    prev, new = np.asarray(prev), np.asarray(new)
    n, S = prev.shape[0], slots(max_item)
    items = np.zeros((depth, n, S), dtype=np.int32)
    masks = np.zeros((depth, n, TILES), dtype=bool)
    for r in range(n):
        c = np.nonzero(prev[r] != new[r])[0]
        for k, rc in enumerate(reach(dil, depth)):
            mask = masks[k, r] = marked_tiles(c, L, rc)
            t = cnt = 0
            while t < TILES:
                if not mask[t]:
                    t += 1
                    continue
                ln = 1
                while ln < max_item and t + ln < TILES and mask[t + ln]:
                    ln += 1
                items[k, r, cnt] = t | ln << 8
                cnt, t = cnt + 1, t + ln
    return items, masks


def live_taps(L, T, dil):
    """Taps (0 .. 8) of row tile T that backbone_kernel's schedule keeps for a 9-tap convolution of dilation dil at length L."""
    return [t for t in range(9) if max(0, -(t - 4) * dil) < 16 * T + 16 and min(L, L - (t - 4) * dil) > 16 * T]


def uniform_unmask_shares(dil, depth, L=200, steps=128, rows=256, seed=0):
    """Marked share of the 13 tiles per carried layer, averaged over a decode in which every still-masked position is unmasked at
    step s with probability 1 / (steps - s) (each position's unmasking step is uniform over the decode)."""
    rng = np.random.default_rng(seed)
    rcs = reach(dil, depth)
    total = np.zeros(depth)
    for _ in range(rows):
        when = rng.integers(0, steps, L)
        for s in range(steps):
            c = np.nonzero(when == s)[0]
            for k, rc in enumerate(rcs):
                total[k] += marked_tiles(c, L, rc).sum()
    return total / (rows * steps * TILES)
