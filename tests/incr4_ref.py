"""What tests/test_backbone_incr4_cpu.py and tests/test_backbone_incr4_gpu.py share: a numpy restatement of the work list of
svdd_backbone_incr4_f32 — the tight cover of the dilation-1 layers (maximal runs of reached rows, 16-row tiles from each run's first
row, a run the cover has reached joins it), the cut into items, the fallback to aligned tiles where the cut needs more than SEG_SLOTS
items — on top of tests/incr3_ref.py, which states the aligned list of the deeper layers."""
import numpy as np

from tests import incr3_ref as R3

SEG_SLOTS = 7


def extents(changed, L, rc):
    """The maximal runs [a, b] of rows within rc of a changed position, in row order."""
    hit = np.zeros(L + 2, dtype=np.int8)
    for p in changed:
        hit[1 + max(0, p - rc):1 + min(L - 1, p + rc) + 1] = 1
    edge = np.flatnonzero(np.diff(hit))
    return [(int(a), int(b) - 1) for a, b in zip(edge[::2], edge[1::2])]


def tight_tiles(ext):
    """Tile origins of the cover: a, a + 16, .. per run; a run whose first row the last tile holds continues behind that tile."""
    tiles = []
    for a, b in ext:
        o = tiles[-1] + 16 if tiles and tiles[-1] + 15 >= a else a
        while o <= b:
            tiles.append(o)
            o += 16
    return tiles


def aligned_tiles(changed, L, rc):
    """Origins 16 T of the marked tiles of svdd_backbone_incr3_f32."""
    return [16 * int(T) for T in np.flatnonzero(R3.marked_tiles(np.asarray(changed, dtype=np.int64), L, rc))]


def cut(tiles, max_item):
    """[(origin, tiles)]: runs of adjacent tiles (origins 16 apart) cut to at most max_item."""
    items = []
    for o in tiles:
        if items and items[-1][1] < max_item and o == items[-1][0] + 16 * items[-1][1]:
            items[-1] = (items[-1][0], items[-1][1] + 1)
        else:
            items.append((o, 1))
    return items


def row_items(changed, L, rc, max_item=2):
    """One (dilation-1 layer, row): ([(origin, tiles)], fallback) — the tight items, or the aligned ones where tight needs > 7."""
    items = cut(tight_tiles(extents(changed, L, rc)), max_item)
    if len(items) <= SEG_SLOTS:
        return items, False
    return cut(aligned_tiles(changed, L, rc), max_item), True


def expected_items(prev, new, L, dil, lead, depth, max_item=2):
    """prev, new [n][L] -> (items [depth][n][7] int32, tiles [depth][n] the tiles cut, fallback [lead][n] bool). Layers <= lead:
    origin | tiles << 8 of row_items; deeper layers: first tile | tiles << 8 of incr3_ref.expected_items."""
    prev, new = np.asarray(prev), np.asarray(new)
    n = prev.shape[0]
    items, masks = R3.expected_items(prev, new, L, dil, depth, max_item)
    tiles = masks.sum(-1).astype(np.int64)
    fallback = np.zeros((lead, n), dtype=bool)
    for r in range(n):
        c = np.flatnonzero(prev[r] != new[r]).tolist()
        for k, rc in enumerate(R3.reach(dil, lead)):
            got, fallback[k, r] = row_items(c, L, rc, max_item)
            items[k, r] = 0
            for s, (o, ln) in enumerate(got):
                items[k, r, s] = o | ln << 8
            tiles[k, r] = sum(ln for _, ln in got)
    return items, tiles, fallback


def fallback_clusters(L):
    """Changed positions that force the slot fallback in the first dilation-1 layer (reach 8): a cluster is two positions 16 apart,
    one run of 33 rows = 3 tiles, cut 2 + 1; four clusters 51 rows apart stay separate runs whose tiles are not adjacent: 8 items.
    (Shorter sequences cannot hold them: at L = 105 a row has at most 7 tiles.)"""
    assert L >= 200
    return [p for c in (8, 59, 110, 161) for p in (c, c + 16)]
