"""No GPU: the tight work list of svdd_backbone_incr4_f32 as tests/incr4_ref.py restates it (the GPU file holds the kernel to that
restatement). For L = 105, 200, 208 and seeded change sets, per (dilation-1 layer, row): every run of reached rows is covered; the
tiles are disjoint with origins < L; at most SEG_SLOTS items of at most max_item adjacent tiles; the fallback to aligned tiles fires
on the constructed 8-item case and on nothing a single changed position produces; the tiles cut are never more than the aligned
tiles. The ratio tight / aligned on SVDD-like steps at masked fractions 0.9, 0.5 and 0.05 is printed (pytest -s), not asserted.
The entry's binding: an explicit stream (`vp`) as its last parameter, ABI 17, SVDD_E_ARG before any HIP call."""
import ctypes

import numpy as np

from svdd_amd import _lib
from tests import incr3_ref as R3
from tests import incr4_ref as R

DIL = (1,) * 8 + (4,) * 4 + (16,) * 4 + (64,) * 4
LEAD = 8
REACH = R3.reach(DIL, LEAD)


def _check_row(changed, L, rc, max_item=2):
    """The properties of one (layer, row). -> (tiles cut, aligned tiles, fallback)."""
    items, fb = R.row_items(changed, L, rc, max_item)
    aligned = R.aligned_tiles(changed, L, rc)
    assert len(items) <= R.SEG_SLOTS, (changed, L, rc)
    covered = np.zeros(L + 16, dtype=np.int32)
    for o, ln in items:
        assert 0 <= o < L and 1 <= ln <= max_item and (not fb or o % 16 == 0), (changed, L, rc, items)
        assert (o | ln << 8) != 0 and o < 256
        covered[o:o + 16 * ln] += 1
    assert covered.max(initial=0) <= 1, ("tiles overlap", changed, L, rc, items)
    for (o, ln), (o2, _) in zip(items, items[1:]):
        assert o + 16 * ln <= o2                                            # in row order
        assert ln == max_item or o + 16 * ln < o2                           # a run is cut only where it is full
    for a, b in R.extents(changed, L, rc):
        assert covered[a:b + 1].all(), ("a reached row is not covered", changed, L, rc, items)
    for p in changed:
        assert covered[max(0, p - rc):min(L - 1, p + rc) + 1].all()
    tiles = sum(ln for _, ln in items)
    assert tiles <= len(aligned) <= 13, (changed, L, rc, items)
    assert fb == (len(R.cut(R.tight_tiles(R.extents(changed, L, rc)), max_item)) > R.SEG_SLOTS)
    return tiles, len(aligned), fb


def test_reach_of_the_tight_layers():
    assert REACH == [8, 12, 16, 20, 24, 28, 32, 36]
    assert [2 * rc + 1 for rc in REACH] == [17, 25, 33, 41, 49, 57, 65, 73]


def test_single_changed_position_never_falls_back():
    saved = {L: [0, 0] for L in (105, 200, 208)}
    for L in saved:
        for p in range(L):
            for rc in REACH:
                tiles, aligned, fb = _check_row([p], L, rc)
                assert not fb
                lo, hi = max(0, p - rc), min(L - 1, p + rc)
                assert tiles == -(-(hi - lo + 1) // 16)                         # the run, started at its first row
                saved[L][0] += tiles
                saved[L][1] += aligned
    # one position, all eight layers, away from the ends: 28 tiles, against (r - 1) / 16 + 1 aligned tiles per run of r rows on
    # average over the position: 30 in all, so a lone change saves 2 tile-layers of 30
    assert sum(-(-(2 * rc + 1) // 16) for rc in REACH) == 28
    mid = [sum(_check_row([p], 200, rc)[1] for rc in REACH) for p in range(48, 64)]
    assert np.mean(mid) == sum(2 * rc / 16 + 1 for rc in REACH) == 30.0
    for L, (t, a) in saved.items():
        print(f"L = {L}, one changed position, every position: tight / aligned tile-layers = {t} / {a} = {t / a:.4f}")


def test_merge_rule():
    # reach 8: positions 17 apart give runs [32, 48] and [49, 65] that touch: ONE run of 34 rows, 3 tiles from row 32
    assert R.extents([40, 57], 200, 8) == [(32, 65)] and R.tight_tiles([(32, 65)]) == [32, 48, 64]
    # 33 apart: runs [32, 48] and [65, 81]; the tile at 48 holds rows .. 63 and does not reach 65: the second run starts its own cover
    assert R.extents([40, 73], 200, 8) == [(32, 48), (65, 81)] and R.tight_tiles([(32, 48), (65, 81)]) == [32, 48, 65, 81]
    assert R.cut([32, 48, 65, 81], 2) == [(32, 2), (65, 2)]
    # 30 apart: runs [32, 48] and [62, 78]; the tile at 48 reaches row 62, so the second run continues the same cover at 64
    assert R.tight_tiles(R.extents([40, 70], 200, 8)) == [32, 48, 64]
    assert R.row_items([40, 70], 200, 8) == ([(32, 2), (64, 1)], False)
    # both ends of the sequence: an item at origin 0 is a non-zero word; the last origin stays below L
    assert R.row_items([0], 200, 8) == ([(0, 1)], False) and R.row_items([199], 200, 8) == ([(191, 1)], False)
    assert R.row_items([104], 105, 36) == ([(68, 2), (100, 1)], False)


def test_fallback_fires_on_the_eight_item_case():
    pos = R.fallback_clusters(200)
    for L in (200, 208):
        tight = R.cut(R.tight_tiles(R.extents(pos, L, 8)), 2)
        assert [ln for _, ln in tight] == [2, 1] * 4                            # four 3-tile runs cut 2 + 1 each: 8 items
        items, fb = R.row_items(pos, L, 8)
        assert fb and all(o % 16 == 0 for o, _ in items) and len(items) <= R.SEG_SLOTS
        _check_row(pos, L, 8)
        assert not _check_row(pos, L, 36)[2]                                    # the widest reach merges them into one run
        assert not _check_row(pos[:6], L, 8)[2]                                 # three clusters: 6 items fit


def test_seeded_change_sets_and_the_ratio():
    """SVDD-like steps: a row holds a masked share of its positions and a step of a 128-step decode unmasks each masked position
    with probability 1 / (steps left)."""
    tot = [0, 0]
    for L in (105, 200, 208):
        for masked in (0.9, 0.5, 0.05):
            rng = np.random.default_rng(int(masked * 100) + L)
            tight = aligned = falls = 0
            for _ in range(96):
                is_masked = rng.random(L) < masked
                changed = np.flatnonzero(is_masked & (rng.random(L) < 1.0 / max(1.0, masked * 128))).tolist()
                for rc in REACH:
                    t, a, fb = _check_row(changed, L, rc)
                    tight, aligned, falls = tight + t, aligned + a, falls + fb
            assert 0 < tight <= aligned
            print(f"L = {L}, masked {masked}: tile-layers tight {tight}, aligned {aligned} ({tight / aligned:.4f}), {falls} fallbacks")
            if L == 200:
                tot[0] += tight; tot[1] += aligned
    print(f"L = 200, all three fractions: tight / aligned = {tot[0] / tot[1]:.4f}")
    # dense and adversarial sets: everything changed, every 16th / 17th / 33rd / 49th position
    for L in (105, 200, 208):
        for changed in (list(range(L)), list(range(0, L, 16)), list(range(3, L, 17)), list(range(5, L, 33)), list(range(7, L, 49)),
                        [0, L - 1], []):
            for rc in REACH:
                _check_row(changed, L, rc)
                _check_row(changed, L, rc, max_item=4)


def test_expected_items_joins_both_lists():
    rng = np.random.default_rng(9)
    L = 200
    prev = rng.integers(0, 5, (4, L))
    new = prev.copy()
    new[1, [40, 57]] += 1
    new[2, R.fallback_clusters(L)] += 1
    new[3, rng.permutation(L)[:5]] += 1
    items, tiles, fb = R.expected_items(prev, new, L, DIL, LEAD, 10)
    deep, masks = R3.expected_items(prev, new, L, DIL, 10, 2)
    assert items.shape == (10, 4, 7) and not items[:, 0].any() and not tiles[:, 0].any()
    assert np.array_equal(items[LEAD:], deep[LEAD:]) and np.array_equal(tiles[LEAD:], masks[LEAD:].sum(-1))
    assert fb[0, 2] and not fb[2:, 2].any() and not fb[:, [0, 1, 3]].any()
    assert np.array_equal(items[0, 2], 16 * (deep[0, 2] & 255) | (deep[0, 2] >> 8) << 8)          # the aligned items as origins
    assert items[0, 1].tolist() == [32 | 2 << 8, 64 | 1 << 8, 0, 0, 0, 0, 0]
    assert (tiles[:LEAD] <= masks[:LEAD].sum(-1)).all()


def test_binding_and_argument_checks():
    sig = _lib.SIGNATURES["svdd_backbone_incr4_f32"]
    assert "svdd_backbone_incr4_f32" in _lib.EXPORTS and sig[-1] is _lib.vp and sig[-1] is not _lib.STREAM
    assert sig == _lib.SIGNATURES["svdd_backbone_incr3_f32"][:-1] + (_lib.vp, _lib.i32, _lib.vp)
    L_ = _lib.lib()
    assert _lib.ABI_VERSION == 17 and L_.svdd_abi_version() == 17
    one, two = ctypes.c_void_p(64), ctypes.c_void_p(128)        # non-NULL pointers that are never dereferenced

    def call(n=16, L=200, nl=20, dil=DIL, lead=8, depth=10, first=0, max_item=2, parity=0, ptrs=(one,) * 11 + (two,)):
        d = None if dil is None else (ctypes.c_int * max(1, len(dil)))(*dil)
        x, table0, tiles, vec, w2, out, planes, x_prev, items, order, count, x_prev2 = ptrs
        return L_.svdd_backbone_incr4_f32(x, table0, tiles, vec, w2, out, n, L, nl, d, lead, planes, x_prev, items, None, first, max_item,
                                          order, count, depth, x_prev2, parity, None)

    for k in range(12):                                          # each pointer NULL in turn
        assert call(ptrs=tuple(None if i == k else (two if i == 11 else one) for i in range(12))) == _lib.E_ARG, k
    bad = (dict(ptrs=(one,) * 12),                               # the two token buffers are one buffer
           dict(max_item=1), dict(max_item=4), dict(max_item=3), dict(parity=2), dict(parity=-1),
           dict(depth=7), dict(depth=13), dict(depth=12, dil=(1,) * 8 + (4, 4, 16, 4) + DIL[12:]), dict(lead=1, depth=8), dict(lead=9),
           dict(L=104), dict(L=209), dict(n=0), dict(n=65537), dict(nl=0), dict(dil=None))
    for kw in bad:
        assert call(**kw) == _lib.E_ARG, kw
        assert call(first=1, **kw) == _lib.E_ARG, kw
