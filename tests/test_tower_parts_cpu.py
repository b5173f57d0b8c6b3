"""The parts of a candidate and the per-layer row ranges of the fp32 windowed tower (svdd_candidate_parts), without a GPU:
  rule        the part rule and the per-layer tile count restated in numpy (part_rule, part_ranges, tile_layers: the GPU test checks the
              kernels against these), on seeded SVDD-like states at masked fractions 0.9, 0.5 and 0.05: at most 3 parts; every
              candidate's tile-layers <= the 6 nt of its tight window — by construction for a gap >= 70, so this is what catches a wrong
              rule; the tiles two parts compute are disjoint on every layer; every layer's computed rows cover what the next layer
              reads of them; the total ratio is printed (pytest -s), not asserted;
  chosen      hand-picked positions: one change costs 4 + 4 + 3 + 3 + 3 + 3 = 20 tile-layers; 69 apart is one part, 70 two; the cap;
  entry       svdd_candidate_parts and svdd_conv_tower_parts_f32 refuse bad arguments before they touch a device."""
import ctypes

import numpy as np

from tests.test_tight_windows_cpu import first_last, svdd_like, tight_windows

REACH, GAP, MAX_PARTS, BLOCKS = 17, 70, 3, 5


def part_rule(cand, x, gap=GAP):
    """cand [B, M, L], x [B, L] -> (parts int32 [n, 3, 2], nparts int32 [n]): the changed positions, ascending, cut wherever two
    consecutive ones are >= gap apart; anything past the third part is merged into it; (-1, -1) where there is no part."""
    d = (cand != x[:, None, :]).reshape(-1, cand.shape[2])
    parts = np.full((d.shape[0], MAX_PARTS, 2), -1, np.int32)
    nparts = np.zeros(d.shape[0], np.int32)
    for c, row in enumerate(d):
        pos = np.flatnonzero(row)
        k = -1
        for i, p in enumerate(pos):
            if i == 0 or (p - pos[i - 1] >= gap and k < MAX_PARTS - 1):
                k += 1
                parts[c, k, 0] = p
            parts[c, k, 1] = p
        nparts[c] = k + 1
    return parts, nparts


def part_ranges(a, b, L, reach=REACH):
    """The needed range [s, e) of the six layers (0 = stem) for one part [a, b]."""
    return [(max(0, a - reach - 2 * (BLOCKS - k)), min(L, b + reach + 1 + 2 * (BLOCKS - k))) for k in range(BLOCKS + 1)]


def layer_tiles(parts, L, reach=REACH):
    """int [n, 6]: 16-row tiles per layer, every range counted from its own first row."""
    out = np.zeros((parts.shape[0], BLOCKS + 1), np.int64)
    for c in range(parts.shape[0]):
        for a, b in parts[c]:
            if a >= 0:
                out[c] += [-(-(e - s) // 16) for s, e in part_ranges(a, b, L, reach)]
    return out


def tile_layers(parts, L, reach=REACH):
    return layer_tiles(parts, L, reach).sum(1).astype(np.int32)


def _check_geometry(parts, L):
    """Disjoint computed tiles on every layer; what layer k + 1 needs to read of layer k lies in layer k's needed range."""
    for c in range(parts.shape[0]):
        live = [(a, b) for a, b in parts[c] if a >= 0]
        rng = [part_ranges(a, b, L) for a, b in live]
        for k in range(BLOCKS + 1):
            spans = [(s, s + 16 * -(-(e - s) // 16)) for s, e in (r[k] for r in rng)]
            for (s0, e0), (s1, e1) in zip(spans, spans[1:]):
                assert e0 <= s1, (c, k, spans)                              # never touch, rounded up from their own start
            assert sum((e - s) // 16 for s, e in spans) <= 13                # the list of tile origins holds them
        for r in rng:
            for k in range(BLOCKS):
                (s, e), (s1, e1) = r[k], r[k + 1]
                assert s <= max(0, s1 - 2) and e >= min(L, e1 + 2), (c, k, r)    # a 5-tap block reads two rows around its needed rows


def test_part_rule_never_costs_more_than_the_tight_window():
    tot = {"old": 0, "layers": 0, "parts": 0}
    for L in (200, 120):
        for masked in (0.9, 0.5, 0.05):
            cand, x = svdd_like(64, 10, L, masked, 128, seed=int(masked * 100) + L)
            lo, hi = first_last(cand, x)
            wt = tight_windows(lo, hi, L)
            old = 6 * (wt[:, 1] - wt[:, 0]) // 16
            one, n_one = part_rule(cand, x, gap=L + 1)                       # per-layer ranges alone
            parts, nparts = part_rule(cand, x)
            live = hi >= 0
            assert live.any() and (~live).any()
            assert (n_one == live).all() and (one[live, 0, 0] == lo[live]).all() and (one[live, 0, 1] == hi[live]).all()
            assert nparts.max() <= MAX_PARTS and ((nparts > 0) == live).all() and (parts[~live] == -1).all()
            t_one, t_parts = tile_layers(one, L), tile_layers(parts, L)
            assert (t_one <= old).all() and (t_parts <= t_one).all()
            assert (t_parts[~live] == 0).all() and (t_parts[live] >= 6).all()
            _check_geometry(parts, L)
            _check_geometry(one, L)
            print(f"L = {L}, masked {masked}: {int(live.sum())} live, {nparts[live].mean():.3f} parts each (max {nparts.max()}); tile-layers "
                  f"window {int(old.sum())}, per-layer {int(t_one.sum())} ({t_one.sum() / old.sum():.4f}), parts {int(t_parts.sum())} "
                  f"({t_parts.sum() / old.sum():.4f})")
            if L == 200:
                tot["old"] += int(old.sum()); tot["layers"] += int(t_one.sum()); tot["parts"] += int(t_parts.sum())
    print(f"L = 200, all three fractions: tile-layers per-layer / window = {tot['layers'] / tot['old']:.4f}, parts / window = "
          f"{tot['parts'] / tot['old']:.4f}")


def test_part_rule_on_chosen_positions():
    L = 200

    def one(*pos, gap=GAP):
        x = np.zeros((1, L), np.uint8)
        cand = x[:, None, :].copy()
        cand[0, 0, list(pos)] = 1
        parts, n = part_rule(cand, x, gap)
        return parts[0].tolist(), int(n[0]), layer_tiles(parts, L)[0].tolist()

    assert one(100) == ([[100, 100], [-1, -1], [-1, -1]], 1, [4, 4, 3, 3, 3, 3])     # 55, 51, 47, 43, 39, 35 rows: 20 tile-layers, not 24
    assert one() == ([[-1, -1]] * 3, 0, [0] * 6)
    assert one(0)[2] == [2, 2, 2, 2, 2, 2] and one(L - 1)[2] == [2, 2, 2, 2, 2, 2]   # 28 .. 18 rows at a sequence end
    assert one(20, 89)[:2] == ([[20, 89], [-1, -1], [-1, -1]], 1)                    # 69 apart: one part
    assert one(20, 90)[:2] == ([[20, 20], [90, 90], [-1, -1]], 2)                    # 70 apart: two
    assert one(0, 70, 140)[:2] == ([[0, 0], [70, 70], [140, 140]], 3)
    assert one(0, 70, 140, 199, gap=70)[:2] == ([[0, 0], [70, 70], [140, 199]], 3)   # 59 apart: the third part anyway
    L = 400                                                                          # (the rule alone: four clusters, the cap)
    assert one(5, 100, 200, 300)[:2] == ([[5, 5], [100, 100], [200, 300]], 3)
    assert one(5, 100, 200, 300, gap=L + 1)[:2] == ([[5, 300], [-1, -1], [-1, -1]], 1)


def test_parts_entries_refuse_bad_arguments_without_a_gpu():
    from svdd_amd import _lib
    L_ = _lib.lib()
    one = ctypes.c_void_p(64)                                 # a non-NULL pointer that is never dereferenced
    assert _lib.SIGNATURES["svdd_candidate_parts"][-1] is _lib.vp and _lib.SIGNATURES["svdd_conv_tower_parts_f32"][-1] is _lib.vp

    def parts_entry(cand=one, x=one, B=1, L=200, M=1, reach=17, gap=70, parts=one):
        return L_.svdd_candidate_parts(cand, x, B, L, M, reach, gap, parts, None, None, None, None)
    for kw in (dict(cand=None), dict(x=None), dict(parts=None), dict(B=0), dict(B=-1), dict(L=0), dict(M=0), dict(reach=-1),
               dict(reach=(1 << 20) + 1), dict(gap=69), dict(gap=0), dict(reach=18, gap=71), dict(B=1 << 16, M=1 << 15), dict(B=(1 << 31) - 3)):
        assert parts_entry(**kw) == _lib.E_ARG, kw

    def tower_entry(onehot=one, tiles=one, bias=one, parts=one, parent_out=one, out=one, n=8, L=200, M=8, nlayers=5, reach=17, live_idx=None):
        return L_.svdd_conv_tower_parts_f32(onehot, tiles, bias, parts, parent_out, out, n, L, M, nlayers, 0, reach, live_idx, None, None)
    for kw in (dict(onehot=None), dict(tiles=None), dict(bias=None), dict(parts=None), dict(parent_out=None), dict(out=None), dict(n=0),
               dict(M=0), dict(n=7), dict(L=104), dict(L=209), dict(nlayers=4), dict(nlayers=6), dict(reach=-1), dict(reach=16), dict(reach=18), dict(reach=(1 << 20) + 1)):
        assert tower_entry(**kw) == _lib.E_ARG, kw
