"""No GPU: svdd_backbone_incr3_f32 answers SVDD_E_ARG — before its profile span and before any HIP call — for NULL buffers, a depth
outside [lead, nlayers], a carried layer whose dilation is neither 1 (the leading run) nor 4 (the run behind it), and everything
svdd_backbone_incr2_f32 refuses. The numpy restatement of its work list (tests/incr3_ref.py, which the GPU file holds the kernel to)
is checked against a brute force over (changed position, tile position) pairs for all 12 carriable layers and items of at most 1, 2
and 4 tiles, and the uniform unmasking model prints the marked shares the depth estimate rests on."""
import ctypes

import numpy as np

from svdd_amd import _lib
from tests import incr3_ref as R

DIL = (1,) * 8 + (4,) * 4 + (16,) * 4 + (64,) * 4             # the backbone's 20 layers


def test_incr3_rejects_bad_arguments_without_a_gpu():
    L_ = _lib.lib()
    one = ctypes.c_void_p(64)                                # a non-NULL pointer that is never dereferenced

    def call(n=16, L=200, nl=20, dil=DIL, lead=8, depth=12, first=0, max_item=2, ptrs=(one,) * 11):
        d = None if dil is None else (ctypes.c_int * max(1, len(dil)))(*dil)
        x, table0, tiles, vec, w2, out, planes, x_prev, items, order, count = ptrs
        return L_.svdd_backbone_incr3_f32(x, table0, tiles, vec, w2, out, n, L, nl, d, lead, planes, x_prev, items, None, first, max_item,
                                          order, count, depth, None)

    for k in range(11):                                      # each pointer NULL in turn
        assert call(ptrs=tuple(None if i == k else one for i in range(11))) == _lib.E_ARG, k
    bad = (dict(depth=7),                                    # the leading run of dilation-1 layers has 8
           dict(depth=13),                                   # 12 carriable layers: layer 13 has dilation 16
           dict(depth=12, dil=(1,) * 8 + (4, 4, 16, 4) + DIL[12:]),      # a dilation-16 layer inside the carried run
           dict(depth=12, dil=(1,) * 8 + (4, 4, 1, 4) + DIL[12:]),       # a dilation-1 layer behind the leading run
           dict(depth=12, dil=(1,) * 7 + (4,) * 5 + DIL[12:]),           # lead reaches a dilated layer
           dict(depth=21), dict(depth=0), dict(depth=-1), dict(nl=11, dil=DIL[:11], depth=12),
           dict(L=104), dict(L=209), dict(L=0), dict(max_item=3), dict(max_item=0), dict(max_item=8),
           dict(n=0), dict(n=-3), dict(n=65537), dict(nl=0), dict(nl=33, dil=(1,) * 33, depth=8), dict(lead=1, depth=8), dict(lead=0),
           dict(lead=9), dict(dil=None), dict(dil=(1,) * 8 + (0,) * 12, depth=8))
    for kw in bad:
        assert call(**kw) == _lib.E_ARG, kw
        assert call(first=1, **kw) == _lib.E_ARG, kw


def _brute(prev, new, L, rc):
    """[n][13] bool: tile T is marked iff a changed position lies within rc of one of T's positions."""
    out = np.zeros((prev.shape[0], 13), dtype=bool)
    for r in range(prev.shape[0]):
        changed = np.nonzero(prev[r] != new[r])[0].tolist()
        for T in range(13):
            out[r, T] = any(abs(p - q) <= rc for p in changed for q in range(16 * T, min(16 * T + 16, L)))
    return out


def test_work_list_restatement_all_12_layers():
    assert R.reach(DIL, 12) == [8, 12, 16, 20, 24, 28, 32, 36, 52, 68, 84, 100]
    assert R.reach((1, 1, 4, 16), 4) == [8, 12, 28, 92]
    rng = np.random.default_rng(5)
    for L in (105, 193, 200, 208):
        prev = rng.integers(0, 5, (12, L))
        new = prev.copy()
        new[1, 0] += 1
        new[2, L - 1] += 1
        new[3, L // 2] += 1
        new[4, [0, L - 3]] += 1
        new[5, [40, 56]] += 1
        new[6] += 1
        for r in range(7, 12):
            new[r, rng.permutation(L)[:r - 6]] += 1
        for max_item in (1, 2, 4):
            items, masks = R.expected_items(prev, new, L, DIL, 12, max_item)
            assert items.shape == (12, 12, R.slots(max_item))
            for k, rc in enumerate(R.reach(DIL, 12)):
                assert np.array_equal(masks[k], _brute(prev, new, L, rc)), (L, k)
                for r in range(12):
                    rebuilt = np.zeros(13, dtype=bool)
                    ent = items[k, r][items[k, r] != 0]
                    assert np.array_equal(items[k, r, :len(ent)], ent)              # packed from slot 0
                    firsts = ent & 255
                    assert np.all(np.diff(firsts) > 0)
                    for e in ent:
                        t, ln = int(e) & 255, int(e) >> 8
                        assert 1 <= ln <= max_item and not rebuilt[t:t + ln].any()
                        rebuilt[t:t + ln] = True
                    assert np.array_equal(rebuilt, masks[k, r]), (L, k, r)
            assert not masks[:, 0].any() and masks[:, 6, :-(-L // 16)].all() and not masks[:, 6, -(-L // 16):].any()
            assert np.all(masks[1:] >= masks[:-1])                                   # the reach only grows with depth


def test_dilation4_liveness_rule():
    """The (row tile, tap) pairs the one-launch kernel's schedule drops at dilation 4, which the segment kernel must drop too."""
    dropped = {L: {T: sorted(set(range(9)) - set(R.live_taps(L, T, 4))) for T in range(-(-L // 16))} for L in (105, 193, 200, 208)}
    assert dropped[200] == {**{T: [] for T in range(1, 12)}, 0: [0], 12: [6, 7, 8]}            # taps -16 ; +8, +12, +16
    assert dropped[208] == {**{T: [] for T in range(1, 12)}, 0: [0], 12: [8]}
    assert dropped[193] == {**{T: [] for T in range(1, 12)}, 0: [0], 12: [5, 6, 7, 8]}         # one row: taps + 4 .. + 16 leave it
    assert dropped[105] == {**{T: [] for T in range(1, 6)}, 0: [0], 6: [7, 8]}
    for L in (105, 200, 208):
        assert all(R.live_taps(L, T, 1) == list(range(9)) for T in range(-(-L // 16)))         # dilation 1: every pair is live


def test_uniform_unmasking_model_shares():
    sh = R.uniform_unmask_shares(DIL, 12, rows=64)
    stem, deep = float(sh[:8].mean()), float(sh[8:].mean())
    print(f"MODEL marked share: dilation-1 layers {stem:.3f}, dilation-4 layers "
          f"{' / '.join(f'{v:.3f}' for v in sh[8:])} (mean {deep:.3f})")
    assert abs(stem - 0.34) < 0.02 and abs(deep - 0.62) < 0.03
    assert np.all(np.diff(sh) > 0)
