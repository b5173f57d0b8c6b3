"""The tight candidate windows of the fp32 windowed tower (svdd_candidate_windows_tight), without a GPU:
  formula     the window rule restated in numpy, on seeded SVDD-like states at masked fractions 0.9, 0.5 and 0.05: every window covers
              [lo - 27, hi + 27] inside the sequence, its length is a multiple of 16, it never has more row tiles than the 16-aligned
              window of svdd_candidate_windows, a copy gets (0, 0); the total tile ratio tight / aligned is printed (pytest -s) — the
              figure recorded in profiles/step_trim_bench_ab.txt;
  entry       svdd_candidate_windows_tight refuses bad arguments before it touches a device."""
import ctypes

import numpy as np

MARGIN, MASK = 27, 4


def first_last(cand, x):
    """cand [B, M, L], x [B, L] -> (lo, hi) int arrays [B * M]: first and last position where a candidate differs from its parent,
    hi = -1 for an exact copy."""
    d = (cand != x[:, None, :]).reshape(-1, cand.shape[2])
    L = d.shape[1]
    any_ = d.any(1)
    lo = np.where(any_, d.argmax(1), 0)
    hi = np.where(any_, L - 1 - d[:, ::-1].argmax(1), -1)
    return lo, hi


def aligned_windows(lo, hi, L, margin=MARGIN):
    """svdd_candidate_windows: both ends multiples of 16."""
    w0 = np.maximum(0, lo - margin) & ~15
    w1 = np.minimum((L + 15) & ~15, (hi + margin + 1 + 15) & ~15)
    live = hi >= 0
    return np.stack([np.where(live, w0, 0), np.where(live, w1, 0)], 1).astype(np.int32)


def tight_windows(lo, hi, L, margin=MARGIN):
    """svdd_candidate_windows_tight: w0 = max(0, lo - margin), w1 = w0 + 16 ceil((min(L, hi + margin + 1) - w0) / 16)."""
    w0 = np.maximum(0, lo - margin)
    w1 = w0 + 16 * -(-(np.minimum(L, hi + margin + 1) - w0) // 16)
    live = hi >= 0
    return np.stack([np.where(live, w0, 0), np.where(live, w1, 0)], 1).astype(np.int32)


def svdd_like(B, M, L, masked, steps, seed):
    """Parents with the given masked fraction and their candidates: every masked position of a candidate is unmasked with probability
    1 / (steps * masked) — what one of `steps` reverse steps does at that point of the log-linear schedule (L / steps changes expected)."""
    g = np.random.default_rng(seed)
    x = g.integers(0, 4, (B, L)).astype(np.uint8)
    x[g.random((B, L)) < masked] = MASK
    flip = (g.random((B, M, L)) < 1.0 / (steps * masked)) & (x == MASK)[:, None, :]
    cand = np.where(flip, g.integers(0, 4, (B, M, L)), x[:, None, :]).astype(np.uint8)
    return cand, x


def test_tight_window_formula_covers_and_never_costs_more():
    total_t = total_a = 0
    for L in (200, 120):
        for masked in (0.9, 0.5, 0.05):
            cand, x = svdd_like(64, 10, L, masked, 128, seed=int(masked * 100) + L)
            lo, hi = first_last(cand, x)
            wt, wa = tight_windows(lo, hi, L), aligned_windows(lo, hi, L)
            live = hi >= 0
            assert live.any() and (~live).any()
            assert (wt[~live] == 0).all() and (wa[~live] == 0).all()
            t0, t1, a0, a1 = wt[live, 0], wt[live, 1], wa[live, 0], wa[live, 1]
            assert (t0 <= np.maximum(0, lo[live] - MARGIN)).all() and (t1 >= np.minimum(L, hi[live] + MARGIN + 1)).all()     # covers
            assert (t0 >= 0).all() and ((t1 - t0) % 16 == 0).all() and (t1 > t0).all()
            assert ((t1 - t0) // 16 <= (L + 15) // 16).all()                              # the LDS image holds ceil(L / 16) tiles
            assert (t1 - t0 <= a1 - a0).all()                                             # never more tiles than the aligned window
            assert (t0 >= a0).all() and (t1 < a1 + 16).all()
            nt, na = int((t1 - t0).sum()) // 16, int((a1 - a0).sum()) // 16
            print(f"L = {L}, masked {masked}: {int(live.sum())} live candidates, row tiles tight {nt} / aligned {na} = {nt / na:.4f} "
                  f"({(na - nt) / live.sum():.3f} tiles less per window, {nt / live.sum():.2f} tiles per window)")
            if L == 200:
                total_t, total_a = total_t + nt, total_a + na
    print(f"L = 200, all three fractions: total tile ratio tight / aligned = {total_t / total_a:.4f}")
    assert total_t < total_a


def test_tight_window_formula_on_chosen_positions():
    """One change at lo: 55 rows = 4 tiles wherever it starts (the aligned window takes 5 at 6 of the 16 start offsets); the sequence
    ends; two far changes; a copy."""
    L = 200
    for r in range(16):
        lo = np.array([27 + 32 + r])
        wt, wa = tight_windows(lo, lo, L)[0], aligned_windows(lo, lo, L)[0]
        assert tuple(wt) == (32 + r, 32 + r + 64) and (wa[1] - wa[0]) // 16 == (5 if r > 9 else 4)
    assert tuple(tight_windows(np.array([5]), np.array([5]), L)[0]) == (0, 48)
    assert tuple(tight_windows(np.array([190]), np.array([190]), L)[0]) == (163, 211)      # w1 passes L rounded up (208), 3 tiles
    assert tuple(tight_windows(np.array([20]), np.array([170]), L)[0]) == (0, 208)
    assert tuple(tight_windows(np.array([30]), np.array([199]), L)[0]) == (3, 211)         # 197 rows: 13 tiles, the most
    assert tuple(tight_windows(np.array([0]), np.array([-1]), L)[0]) == (0, 0)


def test_tight_windows_entry_refuses_bad_arguments_without_a_gpu():
    from svdd_amd import _lib
    L_ = _lib.lib()
    one = ctypes.c_void_p(64)                                 # a non-NULL pointer that is never dereferenced
    assert "svdd_candidate_windows_tight" in _lib.EXPORTS and _lib.SIGNATURES["svdd_candidate_windows_tight"][-1] is _lib.vp

    def entry(cand=one, x=one, B=1, L=200, M=1, margin=27, win=one, flags=None):
        return L_.svdd_candidate_windows_tight(cand, x, B, L, M, margin, win, flags, None)
    for kw in (dict(cand=None), dict(x=None), dict(win=None), dict(B=0), dict(B=-1), dict(L=0), dict(M=0), dict(margin=-1),
               dict(margin=(1 << 20) + 1), dict(B=1 << 16, M=1 << 15)):
        assert entry(**kw) == _lib.E_ARG, kw
    assert L_.svdd_candidate_windows_tight(None, None, 0, 0, 0, 0, None, None, None) == _lib.E_ARG
