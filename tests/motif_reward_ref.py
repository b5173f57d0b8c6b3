"""numpy restatement of svdd_motif_reward and svdd_amd.motifs.MotifReward, written from the contract in
include/svdd_hip.h on top of tests/motif_ref.py's per-window scores: the integer term T of a row as Python-exact int64, the two
fp32 operations that turn it into a score, the quantisation of float weights and the default margin floor. Nothing here shares
code with the module."""
from types import SimpleNamespace

import numpy as np

from tests import motif_ref as R


def term_ref(x, mset, hit_coef, hit_cap, margin_coef, margin_floor, both=True):
    """x [N, L] tokens (a token > 3 reads as 0), mset with width / pwm / threshold -> T int64 [N]:
    sum_m hit_coef_m min(hits_m, hit_cap_m) + margin_coef_m max(min(best_m - threshold_m, 0), -margin_floor_m); no window (L < w):
    no hits and the margin -margin_floor_m."""
    x = np.asarray(x, np.int64)
    x = np.where(x > 3, 0, x)
    T = np.zeros(x.shape[0], np.int64)
    for m in range(len(mset.width)):
        w, thr = int(mset.width[m]), int(mset.threshold[m])
        hc, cap, mc, fl = (int(a[m]) for a in (hit_coef, hit_cap, margin_coef, margin_floor))
        f, r = R.window_scores_ref(x, mset.pwm[m], w)
        if f.shape[1] == 0:
            T += mc * -fl
            continue
        hits = (f >= thr).sum(1) + ((r >= thr).sum(1) if both else 0)
        best = np.maximum(f.max(1), r.max(1)) if both else f.max(1)
        T += hc * np.minimum(hits, cap) + mc * np.maximum(np.minimum(best - thr, 0), -fl)
    return T


def score_ref(T, unit, base=None):
    """fp32 [N]: base + float(T) * unit, one rounding per operation (the int64 -> fp32 conversion rounds to nearest even)."""
    t = np.asarray(T, np.int64).astype(np.float32) * np.float32(unit)
    return t if base is None else (np.asarray(base, np.float32) + t).astype(np.float32)


def quantise_ref(weights, unit):
    """round-half-even(weight / unit) as Python ints."""
    return [int(round(float(w) / float(unit))) for w in weights]


def default_floor_ref(mset):
    """threshold minus the lowest score a window of the motif can have, not below 0."""
    out = []
    for m in range(len(mset.width)):
        low = sum(int(min(col)) for col in np.asarray(mset.pwm[m][:int(mset.width[m])], np.int64))
        out.append(max(int(mset.threshold[m]) - low, 0))
    return out


def bound_ref(hit_coef, hit_cap, margin_coef, margin_floor):
    return sum(abs(int(h)) * int(c) + abs(int(g)) * int(f) for h, c, g, f in zip(hit_coef, hit_cap, margin_coef, margin_floor))


def random_case(rng, widths, lo=-120, hi=120, frac=0.35):
    """A motif set of the given widths with random int16 tables (garbage beyond each width, which nobody may read) and thresholds
    at `frac` of the highest score, plus coefficients that exercise every branch: negative ones, a hit cap of 0, caps that bind and caps
    that never do (the term then follows the exact hit count), a margin floor of 0."""
    M = len(widths)
    pwm = rng.integers(lo, hi + 1, (M, 32, 4)).astype(np.int16)
    width = np.asarray(widths, np.int32)
    live = np.arange(32)[None, :, None] < width[:, None, None]
    top = np.where(live, pwm.astype(np.int64), 0).max(2).sum(1)
    mset = SimpleNamespace(width=width, pwm=pwm, threshold=np.rint(frac * top).astype(np.int32))
    coefs = SimpleNamespace(hit_coef=rng.integers(-5000, 5001, M).astype(np.int32), hit_cap=rng.choice([0, 1, 2, 3, 40, 100000], M).astype(np.int32),
                            margin_coef=rng.integers(-40, 41, M).astype(np.int32),
                            margin_floor=np.where(rng.random(M) < 0.25, 0, rng.integers(0, 600, M)).astype(np.int32))
    return mset, coefs
