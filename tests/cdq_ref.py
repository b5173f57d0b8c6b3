"""numpy restatements of the step boundary of a CD-Q rollout (svdd_value_target, include/svdd_hip.h) and of the training set the
reference builds from its draws (Enformer.py:226-259): the sequential fp32 mean, the log-mean-exp in float64 and in fp32, the
continuation token row with its one-hot, and the step-major assembly of (states, y). Test infrastructure: lives under tests/, not
in the product package."""
import numpy as np

MASK = 4


def seq_mean_f32(scores):
    """[..., M] -> [...] f32: fl(fl(...fl(fl(0 + s_0) + s_1)... + s_{M-1}) / fl(M)), the reference's `case_sum = case_sum + v` over
    the draws followed by `case_sum / len(time_samples)` (Enformer.py:235-238). One fp32 rounding per operation, ascending m."""
    s = np.asarray(scores, np.float32)
    acc = np.zeros(s.shape[:-1], np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for m in range(s.shape[-1]):
            acc = (acc + s[..., m]).astype(np.float32)
        return (acc / np.float32(s.shape[-1])).astype(np.float32)


def _logmeanexp(scores, alpha, ft):
    s = np.asarray(scores, np.float32).astype(ft)
    a = ft(np.float32(alpha))
    M = s.shape[-1]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        mx = np.max(s, axis=-1)                                               # a NaN propagates through np.max
        acc = np.zeros(s.shape[:-1], ft)
        for m in range(M):
            acc = (acc + np.exp(((s[..., m] - mx) / a).astype(ft)).astype(ft)).astype(ft)
        out = (mx + (a * np.log((acc / ft(M)).astype(ft)).astype(ft)).astype(ft)).astype(ft)
    nan = np.isnan(s).any(axis=-1)
    out = np.where(np.isinf(mx), mx, out)                                     # mx = +inf -> +inf ; all -inf -> -inf
    return np.where(nan, ft(np.nan), out).astype(ft)


def logmeanexp_f64(scores, alpha):
    """alpha log mean exp(s / alpha) over the last axis of the fp32 scores, evaluated in float64 (the reference for the kernel's
    finite rows). A NaN score gives NaN, a +inf score +inf, all -inf gives -inf."""
    return _logmeanexp(scores, alpha, np.float64)


def logmeanexp_f32(scores, alpha):
    """The same formula with one fp32 rounding per operation, in the kernel's order: what fp32 can deliver."""
    return _logmeanexp(scores, alpha, np.float32)


def x_next(cand):
    """cand u8 [B, M, L] -> the row a CD-Q rollout continues from: the LAST draw (diffusion_gosai.py:845-851)."""
    return np.ascontiguousarray(np.asarray(cand, np.uint8)[:, -1])


def onehot(x):
    """tokens [..., L] -> f32 [..., L, 4], MASK (and anything above 3) rows zero: transform_samples."""
    x = np.asarray(x)
    return (x[..., None] == np.arange(4)).astype(np.float32)


def boundary(cand, scores=None, reduce="mean", alpha=1.0):
    """The whole launch -> dict(x_next, onehot_next, target | None)."""
    xn = x_next(cand)
    t = None
    if scores is not None:
        t = seq_mean_f32(scores) if reduce == "mean" else logmeanexp_f32(scores, alpha)
    return dict(x_next=xn, onehot_next=onehot(xn), target=t)


def assemble_cdq(all_mid, values, final, reward, reduce=seq_mean_f32):
    """The reference's CD-Q training set from a recorded rollout: all_mid [S, draws, B, L] (all_time_mid_x), values [S, draws, B]
    (the value net on every draw), final [B, L] (x_0), reward [B] -> (states u8 [S, B, L], y f32 [S B]), step-major like the
    reference's torch.cat (Enformer.py:249-254): states[k] = mid_x[k] = the last draw of step k for k < S - 1, states[S - 1] = x_0;
    y[k B + b] = reduce(values[k + 1, :, b]) for k < S - 1 (step 0's values are never used, :233-234), y[(S - 1) B + b] = reward[b]."""
    all_mid, values = np.asarray(all_mid, np.uint8), np.asarray(values, np.float32)
    S = all_mid.shape[0]
    states = np.concatenate([all_mid[:S - 1, -1], np.asarray(final, np.uint8)[None]], axis=0)
    y = [reduce(values[k + 1].T) for k in range(S - 1)] + [np.asarray(reward, np.float32)]
    return states, np.concatenate(y).astype(np.float32)


def assemble_mc(mid, final, reward):
    """The Monte-Carlo training set (Enformer.py:192-218): states = mid_x + [x_0], every state regressed onto r(x_0)."""
    states = np.concatenate([np.asarray(mid, np.uint8), np.asarray(final, np.uint8)[None]], axis=0)
    return states, np.tile(np.asarray(reward, np.float32), states.shape[0])
