"""numpy restatement of Ledidi design: the specification svdd_ledidi_step and Diffusion.ledidi are held to.

  Cfg                the hyper-parameters; dtype np.float32 = the kernel's arithmetic (every derived constant computed in float64 and
                     rounded once, every operation below rounded once, exp / log as float32(f(float64)): the arithmetic contract),
                     dtype np.float64 = the same program in float64
  counters/uniforms  the Philox4x32-10 counter layout of the sampling and its uniforms
  sample             one design's S Gumbel-softmax samples: hard tokens (first argmax), softmax y, edit counts
  losses             output / input / total loss of one design's iteration
  update             the weight gradient through the straight-through estimator and one AdamW step
  step               ONE svdd_ledidi_step launch on a State, in the kernel's order (what is written and what is left alone)
  run                the host loop around a scoring function and a gradient function (a device one or a torch one), one round trip
                     per iteration: what Diffusion.ledidi computes without one

alt=True evaluates the same formulas in another association (samples in descending order, the four-channel sums pairwise): a second
fp32 form whose distance from float64 is the yardstick of the fp32-against-float64 comparison."""
import math

import numpy as np

BETAS, ADAM_EPS, WEIGHT_DECAY = (0.9, 0.999), 1e-8, 0.01           # torch.optim.AdamW's defaults
LEDIDI_STREAM = 4                                                 # low byte of counter word 3
EXISTING_STREAM_WORDS = (0, 1, 2, 3)                              # word 3 (as a whole) of propose, re-mask, multinomial select, ELBO


class Cfg:
    def __init__(self, S, tau=1.0, l=0.1, lr=1.0, eps=1e-4, patience=100, dtype=np.float32):
        f = self.dtype = dtype
        self.S, self.patience, self.lr = int(S), int(patience), float(lr)
        self.tau, self.l = f(tau), f(l)
        self.la, self.lb = f(math.log(1.0 + eps)), f(math.log(eps))
        self.decay, self.w1, self.beta2, self.w2 = f(1.0 - lr * WEIGHT_DECAY), f(1.0 - BETAS[0]), f(BETAS[1]), f(1.0 - BETAS[1])
        self.adam_eps = f(ADAM_EPS)

    def step(self, i):
        """(step_size, bc2_sqrt) of the AdamW step that closes iteration i (step count i + 1)."""
        t = i + 1
        return self.dtype(self.lr / (1.0 - BETAS[0] ** t)), self.dtype(math.sqrt(1.0 - BETAS[1] ** t))


def _exp(x, f):
    return np.exp(np.asarray(x, np.float64)).astype(f)


def _log(x, f):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.log(np.asarray(x, np.float64)).astype(f)


# ---------------------------------------------------------------------------------------------------------- Philox ----
def philox4x32_10(c, k0, k1):
    """c uint32 [..., 4] -> uint32 [..., 4]; key (k0, k1)."""
    c0, c1, c2, c3 = (c[..., i].astype(np.uint64) for i in range(4))
    m32 = np.uint64(0xFFFFFFFF)
    k0, k1 = np.uint64(k0 & 0xFFFFFFFF), np.uint64(k1 & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def counters(row, it, S, L):
    """The counter blocks [S, L, 4] uint32 of design `row` (= row_offset + d, 64 bits) at iteration `it` (32 bits):
    (row low, row high, it, s << 20 | j << 8 | LEDIDI_STREAM)."""
    assert 0 <= it < 2 ** 32 and 0 <= row < 2 ** 64 and S <= 64 and L <= 1024
    c = np.empty((S, L, 4), np.uint32)
    c[..., 0], c[..., 1], c[..., 2] = row & 0xFFFFFFFF, (row >> 32) & 0xFFFFFFFF, it
    c[..., 3] = (np.arange(S, dtype=np.uint32)[:, None] << 20) | (np.arange(L, dtype=np.uint32)[None, :] << 8) | LEDIDI_STREAM
    return c


def uniforms(seed, row, it, S, L):
    """fp32 [S, L, 4]: the four words' top 24 bits of block (row, it, s, j) are channels 0..3."""
    r = philox4x32_10(counters(row, it, S, L), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return (r >> 8).astype(np.float32) * np.float32(1.0 / 16777216.0)


# ---------------------------------------------------------------------------------------------------- one design ----
def onehot(tok):
    return (tok[..., None] == np.arange(4, dtype=tok.dtype)).astype(np.float32)


def _sum4(a, alt):
    return (a[..., 3] + a[..., 2]) + (a[..., 1] + a[..., 0]) if alt else ((a[..., 0] + a[..., 1]) + a[..., 2]) + a[..., 3]


def sample(x0, editable, w, u, cfg, alt=False):
    """x0 u8 [L], editable bool [L], w [L, 4], u fp32 [S, L, 4] -> (tok u8 [S, L], y [S, L, 4] (0 at frozen positions), edits [S])."""
    f = cfg.dtype
    base = np.where(np.arange(4)[None, :] == x0[:, None], cfg.la, cfg.lb).astype(f)
    e = f(1e-10) - _log(u.astype(f) + f(1e-10), f)
    g = -_log(e, f)
    zt = ((base[None] + w[None].astype(f)) + g) / cfg.tau
    best, mx = np.zeros(zt.shape[:2], np.int64), zt[..., 0].copy()
    for c in range(1, 4):                                          # the first maximum: a later channel wins only if strictly greater
        gt = zt[..., c] > mx
        mx, best = np.where(gt, zt[..., c], mx), np.where(gt, c, best)
    ex = _exp(zt - mx[..., None], f)
    y = ex / _sum4(ex, alt)[..., None]
    tok = np.where(editable[None], best, x0[None]).astype(np.uint8)
    y = np.where(editable[None, :, None], y, f(0)).astype(f)
    return tok, y, (tok != x0[None]).sum(axis=1).astype(np.int32)


def losses(sc, edits, target, cfg):
    """sc [S], edits int [S], target scalar | None -> (out, inp, total) scalars of cfg.dtype."""
    f = cfg.dtype
    with np.errstate(all="ignore"):
        tot = f(0)
        for s in range(cfg.S):
            d = f(sc[s]) - (f(0) if target is None else f(target))
            tot = tot + (f(sc[s]) if target is None else d * d)
        q = tot / f(cfg.S)
        out = q if target is not None else -q
        inp = f(int(np.sum(edits))) / f(cfg.S)
        return out, inp, out + cfg.l * inp


def weight_grad(x0, tok, y, grad, sc, target, scale, cfg, alt=False):
    """d total / d w [L, 4] through the straight-through estimator: for every
    sample the gradient G at the hard one-hot row (the score's, times coef_s, plus the L1 subgradient) pulled through the softmax
    Jacobian (1 / tau) y_c (G_c - sum_k y_k G_k)."""
    f = cfg.dtype
    S = cfg.S
    lam, inv_tau = cfg.l / f(2 * S), f(1) / cfg.tau
    ch = np.arange(4)[None, :]
    gw = np.zeros(y.shape[1:], f)
    with np.errstate(all="ignore"):
        for s in (range(S - 1, -1, -1) if alt else range(S)):
            coef = -(f(1) / f(S)) if target is None else (f(2) * (f(sc[s]) - f(target))) / f(S)
            t = tok[s].astype(np.int64)
            edited = (t != x0)[:, None]
            pen = np.where(edited & (ch == t[:, None]), lam, np.where(edited & (ch == x0[:, None]), -lam, f(0))).astype(f)
            G = coef * (f(scale) * grad[s].astype(f)) + pen
            dot = _sum4(y[s] * G, alt)
            gw = gw + (inv_tau * y[s]) * (G - dot[:, None])
    return gw


def adamw(w, m, v, g, i, cfg):
    """torch.optim.AdamW's step number i + 1 on (w, m, v) with gradient g, in the kernel's operation order."""
    step_size, bc2_sqrt = cfg.step(i)
    with np.errstate(all="ignore"):
        w = w * cfg.decay
        m = m + cfg.w1 * (g - m)
        v = v * cfg.beta2 + (cfg.w2 * g) * g
        denom = np.sqrt(v) / bc2_sqrt + cfg.adam_eps
        return w - (step_size * m) / denom, m, v


def update(x0, editable, tok, y, grad, sc, target, w, m, v, i, scale, cfg, alt=False):
    """-> (w, m, v) after iteration i's update; frozen positions keep theirs."""
    gw = weight_grad(x0, tok, y, grad, sc, target, scale, cfg, alt)
    w2, m2, v2 = adamw(w, m, v, gw, i, cfg)
    ed = editable[:, None]
    return np.where(ed, w2, w), np.where(ed, m2, m), np.where(ed, v2, v)


# ------------------------------------------------------------------------------------------------ one launch ----
class State:
    """The buffers svdd_ledidi_step works on (ops.LedidiState), as numpy arrays."""

    def __init__(self, x0, S, score0, output0, dtype=np.float32):
        B, L = x0.shape
        self.w, self.m, self.v = (np.zeros((B, L, 4), dtype) for _ in range(3))
        self.y = np.zeros((B, S, L, 4), dtype)
        self.tok = np.repeat(x0[:, None, :], S, axis=1).copy()
        self.edits = np.zeros((B, S), np.int32)
        self.best_total, self.best_output = np.array(output0, dtype), np.array(output0, dtype)
        self.best_input = np.zeros(B, dtype)
        self.best_iter = np.full(B, -1, np.int32)
        self.x_best = self.tok.copy()
        self.score_best = np.repeat(np.asarray(score0, dtype)[:, None], S, axis=1).copy()
        self.wo, self.stopped = np.zeros(B, np.int32), np.zeros(B, np.int32)
        self.live = np.array([B], np.int32)

    FIELDS = ("w", "m", "v", "y", "tok", "edits", "best_total", "best_output", "best_input", "best_iter", "x_best", "score_best", "wo",
              "stopped", "live")


def step(st, x0, editable, cfg, xin, d0, nd, n_pad, it, grad=None, sc=None, target=None, u=None, philox=None, sample_next=True,
         trace=None, scale=1.0):
    """One svdd_ledidi_step launch on st / xin (both changed in place) for the designs d0 .. d0 + nd - 1. grad [>= nd S, L, 4] and
    sc [B, S] given: close iteration `it`; then (sample_next) draw the samples of iteration it + 1, or with grad None those of `it`.
    u [B, S, L, 4]: the replayed uniforms of the sampled iteration; else philox = (seed, row_offset). trace: three [B] arrays or
    None. -> err (1: an editable start token > 3)."""
    B, L = x0.shape
    S = cfg.S
    editable = np.ones(L, bool) if editable is None else np.asarray(editable, bool)
    assert xin.shape == (nd * S + n_pad, L, 4)
    err = 0
    for dl in range(nd):
        d = d0 + dl
        stops = False
        if grad is not None:
            if st.stopped[d]:
                continue                                            # a stopped design is left alone
            tgt = None if target is None else target[d]
            out, inp, total = losses(sc[d], st.edits[d], tgt, cfg)
            if bool(total < st.best_total[d]):
                st.best_total[d], st.best_output[d], st.best_input[d], st.best_iter[d], st.wo[d] = total, out, inp, it, 0
                st.x_best[d], st.score_best[d] = st.tok[d], sc[d]
            else:
                st.wo[d] += 1
                if st.wo[d] == cfg.patience:
                    st.stopped[d], stops = 1, True
                    st.live[0] -= 1
            if trace is not None:
                trace[0][d], trace[1][d], trace[2][d] = total, out, inp
            st.w[d], st.m[d], st.v[d] = update(x0[d], editable, st.tok[d], st.y[d], grad[dl * S:(dl + 1) * S], sc[d], tgt,
                                               st.w[d], st.m[d], st.v[d], it, scale, cfg)
        if not sample_next or stops:
            continue
        itn = it + 1 if grad is not None else it
        uu = u[d] if u is not None else uniforms(philox[0], philox[1] + d, itn, S, L)
        tok, y, edits = sample(x0[d], editable, st.w[d], uu, cfg)
        if (x0[d][editable] > 3).any():
            err = 1
        st.tok[d], st.edits[d] = tok, edits
        st.y[d][:, editable] = y[:, editable]                       # a frozen position's y is never written (and never read)
        xin[dl * S:(dl + 1) * S] = onehot(tok)
        if dl == 0:
            xin[nd * S:] = onehot(tok[0])
    return err


# ------------------------------------------------------------------------------------------------ the host loop ----
def chunks_of(B, S, chunk_rows, pow2):
    """Diffusion.ledidi's passes: [(d0, nd, n_pad)], whole designs, pow2: padded to a power-of-two number of rows."""
    cap = 1 << (chunk_rows.bit_length() - 1) if pow2 else chunk_rows
    per = max(1, cap // S)
    out = []
    for d0 in range(0, B, per):
        nd = min(per, B - d0)
        n_pass = 1 << (nd * S - 1).bit_length() if pow2 else nd * S
        out.append((d0, nd, n_pass - nd * S))
    return out


def output0(score0, target, S, f=np.float32):
    """The output loss of S copies of the start sequence by losses' own formula (a sequential sum of S equal terms, one division):
    what best_total and best_output start from, so that an iteration that edits nothing ties with the start."""
    score0 = np.asarray(score0, f)
    term = score0 if target is None else (score0 - np.asarray(target, f)) * (score0 - np.asarray(target, f))
    acc = np.zeros_like(score0)
    with np.errstate(all="ignore"):
        for _ in range(S):
            acc = acc + term
        return acc / f(S) if target is not None else -(acc / f(S))


def run(x0, score_fn, grad_fn, cfg, max_iter, editable=None, target=None, noise=None, philox=None, chunks=None, want_trace=True):
    """The whole design loop with a round trip per iteration. score_fn(tok u8 [n, L]) -> scores [n]; grad_fn(xin [n_pass, L, 4]) ->
    (gradient [n_pass, L, 4], scale). noise [max_iter + 1, B, S, L, 4] or philox = (seed, row_offset).
    -> (State, n_iter, trace [n_iter, B, 3] | None)."""
    B, L = x0.shape
    S, f = cfg.S, cfg.dtype
    chunks = [(0, B, 0)] if chunks is None else chunks
    score0 = np.asarray(score_fn(x0), f)
    tgt = None if target is None else np.broadcast_to(np.asarray(target, f).reshape(-1), (B,)).astype(f)
    st = State(x0, S, score0, output0(score0, tgt, S, f), f)
    xins = [np.zeros((nd * S + n_pad, L, 4), np.float32) for _, nd, n_pad in chunks]
    trace = np.full((max_iter + 1, 3, B), np.nan, f) if want_trace else None
    u_of = lambda it: None if noise is None else noise[it]         # noqa: E731
    for (d0, nd, n_pad), xin in zip(chunks, xins):
        step(st, x0, editable, cfg, xin, d0, nd, n_pad, 0, u=u_of(0), philox=philox)
    sc = np.zeros((B, S), f)
    for i in range(max_iter + 1):
        more = i < max_iter
        for (d0, nd, n_pad), xin in zip(chunks, xins):
            sc[d0:d0 + nd] = np.asarray(score_fn(st.tok[d0:d0 + nd].reshape(nd * S, L)), f).reshape(nd, S)
            grad, scale = grad_fn(xin)
            step(st, x0, editable, cfg, xin, d0, nd, n_pad, i, grad=np.asarray(grad), sc=sc, target=tgt,
                 u=u_of(i + 1) if more else None, philox=philox, sample_next=more,
                 trace=None if trace is None else trace[i], scale=scale)
        if st.live[0] == 0:
            break
    ran = np.where(st.stopped != 0, st.best_iter + cfg.patience + 1, max_iter + 1)
    n_iter = int(ran.max())
    return st, n_iter, (None if trace is None else trace[:n_iter].transpose(0, 2, 1).copy())
