"""Plain-torch restatements of the inference net kernels (include/svdd_hip.h: svdd_backbone_cnn_f32 / _lp, svdd_conv_tower_f32 /
_lp, svdd_candidate_windows, svdd_conv_tower_windows_f32 / _lp, svdd_gru_bidir_f32 / _lp, svdd_value_tail_f32 / _lp), one function
per operation, written from the header's description and PyTorch's documented equations. Natural-layout weights in, natural-layout
results out; nothing of svdd_amd is imported. The GRU is grad_ref.gru's `out`.

As in tests/grad_ref.py every function computes in the dtype of its inputs: on float64 tensors it is the reference; grad_ref.ref32
runs it on fp32 inputs in the kernels' stated arithmetic: one fp32 accumulator per output element, advanced in a dependent chain of
4-wide steps along K in the kernels' (32-channel chunk, tap) order (the last 128 -> 5 map of the backbone and the 128 -> n_tasks map
of the tail are per-lane chains of 1-wide steps that start at the bias). ref_lp(mode, fn, ...) is ref32 with both operands of every
matrix product rounded as the header states for the mode:
    x3 modes       hi = rn16(a), lo = rn16(a - hi), a b = hi hi + hi lo + lo hi      (f16x3, bf16x3)
    one-pass modes rn16(a) rn16(b)                                                     (f16, bf16)
with the packers' power-of-two scales (lscale / inv; exact) applied before the rounding and undone after the product, fp32
accumulation, and everything that is not a matrix product in fp32. ref32 and ref_lp exist only to size the bars of
tests/test_net_kernels_gpu.py.

Layouts (rows are channels-last): convolution weights [cout, cin, taps] as nn.Conv1d holds them, "same" zero padding.
    backbone p: dict(w_first [128, 5, 9], b_first, ws [nl x [128, 128, 9]], bs, tbs, gammas, betas [nl x [128]], dil [nl ints],
                     wf1 [128, 128], bf1 [128], w2 [5, 128], b2 [5], eps; ref_lp also reads lscale [nl + 1, 2] = {sa, 1 / (sa s_w)}).
                tbs are the fp32 time biases the kernel is handed (pack_backbone's vec rows), cast up: a float64 recomputation of the
                time embedder moves the logits by 2.5e-7, which is no error of the kernel.
    tower:      stem_w [64, 4, 15], b [1 + nl, 64], layer_ws [nl x [64, 64, 5]] (eval-mode BatchNorm folded), residual_mask bit k.
    tail:       w1 [128, 64], b1 [128], gamma / beta [64], w_eff [128, T], b_eff [T].
"""
import copy

import torch

from tests import grad_ref as R

LP_DTYPES = {"f16x3": (torch.float16, True), "bf16x3": (torch.bfloat16, True), "f16": (torch.float16, False), "bf16": (torch.bfloat16, False)}
_LP = [None]             # inside ref_lp(): (16-bit dtype, x3)


def ref_lp(mode, fn, *args, **kw):
    """ref32(fn, ...) with the operands of every matrix product rounded to the 16-bit format of `mode`."""
    _LP[0] = LP_DTYPES[mode]
    try:
        return R.ref32(fn, *args, **kw)
    finally:
        _LP[0] = None


def _rn16(v):
    return v.to(_LP[0][0]).float()


def _q(v):
    """The value a 16-bit operand image holds: hi + lo in the x3 modes, hi in the one-pass modes (ref_lp only)."""
    if _LP[0] is None:
        return v
    hi = _rn16(v)
    return hi + _rn16(v - hi) if _LP[0][1] else hi


def _mm(a, b, acc=None, sa=1.0, sw=1.0):
    """acc + a @ b through grad_ref._mm (ref32: one accumulator, 4-wide steps). ref_lp: a sa and b sw rounded to 16 bits, the
    products hi hi + hi lo + lo hi (x3) or hi hi on the same accumulator, the scales undone on the finished sum."""
    if _LP[0] is None:
        return R._mm(a, b, acc)
    a, b = a * sa, b * sw
    ahi, bhi = _rn16(a), _rn16(b)
    y = None if acc is None else acc * (sa * sw)
    if _LP[0][1]:
        alo, blo = _rn16(a - ahi), _rn16(b - bhi)
        y = R._mm(torch.cat([ahi, ahi, alo], dim=-1), torch.cat([bhi, blo, bhi], dim=0), y)
    else:
        y = R._mm(ahi, bhi, y)
    return y * (1.0 / (sa * sw))


def _chain1(a, b, acc):
    """acc + a @ b; ref32: a chain of 1-wide steps that starts at acc (the per-lane loops)."""
    if not R._FAST[0]:
        return a @ b + acc
    y = acc
    for k in range(a.shape[-1]):
        y = y + a[..., k:k + 1] * b[k]
    return y


def conv_chunked(x, w, dilation=1, sa=1.0, sw=1.0):
    """y[n, l, co] = sum_c sum_t sum_{ci in chunk c} x[n, l + (t - T/2) dilation, ci] w[co, ci, t], summed in the order
    (32-channel chunk, tap) the kernels' weight tiles arrive in; x [n, L, cin], w [cout, cin, T]. No bias."""
    T, cin = w.shape[2], w.shape[1]
    y = None
    for c0 in range(0, cin, 32):
        for t in range(T):
            y = _mm(R._shift(x[:, :, c0:c0 + 32], (t - T // 2) * dilation), w[:, c0:c0 + 32, t].t(), y, sa, sw)
    return y


# --------------------------------------------------------------------------------------------------------------- backbone
def onehot5(tokens):
    return torch.eye(5)[tokens.long()]


def backbone(onehot, p):
    """onehot [n, L, 5] (of tokens 0..4, MASK = 4 its own channel) -> raw logits [n, L, 5]:
    f = relu(conv9(onehot) + b_first); nl x [f = relu(conv9_dil(LayerNorm(f + tb_i) gamma_i + beta_i) + b_i) + f];
    logits = W2 relu(W_f1 f + b_f1) + b2."""
    ls = p.get("lscale") if _LP[0] is not None else None
    f = torch.relu(R.conv_same(onehot, p["w_first"], p["b_first"], bias_first=True))      # a table lookup per tap: exact products
    for i, d in enumerate(p["dil"]):
        xh, _ = R._ln_stats(f + p["tbs"][i], p["eps"])
        hn = xh * p["gammas"][i] + p["betas"][i]
        sa, sw = (1.0, 1.0) if ls is None else (float(ls[i, 0]), 1.0 / (float(ls[i, 0]) * float(ls[i, 1])))
        f = torch.relu(conv_chunked(hn, p["ws"][i], d, sa, sw) + p["bs"][i]) + f
    sa, sw = (1.0, 1.0) if ls is None else (float(ls[-1, 0]), 1.0 / (float(ls[-1, 0]) * float(ls[-1, 1])))
    h1 = torch.relu(conv_chunked(f, p["wf1"][:, :, None], 1, sa, sw) + p["bf1"])
    return _chain1(h1, p["w2"].t(), p["b2"].expand(h1.shape[0], h1.shape[1], 5))


def backbone_params(cnn, tbs, lscale=None):
    """The natural-layout weights of a CNNModel-shaped module (fp32, CPU) in the form backbone() takes. tbs: the fp32 time biases
    the kernel is handed, [nl] tensors of [128] (or [nl, 128])."""
    c = lambda t: t.detach().float().cpu()   # noqa: E731
    p = dict(w_first=c(cnn.linear.weight), b_first=c(cnn.linear.bias), ws=[c(m.weight) for m in cnn.convs], bs=[c(m.bias) for m in cnn.convs],
             tbs=[c(t).reshape(-1) for t in tbs], gammas=[c(m.weight) for m in cnn.norms], betas=[c(m.bias) for m in cnn.norms],
             dil=[int(m.dilation[0]) for m in cnn.convs], wf1=c(cnn.final_conv[0].weight)[:, :, 0], bf1=c(cnn.final_conv[0].bias),
             w2=c(cnn.final_conv[2].weight)[:, :, 0], b2=c(cnn.final_conv[2].bias), eps=float(cnn.norms[0].eps))
    if lscale is not None:
        p["lscale"] = c(lscale)
    return p


# ------------------------------------------------------------------------------------------------------------------ tower
def onehot4(tokens):
    """transform_samples: tokens 0..3 -> one-hot, MASK (4) -> a zero row."""
    return torch.eye(5)[tokens.long()][..., :4].contiguous()


def tower(onehot, stem_w, b, layer_ws, residual_mask, inv=None):
    """a0 = relu(conv15(onehot) + b[0]); a_{k+1} = relu(conv5(a_k) + b[1 + k] [+ a_k if bit k of residual_mask]); onehot [n, L, 4]
    -> [n, L, 64]. ref_lp: inv [1 + nl] = 1 / s_w of each stage; every stage's output is kept as its 16-bit image (hi + lo, or hi)."""
    sw = lambda k: 1.0 if inv is None or _LP[0] is None else 1.0 / float(inv[k])   # noqa: E731
    a = _q(torch.relu(conv_chunked(onehot, stem_w, 1, 1.0, sw(0)) + b[0]))      # k = 4 tap + channel: one 4-wide step per tap
    for k, w in enumerate(layer_ws):
        y = conv_chunked(a, w, 1, 1.0, sw(1 + k)) + b[1 + k]
        a = _q(torch.relu(y + a if (residual_mask >> k) & 1 else y))
    return a


def tower_inputs(nlayers, seed):
    """Weights of a tower at the default initialisation's scale (uniform +- 1 / sqrt(fan_in)), each layer drawn on its own."""
    g = R._gen(11, nlayers, seed)
    u = lambda shape, fan: (torch.rand(shape, generator=g) * 2.0 - 1.0) / fan ** 0.5   # noqa: E731
    stem_w = u((64, 4, 15), 60)
    ws = [u((64, 64, 5), 320) for _ in range(nlayers)]
    b = torch.cat([u((1, 64), 60), u((nlayers, 64), 320)])
    return stem_w, b, ws


def windows(cand, x, margin):
    """cand [B, M, L], x [B, L] integer tokens -> (win [B M, 2] int32, flags [B M] int32): the 16-aligned row window (w0, w1) that
    covers the positions where a candidate differs from its parent +- margin, clipped to [0, L rounded up to 16); (0, 0) for an exact
    copy; flags = (w1 - w0) / 16, the row tiles of the window (0: a copy)."""
    B, M, L = cand.shape
    diff = (cand != x[:, None, :]).reshape(B * M, L)
    win = torch.zeros(B * M, 2, dtype=torch.int32)
    for c in range(B * M):
        pos = diff[c].nonzero().flatten()
        if len(pos):
            lo, hi = int(pos.min()), int(pos.max())
            win[c, 0] = max(0, lo - margin) // 16 * 16
            win[c, 1] = min((L + 15) // 16 * 16, (hi + margin + 1 + 15) // 16 * 16)
    return win, (win[:, 1] - win[:, 0]) // 16


# ------------------------------------------------------------------------------------------------------------------- tail
# step sidx of the fp32 tail's MFMA chain multiplies the channels 16 (sidx / 4) + 4 g + sidx % 4, g = 0 .. 3
_TAIL_K = [16 * (s // 4) + 4 * g + s % 4 for s in range(16) for g in range(4)]


def _tail_mean(z, w_eff, L):
    """mean_l sum_c z[n, l, c] w_eff[c, t]. ref32: as the kernels sum it — lane (j, g) of a sequence's wave adds z w_eff of rows
    16 tile + 4 g + rho and columns 16 ct + j to ONE accumulator in (tile, rho, ct) order (32 L / 16 one-wide steps from zero), the 64
    lanes are summed by an xor butterfly (offsets 32 .. 1), and the total is divided by L."""
    if not R._FAST[0]:
        return (z @ w_eff).mean(dim=1)
    n, T, nt = z.shape[0], w_eff.shape[1], (L + 15) // 16
    zz = torch.zeros(n, 16 * nt, 128, dtype=z.dtype)
    zz[:, :L] = z
    zz = zz.view(n, nt, 4, 4, 8, 16)                       # [n][tile][g][rho][ct][j]
    we = w_eff.reshape(8, 16, T)
    part = torch.zeros(n, 4, 16, T, dtype=z.dtype)
    for tile in range(nt):
        for rho in range(4):
            for ct in range(8):
                part = part + zz[:, tile, :, rho, ct, :, None] * we[ct]
    tot = part.reshape(n, 64, T)                           # lane = 16 g + j
    while tot.shape[1] > 1:
        h = tot.shape[1] // 2
        tot = tot[:, :h] + tot[:, h:]
    return tot[:, 0] / float(L)


def tail(h_fwd, h_bwd, w1, b1, gamma, beta, w_eff, b_eff, eps=1e-5, inv=None):
    """out[n, t] = b_eff[t] + mean_l sum_c w_eff[c, t] relu(b1[c] + sum_k W1[c, k] (LayerNorm(h_fwd + h_bwd) gamma + beta)[n, l, k]),
    with the LayerNorm affine folded into the linear map as the kernel is handed it: W1' = W1 diag(gamma), b1' = b1 + W1 beta.
    ref32: the 64 -> 128 chain starts at b1' and takes the channels in the kernel's k order; ref_lp: it starts at zero, takes the two
    32-channel chunks in turn (hi hi, hi lo, lo hi each), and b1' is added to the descaled sum."""
    n, L, _ = h_fwd.shape
    xh, _ = R._ln_stats(h_fwd + h_bwd, eps)
    w1f, b1f = w1 * gamma[None, :], b1 + w1 @ beta
    if _LP[0] is None:
        z = torch.relu(R._mm(xh[..., _TAIL_K], w1f.t()[_TAIL_K], b1f.expand(n, L, w1.shape[0])))
    else:
        sw, y = 1.0 if inv is None else 1.0 / float(inv), None
        for c0 in (0, 32):
            y = _mm(xh[..., c0:c0 + 32], w1f.t()[c0:c0 + 32], y, 1.0, sw)
        z = torch.relu(y + b1f)
    return _tail_mean(z, w_eff, L) + b_eff


def tail_inputs(n, L, T, net_scale=False):
    """h [2, n, L, 64] and the tail's natural weights. Default: the scales of test_value_tail_vs_torch (scores of order 1).
    net_scale: dense1, dense2 and the head drawn at the default initialisation's scale (uniform +- 1 / sqrt(fan_in)) and collapsed
    as the net collapses them, so that the scores have the magnitude (< 0.1) the absolute tolerances of the split-precision modes
    were set at."""
    g = R._gen(12, n, L, T, int(net_scale))
    h = torch.randn(2, n, L, 64, generator=g)
    h[:, 1::2] *= 3.0                                    # neighbouring sequences at different scales
    gam, bet = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.2
    if not net_scale:
        w1, b1 = torch.randn(128, 64, generator=g) * 0.2, torch.randn(128, generator=g) * 0.1
        return h, w1, b1, gam, bet, torch.randn(128, T, generator=g) * 0.2, torch.randn(T, generator=g)
    u = lambda shape, fan: (torch.rand(shape, generator=g, dtype=torch.float64) * 2.0 - 1.0) / fan ** 0.5   # noqa: E731
    w1, b1, w2, b2, wh, bh = u((128, 64), 64), u((128,), 64), u((64, 128), 128), u((64,), 128), u((T, 64), 64), u((T,), 64)
    return h, w1.float(), b1.float(), gam, bet, (wh @ w2).t().float().contiguous(), (wh @ b2 + bh).float()


def gru_out(x, weights):
    return R.gru(x, weights)["out"]


def gru_out_lp(x, weights, inv=None):
    """grad_ref.gru's out with the six matrix products of a step on 16-bit operands (ref_lp): x and h as their 16-bit images, the
    weights scaled by s_w = 1 / inv[direction]."""
    n, L, H = x.shape
    out = torch.zeros(2, n, L, H, dtype=x.dtype)
    for d in range(2):
        sw = 1.0 if inv is None or _LP[0] is None else 1.0 / float(inv[d])
        w_ih, w_hh, b_ih, b_hh = (weights[k][d] for k in ("w_ih", "w_hh", "b_ih", "b_hh"))
        bias = b_ih.clone()
        bias[:2 * H] += b_hh[:2 * H]
        gi = _mm(x, w_ih.t(), bias.expand(n, L, 3 * H), 1.0, sw)
        h = torch.zeros(n, H, dtype=x.dtype)
        for t in (range(L) if d == 0 else range(L - 1, -1, -1)):
            r = R._sigmoid(_mm(h, w_hh[:H].t(), gi[:, t, :H], 1.0, sw))
            z = R._sigmoid(_mm(h, w_hh[H:2 * H].t(), gi[:, t, H:2 * H], 1.0, sw))
            lin = _mm(h, w_hh[2 * H:].t(), b_hh[2 * H:].expand(n, H), 1.0, sw)
            c = R._tanh(gi[:, t, 2 * H:] + r * lin)
            h = (1.0 - z) * c + z * h
            out[d, :, t] = h
    return out


def value_net(onehot, p):
    """The whole ConvGRU value net: tower -> GRU -> tail; onehot [n, L, 4] -> scores [n, T]."""
    a = tower(onehot, p["stem_w"], p["tw_b"], p["ws"], p["residual_mask"])
    h = R.gru(a, p["gru"])["out"]
    return tail(h[0], h[1], p["w1"], p["b1"], p["gamma"], p["beta"], p["w_eff"], p["b_eff"], p["eps"])


def value_params(embedding, head):
    """The natural-layout weights of a ConvGRUTrunk + ConvHead pair as float64 CPU tensors in the form value_net takes: eval-mode
    BatchNorm folded into the preceding convolution, dense2 and the head collapsed into one 128 -> T map (both in float64)."""
    c = lambda t: t.detach().double().cpu()   # noqa: E731
    blocks = embedding.conv_tower.blocks
    ws, bs, mask = [], [c(blocks[0].conv.bias)], 0
    for k, blk in enumerate(blocks[1:]):
        w, b, bn = c(blk.conv.weight), c(blk.conv.bias), blk.norm.layer
        if isinstance(bn, torch.nn.BatchNorm1d):
            s = c(bn.weight) / torch.sqrt(c(bn.running_var) + bn.eps)
            w, b = w * s[:, None, None], (b - c(bn.running_mean)) * s + c(bn.bias)
        ws.append(w)
        bs.append(b)
        mask |= int(bool(blk.residual)) << k
    gt = embedding.gru_tower
    d1, d2, hw = gt.ffn.dense1, gt.ffn.dense2, head.channel_transform.conv.layer
    wh = c(hw.weight)[:, :, 0]
    return dict(stem_w=c(blocks[0].conv.weight), tw_b=torch.stack(bs), ws=ws, residual_mask=mask, gru=R.to(torch.float64, R.gru_weights_of(gt.gru)),
                w1=c(d1.linear.weight), b1=c(d1.linear.bias), gamma=c(d1.norm.layer.weight), beta=c(d1.norm.layer.bias),
                w_eff=(wh @ c(d2.linear.weight)).t().contiguous(), b_eff=wh @ c(d2.linear.bias) + c(hw.bias), eps=float(d1.norm.layer.eps))


# ------------------------------------------------------------------------------------------------------- distinct layers
def equal_pairs(module):
    """[(name_a, name_b)] of the convolutions of `module` whose weight tensors hold the same values."""
    convs = [(n, m) for n, m in module.named_modules() if isinstance(m, torch.nn.Conv1d)]
    return [(na, nb) for i, (na, a) in enumerate(convs) for nb, b in convs[i + 1:]
            if a.weight.shape == b.weight.shape and torch.equal(a.weight, b.weight)]


def distinct_layers(module, seed=0):
    """Re-draws every convolution's weight and bias with its own reset_parameters() (the default initialisation's scale) from a
    seeded generator, on the CPU so that the values do not depend on the module's device, and gives every LayerNorm / BatchNorm a
    non-trivial affine map (and running statistics). CNNModel deep-copies each of its five base convolutions num_cnn_stacks times:
    at random init its 20 layers are 5 groups of 4 equal ones, and a kernel that takes a layer's tiles for its neighbour's inside a
    group computes the right answer. Asserts that no two convolutions of the module are left with equal weights. -> module."""
    with torch.random.fork_rng(devices=[]), torch.no_grad():
        torch.manual_seed(1000003 * seed + 17)
        for m in module.modules():
            if isinstance(m, torch.nn.Conv1d):
                fresh = copy.deepcopy(m).cpu()
                fresh.reset_parameters()
                m.weight.copy_(fresh.weight)
                if m.bias is not None:
                    m.bias.copy_(fresh.bias)
            elif isinstance(m, (torch.nn.LayerNorm, torch.nn.BatchNorm1d)) and m.weight is not None:
                m.weight.copy_(torch.rand(m.weight.shape) + 0.5)
                m.bias.copy_(torch.rand(m.bias.shape) * 0.6 - 0.3)
                if isinstance(m, torch.nn.BatchNorm1d):
                    m.running_mean.copy_(torch.randn(m.num_features) * 0.1)
                    m.running_var.copy_(torch.rand(m.num_features) + 0.5)
    left = equal_pairs(module)
    assert not left, f"layers with equal weights: {left[:4]}"
    return module


# -------------------------------------------------------------------------------------------- inputs shared by CPU and GPU
MAX_DISTINCT = 32


def replicated(n, seed, dmax=MAX_DISTINCT):
    """-> (d, idx [n]): a batch of n rows built from d = min(n, dmax) distinct ones in shuffled order; idx[:d] is a permutation, so
    every distinct row occurs, and the copies of a row get different neighbours."""
    g = R._gen(13, n, seed)
    d = min(n, dmax)
    idx = torch.cat([torch.randperm(d, generator=g), torch.randint(0, d, (n - d,), generator=g)])
    return d, idx


def tokens(d, L, seed):
    """d distinct token rows, 40 % MASK; of two or more, row 0 is all MASK and row 1 has no MASK."""
    g = R._gen(14, d, L, seed)
    x = torch.randint(0, 4, (d, L), generator=g)
    x[torch.rand(d, L, generator=g) < 0.4] = 4
    if d > 1:
        x[0] = 4
        x[1] = torch.randint(0, 4, (L,), generator=g)
    return x.to(torch.uint8)
