"""Plain-torch restatements of the backbone's one-launch input gradient (include/svdd_hip.h: svdd_backbone_cnn_save_f32 /
svdd_backbone_cnn_grad_f32), of the layer-wise dilated convolution (svdd_conv1d_cl_f32, both directions) and of the fused epilogue
(svdd_conv1d_cl_f32's and svdd_epilogue_ln_f32), written from the header's description; and the index map between the lane-private
layout the save / grad pair exchanges and natural [row][channel] tensors. Nothing of svdd_amd is imported.

As in tests/grad_ref.py every function computes in the dtype of its inputs: on float64 tensors it is the reference (grad_ref.ref64);
grad_ref.ref32 runs it on fp32 inputs in the kernels' stated arithmetic, which exists only to size the bars of
tests/test_backbone_grad_kernel_gpu.py and tests/test_conv_epilogue_kernels_gpu.py. For a matrix product that is ONE fp32
accumulator per output element, starting at zero, advanced in a dependent chain along K in (32-channel chunk, tap) order — the
order the weight tiles arrive in — with the step width and the channels of a step read off the kernel:
    "32x32x2"  conv1d_cl_kernel / conv1d_cl_static_kernel (v_mfma_f32_32x32x2_f32): 16 steps per tile, step m multiplies the TWO
               channels m and 16 + m of the chunk (lane half h reads the 16 consecutive channels at 16 h); taps ascending; the
               bias joins the finished sum in the epilogue.
    "16x16x4"  backbone_grad_kernel (v_mfma_f32_16x16x4_f32): 8 steps per tile, step m multiplies the FOUR channels m, 8 + m,
               16 + m, 24 + m (lane group g reads the 8 consecutive channels at 8 g); the packed taps ascending, which is the
               natural taps descending (the pack is flipped).
A tap all of whose rows are padding is skipped by the kernels and here. G1 = dlogits W2 is a per-lane chain of five 1-wide steps
from zero, the first convolution's transpose a per-thread chain of 4-wide steps over (tap, 128 channels) from zero
(grad_ref.conv_same_t). Everything else is element-wise fp32; LayerNorm statistics are two-pass (mean, then the biased variance of
the centred values).

Layouts (rows are channels-last): convolution weights [cout, cin, taps] as nn.Conv1d holds them, "same" zero padding.
    backbone weights: dict(w_first [128, 5, 9], ws [nl x [128, 128, 9]], gammas [nl x [128]], wf1 [128, 128], w2 [5, 128], ...) as
    weights_of() returns them."""
import torch

from tests import grad_ref as R

MFMA = {"32x32x2": (2, [m + 16 * h for m in range(16) for h in range(2)]),
        "16x16x4": (4, [m + 8 * g for m in range(8) for g in range(4)])}


def _chain(a, b, acc=None, width=4, order=None):
    """acc + a @ b (a [..., K], b [K, N]). ref32: one accumulator, a dependent chain of `width`-wide steps along K taken in `order`."""
    if not R._FAST[0]:
        y = a @ b
        return y if acc is None else y + acc
    if order is not None:
        a, b = a[..., order], b[order]
    y = acc
    for k in range(0, a.shape[-1], width):
        step = a[..., k:k + width] @ b[k:k + width]
        y = step if y is None else y + step
    return y


# ------------------------------------------------------------------------------------------------------------ convolutions
def conv_dilated(x, w, dilation=1, mfma="32x32x2"):
    """y[n, l, co] = sum_t sum_ci x[n, l + (t - T/2) dilation, ci] w[co, ci, t]; x [n, L, cin], w [cout, cin, T], cin % 32 == 0.
    No bias. (net_ref.conv_chunked is the same sum in 4-wide steps of consecutive channels, the forward backbone's; the kernels
    restated here step otherwise, see the module docstring.)"""
    T, cin, L = w.shape[2], w.shape[1], x.shape[1]
    width, order = MFMA[mfma]
    y = None
    for c0 in range(0, cin, 32):
        for t in range(T):
            s = (t - T // 2) * dilation
            if abs(s) < L:                                      # else every row of the tap is padding
                y = _chain(R._shift(x[:, :, c0:c0 + 32], s), w[:, c0:c0 + 32, t].t(), y, width, order)
    return y


def conv_dilated_t(g, w, dilation=1, mfma="32x32x2"):
    """The transpose of conv_dilated in x: dx[n, p, ci] = sum_t sum_co w[co, ci, t] g[n, p - (t - T/2) dilation, co]; g [n, L, cout]
    -> [n, L, cin]. It is conv_dilated on the flipped taps with the channel axes swapped, which is how the kernels compute it."""
    return conv_dilated(g, w.flip(2).transpose(0, 1), dilation, mfma)


# ---------------------------------------------------------------------------------------------------------------- epilogue
def epilogue(y, bias, f_prev, tb, gamma, beta, act, eps=1e-5):
    """rows y [..., C] -> (f_out, hn): t = y + bias ; f_out = relu(t) + f_prev (act 0) | relu(t + f_prev) (act 1) | t + f_prev (act 2)
    ; hn = LayerNorm(f_out + tb) gamma + beta (gamma None: hn None). bias, tb, gamma, beta [C] — one value per CHANNEL, the same
    for every row, in svdd_epilogue_ln_f32 and in svdd_conv1d_cl_f32 alike; f_prev like y. bias / f_prev / tb None: zero."""
    t = y if bias is None else y + bias
    p = torch.zeros_like(y) if f_prev is None else f_prev
    f = torch.relu(t) + p if act == 0 else torch.relu(t + p) if act == 1 else t + p
    if gamma is None:
        return f, None
    xh, _ = R._ln_stats(f if tb is None else f + tb, eps)
    return f, xh * gamma + beta


# ------------------------------------------------------------------------------------------------- the backbone's gradient
def backbone_grad(dlogits, masks, xhat, rstd, weights, dilations):
    """d loss / d onehot(x) [n, L, 5] from dlogits [n, L, 5] = d loss / d logits, given the forward's state in natural layout:
    masks bool [n, nl + 2, L, 128] (ReLU decisions of the first layer, of every conv layer, of final_conv's first 1x1), xhat
    [n, nl, L, 128] (the LayerNorm'd value before the affine map), rstd [n, nl, L]. With the decisions given this is LINEAR in dlogits."""
    nl = len(dilations)
    on = lambda k, v: torch.where(masks[:, k], v, torch.zeros_like(v))   # noqa: E731
    g1 = on(nl + 1, _chain(dlogits, weights["w2"], None, 1))                                   # (dlogits W2) relu'(final 1x1)
    G = conv_dilated_t(g1, weights["wf1"][:, :, None], 1, "16x16x4")                          # the transposed 1x1
    for i in range(nl - 1, -1, -1):
        dhn = conv_dilated_t(on(1 + i, G), weights["ws"][i], dilations[i], "16x16x4")
        G = G + R._ln_bwd(dhn * weights["gammas"][i], xhat[:, i], rstd[:, i, :, None])
    return R.conv_same_t(on(0, G), weights["w_first"])


def forward_state(onehot, weights, tbs):
    """The backbone forwards on onehot [n, L, 5] with the time biases tbs [nl x [128]], keeping what the gradient needs ->
    dict(logits [n, L, 5], masks bool [n, nl + 2, L, 128], xhat [n, nl, L, 128], rstd [n, nl, L])."""
    pre = R.conv_same(onehot, weights["w_first"], weights["b_first"], bias_first=True)
    masks, xs, rs = [pre > 0], [], []
    f = torch.relu(pre)
    for i, d in enumerate(weights["dil"]):
        xh, r1 = R._ln_stats(f + tbs[i], weights["eps"])
        pre = conv_dilated(xh * weights["gammas"][i] + weights["betas"][i], weights["ws"][i], d) + weights["bs"][i]
        masks.append(pre > 0)
        xs.append(xh)
        rs.append(r1[..., 0])
        f = torch.relu(pre) + f
    pre = f @ weights["wf1"].t() + weights["bf1"]
    masks.append(pre > 0)
    logits = torch.relu(pre) @ weights["w2"].t() + weights["b2"]
    return dict(logits=logits, masks=torch.stack(masks, dim=1), xhat=torch.stack(xs, dim=1), rstd=torch.stack(rs, dim=1))


def weights_of(cnn, layers=None):
    """The natural-layout weights of a CNNModel-shaped module, in its own dtype, on the CPU. layers: the conv layers to keep, in
    order (default all) — any subsequence of the residual layers is a backbone of that many layers."""
    c = lambda t: t.detach().cpu()   # noqa: E731
    ks = list(range(len(cnn.convs))) if layers is None else list(layers)
    return dict(w_first=c(cnn.linear.weight), b_first=c(cnn.linear.bias), ws=[c(cnn.convs[k].weight) for k in ks],
                bs=[c(cnn.convs[k].bias) for k in ks], gammas=[c(cnn.norms[k].weight) for k in ks], betas=[c(cnn.norms[k].bias) for k in ks],
                dil=[int(cnn.convs[k].dilation[0]) for k in ks], wf1=c(cnn.final_conv[0].weight)[:, :, 0], bf1=c(cnn.final_conv[0].bias),
                w2=c(cnn.final_conv[2].weight)[:, :, 0], b2=c(cnn.final_conv[2].bias), eps=float(cnn.norms[0].eps))


# ------------------------------------------------------------------------------------------------- the lane-private layout
TILE_ROWS, SLOTS, THREADS = 208, 56, 512


def save_layout():
    """The lane-private layout of svdd_backbone_cnn_save_f32's xhat [56 slots][512 threads] as include/svdd_hip.h states it: thread
    tid = 64 w + 16 g + j (w = wave, cg = w & 3, rh = w >> 2) keeps in slot (2 r + ct) 4 + e the value of row 16 (rh + 2 r) + 4 g + e,
    channel 32 cg + j + 16 ct; a slot whose row is >= 208 is never written. Bit s of the thread's mask word is slot s's decision.
    -> (row, col) int64 [56, 512], valid bool [56, 512]."""
    tid, slot = torch.arange(THREADS)[None, :], torch.arange(SLOTS)[:, None]
    w, lane = tid >> 6, tid & 63
    cg, rh, j, g = w & 3, w >> 2, lane & 15, lane >> 4
    r, ct, e = slot // 8, (slot // 4) % 2, slot % 4
    row, col = 16 * (rh + 2 * r) + 4 * g + e, 32 * cg + j + 16 * ct + 0 * slot
    return row, col, row < TILE_ROWS


def decode_xhat(raw, L):
    """xhat [n, nl, 56, 512] as saved -> [n, nl, L, 128]."""
    row, col, valid = save_layout()
    img = torch.zeros(*raw.shape[:2], TILE_ROWS, 128, dtype=raw.dtype)
    img[:, :, row[valid], col[valid]] = raw[:, :, valid]
    return img[:, :, :L].contiguous()


def decode_masks(words, L):
    """mask [n, nl + 2, 512] (the u64 words as int64) as saved -> bool [n, nl + 2, L, 128]."""
    row, col, valid = save_layout()
    img = torch.zeros(*words.shape[:2], TILE_ROWS, 128, dtype=torch.bool)
    for s in range(SLOTS):
        ok = valid[s]
        img[:, :, row[s][ok], col[s][ok]] = ((words[:, :, ok] >> s) & 1).bool()
    return img[:, :, :L].contiguous()
