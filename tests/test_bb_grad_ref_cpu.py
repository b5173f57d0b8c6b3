"""The float64 references of tests/bb_grad_ref.py proved against torch (autograd through a float64 CNNModel with 20 distinct layers,
torch.nn.functional's conv1d / layer_norm) to 1e-10 of the scale, and the index map of the lane-private layout shown to be a
bijection onto the 208 x 128 tile. No GPU."""
import copy

import pytest
import torch
import torch.nn.functional as F

from tests import bb_grad_ref as B
from tests import grad_ref as R
from tests import net_ref as N

TOL = 1e-10


def _close(got, want, what):
    scale = max(float(want.abs().max()), 1e-300)
    err = float((got - want).abs().max())
    assert err <= TOL * scale, (what, err, scale)


@pytest.mark.parametrize("L", [105, 200])
def test_backbone_grad_vs_autograd_through_a_float64_cnn_model(L):
    """backbone_grad on the masks / xhat / rstd of a float64 forward (forward_state, itself held to the module's logits) against
    torch autograd through CNNModel.forward2 in float64, n = 2."""
    from svdd_amd import backbone, config
    torch.manual_seed(3)
    cnn = N.distinct_layers(backbone.CNNModel(config.dna_config().model, alphabet_size=5).eval(), 3).double()
    n = 2
    g = R._gen(21, L)
    tok = N.tokens(n, L, 1)
    xi = N.onehot5(tok).double().requires_grad_(True)
    dl = torch.randn(n, L, 5, generator=g, dtype=torch.float64)
    t0 = torch.zeros(n, dtype=torch.float64)
    out = cnn.forward2(xi, t0)
    (want,) = torch.autograd.grad(out, xi, dl)
    w = B.weights_of(cnn)
    with torch.no_grad():
        tbs = [t[0, :, 0] for t in cnn._time_biases(t0[:1])]
        st = B.forward_state(xi.detach(), w, tbs)
    _close(st["logits"], out.detach(), "forward_state logits")
    _close(B.backbone_grad(dl, st["masks"], st["xhat"], st["rstd"], w, w["dil"]), want, "backbone_grad")
    # ... and on a subsequence of the layers (what the GPU file does for other layer counts)
    sub = [8, 16]
    small = copy.deepcopy(cnn)
    for name in ("convs", "norms", "time_layers"):
        setattr(small, name, torch.nn.ModuleList([getattr(cnn, name)[k] for k in sub]))
    small.num_layers = len(sub)
    out = small.forward2(xi, t0)
    (want,) = torch.autograd.grad(out, xi, dl)
    w2 = B.weights_of(cnn, sub)
    with torch.no_grad():
        st = B.forward_state(xi.detach(), w2, [tbs[k] for k in sub])
    _close(st["logits"], out.detach(), "forward_state logits, 2 layers")
    _close(B.backbone_grad(dl, st["masks"], st["xhat"], st["rstd"], w2, w2["dil"]), want, "backbone_grad, 2 layers")


@pytest.mark.parametrize("n,L,cin,cout,T,dil", [(2, 37, 64, 128, 9, 16), (3, 50, 128, 128, 9, 64), (5, 1, 64, 64, 5, 1), (2, 113, 128, 64, 3, 7),
                                                (1, 224, 64, 64, 1, 1), (2, 200, 128, 128, 9, 4)])
def test_conv_dilated_and_its_transpose_vs_conv1d_autograd(n, L, cin, cout, T, dil):
    gen = R._gen(22, n, L, cin, cout, T, dil)
    x = torch.randn(n, L, cin, generator=gen, dtype=torch.float64).requires_grad_(True)
    w = torch.randn(cout, cin, T, generator=gen, dtype=torch.float64)
    g = torch.randn(n, L, cout, generator=gen, dtype=torch.float64)
    want = F.conv1d(x.transpose(1, 2), w, padding=(T // 2) * dil, dilation=dil).transpose(1, 2)
    (dx,) = torch.autograd.grad(want, x, g)
    for mfma in B.MFMA:
        _close(B.conv_dilated(x.detach(), w, dil, mfma), want.detach(), "conv_dilated")
        _close(B.conv_dilated_t(g, w, dil, mfma), dx, "conv_dilated_t")


def test_chained_fp32_restatement_visits_every_channel_once():
    """The step tables are permutations of a 32-channel chunk, and ref32 of conv_dilated is the float64 value to fp32 round-off."""
    for width, order in B.MFMA.values():
        assert sorted(order) == list(range(32)) and 32 % width == 0
    gen = R._gen(23)
    x, w = torch.randn(2, 50, 64, generator=gen), torch.randn(64, 64, 5, generator=gen) * 0.1
    for mfma in B.MFMA:
        r64, r32 = R.ref64(B.conv_dilated, x, w, 4, mfma), R.ref32(B.conv_dilated, x, w, 4, mfma)
        assert r32.dtype == torch.float32 and float((r32.double() - r64).abs().max()) <= 64 * R.FP32_EPS * float(r64.abs().max())


@pytest.mark.parametrize("C", [64, 128, 256])
@pytest.mark.parametrize("act", [0, 1, 2])
def test_epilogue_vs_torch_functional(C, act):
    gen = R._gen(24, C, act)
    y, fp = (torch.randn(7, C, generator=gen, dtype=torch.float64) for _ in range(2))
    y[3] = 100.0 + y[3]                                               # a row with a large common offset
    b, tb, gm, bt = (torch.randn(C, generator=gen, dtype=torch.float64) for _ in range(4))
    for bias, f_prev, tbv in ((b, fp, tb), (None, fp, None), (b, None, tb), (None, None, None)):
        t = y + (0 if bias is None else bias)
        p = 0 if f_prev is None else f_prev
        want = {0: torch.relu(t) + p, 1: torch.relu(t + p), 2: t + p}[act]
        f, hn = B.epilogue(y, bias, f_prev, tbv, gm, bt, act, 1e-5)
        _close(f, want, "f_out")
        _close(hn, F.layer_norm(want + (0 if tbv is None else tbv), (C,), gm, bt, 1e-5), "hn")
        assert B.epilogue(y, bias, f_prev, tbv, None, None, act)[1] is None
    const = torch.full((1, C), 3.0, dtype=torch.float64)              # variance 0: hn = beta through the eps path
    _close(B.epilogue(const, None, None, None, gm, bt, 2)[1], bt.expand(1, C), "constant row")


def test_lane_private_layout_is_a_bijection_and_the_decoders_invert_it():
    row, col, valid = B.save_layout()
    assert int(valid.sum()) == 208 * 128
    seen = torch.zeros(208, 128, dtype=torch.int32)
    seen.index_put_((row[valid], col[valid]), torch.ones(int(valid.sum()), dtype=torch.int32), accumulate=True)
    assert bool((seen == 1).all())
    gen = R._gen(25)
    img = torch.randn(2, 3, 208, 128, generator=gen)
    raw = torch.zeros(2, 3, 56, 512)
    raw[:, :, valid] = img[:, :, row[valid], col[valid]]
    assert torch.equal(B.decode_xhat(raw, 208), img) and torch.equal(B.decode_xhat(raw, 105), img[:, :, :105])
    bits = torch.rand(2, 3, 208, 128, generator=gen) < 0.5
    words = torch.zeros(2, 3, 512, dtype=torch.int64)
    for s in range(56):
        ok = valid[s]
        words[:, :, ok] |= bits[:, :, row[s][ok], col[s][ok]].long() << s
    assert torch.equal(B.decode_masks(words, 208), bits) and torch.equal(B.decode_masks(words, 200), bits[:, :, :200])
