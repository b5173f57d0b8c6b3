"""CPU: the float64 restatements of tests/net_ref.py equal the float64 PyTorch modules given the same operands, distinct_layers
leaves no two layers equal (and a random-init backbone does have equal groups, which is why it exists), and ref32 / ref_lp run and
give errors of the order the bars of tests/test_net_kernels_gpu.py are meant to have."""
import copy

import pytest
import torch

from tests import grad_ref as R
from tests import net_ref as N


def _cnn(seed=0):
    from svdd_amd import backbone, config
    torch.manual_seed(5)
    cnn = backbone.CNNModel(config.dna_config().model, alphabet_size=5).eval()
    return N.distinct_layers(cnn, seed)


def _tbs(cnn):
    with torch.no_grad():
        return [t.reshape(-1) for t in cnn._time_biases(torch.zeros(1))]


@pytest.mark.parametrize("L", [50, 9])
def test_backbone_restatement_equals_the_float64_module(L):
    cnn = _cnn()
    tbs = _tbs(cnn)
    tok = N.tokens(3, L, 1)
    got = R.ref64(N.backbone, N.onehot5(tok), N.backbone_params(cnn, tbs))
    c64 = copy.deepcopy(cnn).double()
    with torch.no_grad():
        want = c64.trunk(N.onehot5(tok).double().permute(0, 2, 1), [t.double().reshape(1, -1, 1) for t in tbs]).permute(0, 2, 1)
    err = float((got - want).abs().max())
    assert got.shape == (3, L, 5) and err <= 1e-12, err


def test_value_net_restatement_equals_the_float64_modules():
    from svdd_amd.value_nets import ConvGRUTrunk, ConvHead
    torch.manual_seed(3)
    emb, head = ConvGRUTrunk().eval(), ConvHead(3, 64).eval()
    N.distinct_layers(emb, 2)
    x = N.onehot4(N.tokens(4, 37, 2))
    got = R.ref64(N.value_net, x, N.value_params(emb, head))
    with torch.no_grad():
        want = copy.deepcopy(head).double()(copy.deepcopy(emb).double()(x.double()))[:, :, 0]
    err = float((got - want).abs().max())
    assert got.shape == (4, 3) and err <= 1e-13, err
    p = N.value_params(emb, head)
    assert p["residual_mask"] == 31 and len(p["ws"]) == 5


def test_gru_restatement_equals_nn_gru_in_float64():
    mod, x, _ = R.gru_inputs(5, 7)
    got = R.ref64(N.gru_out, x, R.gru_weights_of(mod))
    with torch.no_grad():
        want = copy.deepcopy(mod).double()(x.double())[0]
    assert float((got[0] - want[:, :, :64]).abs().max()) <= 1e-14 and float((got[1] - want[:, :, 64:]).abs().max()) <= 1e-14
    assert torch.equal(R.ref64(N.gru_out_lp, x, R.gru_weights_of(mod)), got)          # outside ref_lp the lp form is the same function


def test_distinct_layers_leaves_no_equal_pair_and_random_init_has_equal_groups():
    from svdd_amd import synthetic
    from svdd_amd.value_nets import ConvGRUTrunk
    model, emb, _, _ = synthetic.build("dna", "cpu")
    cnn = model.backbone
    pairs = N.equal_pairs(cnn)
    for g in range(5):                                   # 5 groups of 4 bit-identical layers: 6 pairs each
        for i in range(4 * g, 4 * g + 4):
            assert torch.equal(cnn.convs[i].weight, cnn.convs[4 * g].weight) and torch.equal(cnn.convs[i].bias, cnn.convs[4 * g].bias)
    assert len([p for p in pairs if p[0].startswith("convs.") and p[1].startswith("convs.")]) == 30
    assert not N.equal_pairs(emb)                        # the value net's layers are drawn one by one
    before = [c.weight.clone() for c in cnn.convs]
    N.distinct_layers(cnn, 1)
    assert not N.equal_pairs(cnn)
    for c, w0 in zip(cnn.convs, before):                 # the default initialisation's scale
        assert 0.8 <= float(c.weight.abs().max() / w0.abs().max()) <= 1.25
    for nm in cnn.norms:
        assert 0.5 <= float(nm.weight.min()) and float(nm.weight.max()) <= 1.5 and float(nm.bias.abs().max()) <= 0.3
    a, b = N.distinct_layers(ConvGRUTrunk(), 4), N.distinct_layers(ConvGRUTrunk(), 4)
    assert all(torch.equal(p, q) for p, q in zip(a.parameters(), b.parameters()) if p.dim() == 3)     # seeded


def test_swapping_two_layers_of_one_group_moves_the_logits_far_beyond_the_bar():
    cnn = _cnn()
    tok = N.tokens(2, 50, 3)
    p = N.backbone_params(cnn, _tbs(cnn))
    r64, r32 = R.ref64(N.backbone, N.onehot5(tok), p), R.ref32(N.backbone, N.onehot5(tok), p)
    q = dict(p, ws=list(p["ws"]))
    q["ws"][17], q["ws"][18] = p["ws"][18], p["ws"][17]
    moved = float((R.ref64(N.backbone, N.onehot5(tok), q) - r64).abs().max())
    b = R.bar(8, r32, r64)
    print(f"swap moves the logits by {moved:.3g}; bar {b:.2g}")
    assert 2e-8 <= b <= 2e-5 and moved >= 1e3 * b


def test_ref32_and_ref_lp_give_the_bars_order_of_magnitude():
    cnn = _cnn()
    tok = N.tokens(2, 50, 4)
    p = N.backbone_params(cnn, _tbs(cnn))
    oh = N.onehot5(tok)
    r64 = R.ref64(N.backbone, oh, p)
    e32 = float((R.ref32(N.backbone, oh, p).double() - r64).abs().max())
    assert 1e-8 <= e32 <= 1e-5, e32
    p["lscale"] = torch.ones(len(p["dil"]) + 1, 2)
    errs = {m: float((N.ref_lp(m, N.backbone, oh, p).double() - r64).abs().max()) for m in N.LP_DTYPES}
    print("backbone ref32", e32, "ref_lp", errs)
    assert errs["f16x3"] <= 3e-5 and errs["bf16x3"] <= 3e-4 and 1e-5 <= errs["f16"] <= 2e-2 and 1e-4 <= errs["bf16"] <= 1e-1
    assert errs["f16x3"] < errs["bf16x3"] < errs["f16"] < errs["bf16"]
    # tower, GRU and tail
    stem_w, b, ws = N.tower_inputs(5, 0)
    x4 = N.onehot4(N.tokens(3, 37, 5))
    t64 = R.ref64(N.tower, x4, stem_w, b, ws, 31)
    assert float((R.ref32(N.tower, x4, stem_w, b, ws, 31).double() - t64).abs().max()) <= 1e-5
    assert float((N.ref_lp("bf16", N.tower, x4, stem_w, b, ws, 31).double() - t64).abs().max()) <= 1e-1
    mod, x, _ = R.gru_inputs(3, 7)
    w = R.gru_weights_of(mod)
    g64 = R.ref64(N.gru_out, x, w)
    assert float((R.ref32(N.gru_out, x, w).double() - g64).abs().max()) <= 1e-5
    assert float((N.ref_lp("f16x3", N.gru_out_lp, x, w).double() - g64).abs().max()) <= 1e-5
    assert 1e-5 <= float((N.ref_lp("bf16", N.gru_out_lp, x, w).double() - g64).abs().max()) <= 1e-1
    args = N.tail_inputs(3, 17, 2)
    h, rest = args[0], args[1:]
    s64 = R.ref64(N.tail, h[0], h[1], *rest)
    assert float((R.ref32(N.tail, h[0], h[1], *rest).double() - s64).abs().max()) <= 1e-5
    assert float((N.ref_lp("f16", N.tail, h[0], h[1], *rest).double() - s64).abs().max()) <= 2e-2


def test_windows_restatement_covers_every_changed_position_and_its_margin():
    g = R._gen(15)
    B, M, L = 4, 5, 200
    x = torch.randint(0, 5, (B, L), generator=g)
    cand = x[:, None, :].repeat(1, M, 1)
    cand[0, 1, 0] ^= 1
    cand[1, 2, L - 1] ^= 1
    cand[2, 3, 28] ^= 1                                   # 28 - 27 = 1: w0 = 0; 27 - 27 = 0 likewise; 43 - 27 = 16
    cand[3, 4, 43] ^= 1
    win, flags = N.windows(cand, x, 27)
    assert win.dtype == torch.int32 and win[0].tolist() == [0, 0] and int(flags[0]) == 0
    assert win[1].tolist() == [0, 32] and win[1 * M + 2].tolist() == [160, 208] and win[2 * M + 3].tolist() == [0, 64]
    assert win[3 * M + 4].tolist() == [16, 80] and flags[3 * M + 4] == 4
    assert bool((win % 16 == 0).all()) and int(win.max()) <= 208
