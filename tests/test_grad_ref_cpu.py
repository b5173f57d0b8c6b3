"""The float64 reference of the reward net's gradient pass (tests/grad_ref.py) proved against torch autograd through the plain
modules (nn.GRU, F.conv1d, F.layer_norm, F.linear) in float64, to 1e-12 of the scale; and the shares of elements / rows / sequences
the GPU tests (tests/test_grad_kernels_gpu.py) may exclude as ReLU kinks shown to stay inside their caps, from the reference alone,
for every seed and shape that file uses. No GPU."""
import copy

import pytest
import torch
import torch.nn.functional as F

from tests import grad_ref as R

TOL = 1e-12


def _close(got, want, what):
    scale = max(float(want.abs().max()), 1e-300)
    err = float((got - want).abs().max())
    assert err <= TOL * scale, (what, err, scale)


def _d(*ts):
    return [t.double() for t in ts]


@pytest.mark.parametrize("n,L", [(1, 7), (3, 50), (2, 200)])
def test_stem_and_its_transpose_vs_conv1d_autograd(n, L):
    x, w, b, g = _d(*R.stem_inputs(n, L))
    xr = x.clone().requires_grad_(True)
    want = F.relu(F.conv1d(xr.transpose(1, 2), w, b, padding=7)).transpose(1, 2)
    _close(R.stem(x, w, b), want.detach(), "stem")
    gm = torch.where(want > 0, g, torch.zeros_like(g))                 # the gradient at the pre-activation
    (dx,) = torch.autograd.grad(want, xr, g)
    _close(R.stem_bwd(gm, w), dx, "stem_bwd")
    assert bool((R.stem_terms(x, w, b) >= R.stem_pre(x, w, b).abs()).all())


@pytest.mark.parametrize("n,L", [(1, 200), (5, 50), (2, 3)])
@pytest.mark.parametrize("res,gated", [(True, True), (False, True), (True, False), (False, False)])
def test_conv_gated_vs_conv1d_autograd(n, L, res, gated):
    gen = torch.Generator().manual_seed(n * 100 + L)
    w5 = torch.randn(64, 64, 5, generator=gen, dtype=torch.float64) * 0.1
    b = torch.randn(64, generator=gen, dtype=torch.float64)
    g = torch.randn(n, L, 64, generator=gen, dtype=torch.float64)
    f = torch.randn(n, L, 64, generator=gen, dtype=torch.float64)
    fr = f.clone().requires_grad_(True)
    a = F.relu(fr) if gated else fr                                     # the layer below: its ReLU is this layer's gate
    out = F.conv1d(a.transpose(1, 2), w5, b, padding=2).transpose(1, 2)
    if res:
        out = out + a
    (want,) = torch.autograd.grad(out, fr, g)
    _close(R.conv_gated(g, w5, g if res else None, f if gated else None), want, "conv_gated")
    _close(R.conv_act1(f, w5, b, f if res else None), (F.conv1d(f.transpose(1, 2), w5, b, padding=2).transpose(1, 2) + (f if res else 0)),
           "conv_act1")


def _gru_from_gi(gi, w, n, L):
    """The recurrence as a function of the input halves gi [2, n, L, 192] (a leaf autograd can differentiate): torch's documented
    cell, n = tanh(gi_n + r (W_hn h + b_hn)), with b_hr and b_hz already inside gi."""
    outs = []
    for d in range(2):
        h = torch.zeros(n, 64, dtype=gi.dtype)
        hs = [None] * L
        for t in (range(L) if d == 0 else range(L - 1, -1, -1)):
            gh = F.linear(h, w["w_hh"][d])
            r = torch.sigmoid(gi[d, :, t, :64] + gh[:, :64])
            z = torch.sigmoid(gi[d, :, t, 64:128] + gh[:, 64:128])
            c = torch.tanh(gi[d, :, t, 128:] + r * (gh[:, 128:] + w["b_hh"][d][128:]))
            h = (1 - z) * c + z * h
            hs[t] = h
        outs.append(torch.stack(hs, dim=1))
    return torch.stack(outs)


@pytest.mark.parametrize("n,L", [(1, 1), (3, 2), (5, 7), (2, 50), (17, 200)])
def test_gru_forward_saved_gates_and_bptt_vs_nn_gru_autograd(n, L):
    mod, x, gout = R.gru_inputs(n, L)
    w = R.to(torch.float64, R.gru_weights_of(mod))
    x, gout = x.double(), gout.double()
    m64 = copy.deepcopy(mod).double()
    xr = x.clone().requires_grad_(True)
    y = m64(xr)[0]
    want_out = torch.stack([y[:, :, :64], y[:, :, 64:]])
    (want_dx,) = torch.autograd.grad(want_out, xr, gout)
    fw = R.gru(x, w)
    _close(fw["out"], want_out.detach(), "gru out")
    # gi and the recurrence on it: the same function as nn.GRU, so its autograd is the witness of `da`
    gi = fw["gi"].reshape(2, n, L, 192).clone().requires_grad_(True)
    for d in range(2):
        bias = w["b_ih"][d] + torch.cat([w["b_hh"][d][:128], torch.zeros(64, dtype=torch.float64)])
        _close(fw["gi"][d], F.linear(x, w["w_ih"][d], bias).reshape(n * L, 192), "gi")
    out_gi = _gru_from_gi(gi, w, n, L)
    _close(out_gi.detach(), want_out.detach(), "recurrence on gi")
    (want_da,) = torch.autograd.grad(out_gi, gi, gout)
    # the saved planes: gates in (0, 1) / (-1, 1), and they reconstruct the hidden states
    r, z, c, lin = (fw["save"][:, :, :, k] for k in range(4))
    assert bool(((r > 0) & (r < 1) & (z > 0) & (z < 1) & (c.abs() < 1)).all())
    for d in range(2):
        hp = torch.zeros_like(fw["out"][d])
        if L > 1:
            if d == 0:
                hp[:, 1:] = fw["out"][d][:, :-1]
            else:
                hp[:, :-1] = fw["out"][d][:, 1:]
        _close((1 - z[d]) * c[d] + z[d] * hp, fw["out"][d], "h from the saved gates")
        _close(lin[d], F.linear(hp, w["w_hh"][d][128:], w["b_hh"][d][128:]), "saved W_hn h + b_hn")
        _close(c[d], torch.tanh(fw["gi"][d].reshape(n, L, 192)[:, :, 128:] + r[d] * lin[d]), "saved n")
    # BPTT from the saved gates = autograd through the recurrence
    bw = R.gru_bwd(gout, fw["out"], fw["save"], w)
    _close(bw["da"], want_da.reshape(2, n * L, 192), "da")
    _close(bw["dx"][0] + bw["dx"][1], want_dx, "dx")
    gate = x - 0.3
    (lin_dx,) = torch.autograd.grad(torch.stack([F.linear(xr, w["w_ih"][d]) for d in range(2)]), xr, bw["da"].reshape(2, n, L, 192))
    _close(R.gru_dx_gate(bw["da"], w, None), lin_dx.reshape(n * L, 64), "dx from da")
    _close(R.gru_dx_gate(bw["da"], w, gate), torch.where(gate > 0, want_dx, torch.zeros_like(want_dx)).reshape(n * L, 64), "gated dx")
    for d in range(2):
        _close(bw["dx"][d], (bw["da"][d] @ w["w_ih"][d]).reshape(n, L, 64), "dx per direction")


def test_kernel_stated_activations_are_the_same_functions():
    a = torch.linspace(-20, 20, 4001, dtype=torch.float64)
    R._FAST[0] = True
    try:
        s, t = R._sigmoid(a), R._tanh(a)
    finally:
        R._FAST[0] = False
    assert float((s - torch.sigmoid(a)).abs().max()) <= 1e-15 and float((t - torch.tanh(a)).abs().max()) <= 1e-15


@pytest.mark.parametrize("n,L", [(1, 1), (1, 7), (3, 50), (7, 200)])
def test_tail_grad_vs_layer_norm_linear_autograd(n, L):
    h, w1, b1, gam, bet, weff = _d(*R.tail_inputs(n, L))
    hr = h.clone().requires_grad_(True)
    z = F.linear(F.layer_norm(hr[0] + hr[1], (64,), gam, bet, 1e-5), w1, b1)
    (F.relu(z) @ weff).mean(dim=1).mean().backward()
    g, z_ref = R.tail_grad(h[0], h[1], w1, b1, gam, bet, weff, 1e-5)
    _close(z_ref, z.detach(), "tail z")
    _close(g, hr.grad[0], "tail grad")
    assert torch.equal(hr.grad[0], hr.grad[1])


@pytest.mark.parametrize("C", R.BB_CHANNELS)
@pytest.mark.parametrize("rows,rps", [(1, 1), (5, 1), (600, 200), (600, 50), (103, 7)])
def test_bb_layer_pair_vs_layer_norm_autograd(rows, rps, C):
    d = {k: (v.double() if v.is_floating_point() else v) for k, v in R.bb_inputs(rows, rps, C).items()}
    seq = torch.arange(rows) // rps
    for with_y in (True, False):
        for with_ln in (True, False):
            if not with_y and not with_ln:
                continue
            res = R.bb_layer_fwd(d["y"] if with_y else None, d["bias"], d["f_prev"], d["tb"], d["gamma"] if with_ln else None, d["beta"],
                                 1e-5, rps)
            f_want = F.relu(d["y"] + d["bias"]) + d["f_prev"] if with_y else d["f_prev"]
            _close(res["f_out"], f_want, "f_out")
            if with_y:
                assert torch.equal(res["mask"], d["y"] + d["bias"] > 0)
            if with_ln:
                _close(res["hn"], F.layer_norm(f_want + d["tb"][seq], (C,), d["gamma"], d["beta"], 1e-5), "hn")
            else:
                assert res["hn"] is None
    fr = d["f_prev"].clone().requires_grad_(True)
    hn = F.layer_norm(fr + d["tb"][seq], (C,), d["gamma"], d["beta"], 1e-5)
    (gl,) = torch.autograd.grad(hn, fr, d["g_hn"])
    for mp in (d["mask_prev"], None):
        res = R.bb_layer_bwd(d["g_hn"], d["f_prev"], d["tb"], d["gamma"], 1e-5, d["g_in"], mp, rps)
        _close(res["g_out"], d["g_in"] + gl, "g_out")
        if mp is None:
            assert res["gt_out"] is None
        else:
            _close(res["gt_out"], (d["g_in"] + gl) * mp, "gt_out")


def test_sum_gate_shuts_on_both_zeros():
    f = torch.tensor([1.0, 0.0, -0.0, -1.0, 1e-45, -1e-45], dtype=torch.float32)
    a, b = torch.arange(6, dtype=torch.float32) + 1, torch.ones(6)
    assert R.sum_gate(a, b, f).tolist() == [2.0, 0.0, 0.0, 0.0, 6.0, 0.0]


def _value_net(task):
    from svdd_amd import synthetic
    from svdd_amd.fused import FusedValueNet
    _, _, _, reward = synthetic.build(task, "cpu")
    return reward, FusedValueNet(reward.embedding, reward.head)


@pytest.mark.parametrize("task,B", [("dna", 3), ("rna", 5)])
def test_whole_pass_vs_autograd_through_the_reward_model(task, B):
    """value_grad with the reference's own tower decisions = autograd through the plain float64 reward model (which also proves the
    natural-layout weights params_of reads, BatchNorm fold and collapsed head included)."""
    reward, fn = _value_net(task)
    L = 200 if task == "dna" else 50
    p = R.to(torch.float64, R.params_of(fn))
    x = R.pass_input(task, B, L).double()
    xr = x.clone().requires_grad_(True)
    copy.deepcopy(reward).double()(xr.transpose(1, 2))[:, 0].mean().backward()
    res = R.value_grad(x, p, [m.double() for m in R.free_masks(x, p)])
    # (the fused net folds the eval-mode BatchNorm and collapses the head in fp32: each a float64 product rounded once, 6e-8 relative)
    scale = float(xr.grad.abs().max())
    assert float((res["grad"] - xr.grad).abs().max()) <= 5e-7 * scale
    # ... and exactly the same function once those two products are made in float64 from the reward model's own weights
    head, d2 = reward.head.channel_transform.conv.layer, reward.embedding.gru_tower.ffn.dense2.linear
    p["w_eff"] = (head.weight.detach()[:, :, 0].double() @ d2.weight.detach().double())[0]
    for k, blk in enumerate(reward.embedding.conv_tower.blocks[1:]):
        bn = blk.norm.layer
        w, b = blk.conv.weight.detach().double(), blk.conv.bias.detach().double()
        if isinstance(bn, torch.nn.BatchNorm1d):
            s = bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)
            w, b = w * s[:, None, None], (b - bn.running_mean.double()) * s + bn.bias.detach().double()
        p["ws"][k], p["bs"][k] = w, b
    res = R.value_grad(x, p, [m.double() for m in R.free_masks(x, p)])
    _close(res["grad"], xr.grad, "value_grad")


# ---------------------------------------------------------------------------------------------- exclusion shares stay capped
@pytest.mark.parametrize("n,L", R.STEM_CASES)
def test_stem_kink_share_within_cap(n, L):
    x, w, b, _ = _d(*R.stem_inputs(n, L))
    share = float(R.near_kink(R.stem_pre(x, w, b), R.stem_terms(x, w, b)).double().mean())
    assert share <= R.STEM_KINK_CAP, share


@pytest.mark.parametrize("n,L", R.TAIL_CASES)
def test_tail_kink_row_share_within_cap(n, L):
    h, w1, b1, gam, bet, weff = _d(*R.tail_inputs(n, L))
    _, z = R.tail_grad(h[0], h[1], w1, b1, gam, bet, weff, 1e-5)
    share = float(R.tail_kink_rows(z).double().mean())
    assert share <= R.TAIL_ROW_CAP, share


@pytest.mark.parametrize("C", R.BB_CHANNELS)
@pytest.mark.parametrize("rows,rps", R.BB_CASES)
def test_bb_mask_kink_share_within_cap(rows, rps, C):
    d = R.bb_inputs(rows, rps, C)
    y, bias = d["y"].double(), d["bias"].double()
    share = float(R.near_kink(y + bias, y.abs() + bias.abs()).double().mean())
    assert share <= R.MASK_KINK_CAP, share


@pytest.mark.parametrize("task,B", R.PASS_CASES)
def test_whole_pass_kink_sequences_within_cap(task, B):
    _, fn = _value_net(task)
    L = 200 if task == "dna" else 50
    p = R.to(torch.float64, R.params_of(fn))
    x = R.pass_input(task, B, L).double()
    res = R.value_grad(x, p, [m.double() for m in R.free_masks(x, p)])
    assert int(R.tail_kink_seqs(res["z"]).sum()) <= R.seq_cap(B)
