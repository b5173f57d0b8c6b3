"""No GPU: the value function's training data (MC / CD-Q rollouts, ABI 17).

  fixtures  g34 / g35 (the reference's own _sample(cdq=True) and nets, tests/golden/make_golden_cdq.py): the restated sequential fp32
            mean reproduces the recorded targets bit for bit, the recorded lists have the reference's structure, and the assembled
            training set has its order
  entry     svdd_value_target refuses bad arguments before it touches a device
  harness   BaseModel.train() keeps the frozen nets in eval mode; forward outside training is the plain supervised loss
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import cdq_ref as C
from tests.conftest import load_golden

FIXTURES = ["g34_cdq_tiny.npz", "g35_cdq_full.npz"]


@pytest.mark.parametrize("name", FIXTURES)
def test_restated_mean_is_the_recorded_target_bit_for_bit(name):
    """The numpy restatement (sequential fp32 sum in ascending draw order, one fp32 division) over the recorded eval-mode values of
    steps 1 .. S - 1 IS the reference's `case_sum / len` tensor: 0 elements differ. A pairwise sum, a float64 mean or a product with
    1 / M does not reproduce it: the order is pinned to the reference's."""
    g = load_golden(name)
    S, draws = int(g["S"]), int(g["draws"])
    values, y = g["values"], g["y_cdq"]
    B = y.shape[1]
    assert values.shape == (S, draws, B) and values.dtype == np.float32 and y.shape == (S - 1, B) and y.dtype == np.float32
    got = C.seq_mean_f32(np.moveaxis(values[1:], 1, -1))
    assert got.dtype == np.float32 and got.tobytes() == y.tobytes()
    others = {"float64 mean": values[1:].astype(np.float64).mean(1).astype(np.float32),
              "times 1 / M": (np.moveaxis(values[1:], 1, -1).cumsum(-1, dtype=np.float32)[..., -1] * np.float32(1.0 / draws)),
              "descending": C.seq_mean_f32(np.moveaxis(values[1:, ::-1], 1, -1))}
    assert any(v.astype(np.float32).tobytes() != y.tobytes() for v in others.values())
    # step pairing: the targets of neighbouring steps are far apart next to the engine tests' 1e-4
    assert np.abs(y[1:] - y[:-1]).mean() > 5e-4 and np.abs(y - np.moveaxis(values[:-1], 1, -1).mean(-1)).mean() > 5e-4


@pytest.mark.parametrize("name", FIXTURES)
def test_recorded_lists_and_the_assembled_training_set(name):
    g = load_golden(name)
    S, draws = int(g["S"]), int(g["draws"])
    all_mid, mid, final = g["all_mid"], g["mid"], g["final"]
    _, _, B, L = all_mid.shape
    assert all_mid.shape[:2] == (S, draws) and mid.shape == (S - 1, B, L) and final.shape == (B, L)
    assert np.array_equal(mid, all_mid[:S - 1, -1])                            # mid_x[i] is all_time_mid_x[i][-1]
    assert final.max() <= 3 and all_mid.max() <= C.MASK
    # a draw keeps every token of the state it was drawn from (the last draw of the step before), and so does x_0
    prev = np.concatenate([np.full((1, B, L), C.MASK, np.uint8), all_mid[:-1, -1]])
    keep = prev != C.MASK
    assert all(np.array_equal(all_mid[:, j][keep], prev[keep]) for j in range(draws))
    assert np.array_equal(final[all_mid[-1, -1] != C.MASK], all_mid[-1, -1][all_mid[-1, -1] != C.MASK])
    states, y = C.assemble_cdq(all_mid, g["values"], final, g["reward"])
    assert states.shape == (S, B, L) and y.shape == (S * B,) and y.dtype == np.float32
    assert np.array_equal(states[:-1], mid) and np.array_equal(states[-1], final)
    assert y[:(S - 1) * B].tobytes() == g["y_cdq"].tobytes() and np.array_equal(y[(S - 1) * B:], g["reward"])
    for k, b in ((0, 0), (S - 2, B - 1)):                                      # row k B + b pairs state k with step k + 1's draws
        assert y[k * B + b] == C.seq_mean_f32(g["values"][k + 1, :, b])
    oh = C.onehot(states).reshape(S * B, L, 4)
    assert np.array_equal(oh.sum(-1), (states != C.MASK).reshape(S * B, L).astype(np.float32))
    ms, my = C.assemble_mc(g["mc_mid"], g["mc_final"], g["mc_reward"])
    assert ms.shape == (S, B, L) and np.array_equal(my.reshape(S, B), np.broadcast_to(g["mc_reward"], (S, B)))


def test_reductions_special_values():
    inf, nan = np.inf, np.nan
    assert C.seq_mean_f32([[1e8, 1.0, -1e8]])[0] == 0.0                        # fl(1e8 + 1) = 1e8: the sequential order shows
    assert C.seq_mean_f32([[1.0, -1e8, 1e8]])[0] == np.float32(0.0) and C.seq_mean_f32([[1e8, -1e8, 1.0]])[0] == np.float32(1.0) / np.float32(3)
    assert np.isnan(C.seq_mean_f32([[inf, -inf, 0.0]])[0]) and C.seq_mean_f32([[inf, 1.0]])[0] == inf
    for f in (C.logmeanexp_f64, C.logmeanexp_f32):
        for a in (0.1, 1.0, 10.0):
            out = f([[nan, 1.0, 2.0], [inf, 1.0, nan], [inf, 0.0, 1.0], [-inf, -inf, -inf], [-inf, 2.0, -inf], [3.0, 3.0, 3.0]], a)
            assert np.isnan(out[0]) and np.isnan(out[1]) and out[2] == inf and out[3] == -inf
            assert abs(out[4] - (2.0 + a * np.log(1 / 3))) < 1e-5 * max(1.0, a) and out[5] == 3.0
            assert f([[0.37]], a)[0] == np.float32(0.37)                       # M = 1: the score itself


def test_value_target_entry_refuses_bad_arguments_without_a_device():
    from svdd_amd import _lib
    L_ = _lib.lib()
    assert _lib.ABI_VERSION == 17 and L_.svdd_abi_version() == 17
    p, q, f, t = (ctypes.c_void_p(v) for v in (4096, 8192, 12288, 16384))     # non-NULL pointers that are never dereferenced
    ok = (f, p, 2, 8, 3, _lib.TARGET_MEAN, 1.0, q, None, t, None)

    def with_(**kw):
        names = ("scores", "cand", "B", "L", "M", "reduce", "alpha", "x_next", "onehot_next", "target", "stream")
        return tuple(kw.get(n, v) for n, v in zip(names, ok))
    lme = _lib.TARGET_LOGMEANEXP
    bad = {"cand null": with_(cand=None), "x_next null": with_(x_next=None), "B = 0": with_(B=0), "L = 0": with_(L=0),
           "M = 0": with_(M=0), "B < 0": with_(B=-1), "M > MAX_M": with_(M=_lib.MAX_M + 1), "reduce 2": with_(reduce=2),
           "reduce -1": with_(reduce=-1), "alpha 0": with_(reduce=lme, alpha=0.0), "alpha < 0": with_(reduce=lme, alpha=-1.0),
           "alpha nan": with_(reduce=lme, alpha=float("nan")), "alpha inf": with_(reduce=lme, alpha=float("inf")),
           "scores without target": with_(target=None), "target without scores": with_(scores=None),
           "x_next is cand": with_(x_next=p)}
    for what, a in bad.items():
        assert L_.svdd_value_target(*a) == _lib.E_ARG, what
    sig = _lib.SIGNATURES["svdd_value_target"]
    assert sig[-1] is _lib.vp and sig[-1] is not _lib.STREAM                 # the stream is the caller's to pass (`on_stream`)


def _tiny_harness(**kw):
    from svdd_amd.config import Config, ModelConfig, SamplingConfig
    from svdd_amd.diffusion import Diffusion
    from svdd_amd.harness import BaseModel
    from svdd_amd.value_nets import ConvGRUTrunk, ConvHead, RewardModel
    torch.manual_seed(0)
    cfg = Config(model=ModelConfig(hidden_dim=16, num_cnn_stacks=1, length=20), sampling=SamplingConfig(steps=4))
    model = Diffusion(cfg)
    mk = lambda: (ConvGRUTrunk(stem_in_channels=4, stem_channels=8, stem_kernel_size=15, n_conv=3, channel_init=8, kernel_size=5,  # noqa: E731
                               dropout=0.1), ConvHead(1, 8))
    emb, head = mk()
    return BaseModel(emb, head, model, RewardModel(*mk()), 4, **kw)


def test_train_keeps_the_frozen_nets_in_eval_mode():
    h = _tiny_harness()
    assert h.cdq is False and h.cdq_alpha is None and isinstance(h.loss_fct, torch.nn.MSELoss)
    for mode in (True, False, True):
        assert h.train(mode) is h
        assert h.training == mode and h.embedding.training == mode and h.head.training == mode
        assert all(m.training == mode for m in h.embedding.modules())
        assert not any(m.training for m in h.ref_model.modules()) and not any(m.training for m in h.reward_model.modules())
    h.eval()
    assert not h.training and not h.embedding.training and not h.ref_model.training
    assert not any(p.requires_grad for p in h.ref_model.parameters()) and not any(p.requires_grad for p in h.reward_model.parameters())
    h2 = _tiny_harness(cdq=True, cdq_alpha=0.5)
    assert h2.cdq is True and h2.cdq_alpha == 0.5


def test_forward_outside_training_is_the_supervised_loss():
    h = _tiny_harness().eval()
    g = torch.Generator().manual_seed(1)
    x0 = torch.nn.functional.one_hot(torch.randint(0, 4, (6, 20), generator=g), 4).float()
    y = torch.randn(6, 1, generator=g)
    loss = h(x0=x0, y=y)
    want = torch.nn.functional.mse_loss(h.head(h.embedding(x0)).view(-1), y.view(-1))
    assert loss.shape == () and torch.equal(loss, want)
    loss.backward()
    assert all(p.grad is not None for p in h.head.parameters())
    assert all(p.grad is None for p in h.ref_model.parameters()) and all(p.grad is None for p in h.reward_model.parameters())


def test_training_forward_has_no_cpu_fallback():
    from svdd_amd import ops
    h = _tiny_harness().train()
    with pytest.raises(ops.SvddError):
        h()


def test_gru_block_chunks_an_oversized_batch():
    """A training batch of steps x batch rows is beyond what one call of the vendor RNN library takes: GRUBlock sends the rows
    through in chunks. Same outputs and gradients as the one call (rows are independent), and a batch below the limit is one call."""
    from svdd_amd.value_nets import GRUBlock
    torch.manual_seed(0)
    g = GRUBlock(8).eval()
    x = torch.randn(10, 8, 7)
    calls = []
    g.gru.register_forward_hook(lambda m, a, o: calls.append(a[0].shape[0]))
    outs, grads = [], []
    for limit in (GRUBlock.gru_call_bytes, 3 * 7 * 6 * 8 * 4, 1):
        g.gru_call_bytes = limit
        xi = x.clone().requires_grad_(True)
        g.zero_grad()
        y = g(xi)
        y.square().sum().backward()
        outs.append(y.detach()), grads.append((xi.grad, g.gru.weight_hh_l0.grad.clone()))
    assert calls == [10] + [3, 3, 3, 1] + [1] * 10
    for y, (gx, gw) in zip(outs[1:], grads[1:]):
        assert torch.allclose(y, outs[0], rtol=1e-5, atol=1e-6) and torch.allclose(gx, grads[0][0], rtol=1e-5, atol=1e-6)
        assert torch.allclose(gw, grads[0][1], rtol=1e-4, atol=1e-5)
