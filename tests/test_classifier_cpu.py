"""Classifier guidance (reference diffusion_gosai.py:1064-1104, 1332-1371; Enformer.py:639-716; decode_classfier.py), CPU side:

  * `Diffusion.compute_gradient` on the PyTorch mirrors of the reference's nets equals the gradients the reference recorded in its
    own runs (g27: tiny nets, g28: full-size nets);
  * the numpy restatement of one guided step (`guided_step`: SUBS and the race from the C oracle, q and w in fp32 with one rounding
    per operation) reproduces every recorded next state of g27 / g28 token for token. The GPU tests (test_classifier_gpu.py) check
    svdd_classifier_propose against this restatement;
  * argument validation of svdd_classifier_propose, the API surface, the guidance_scale=None refusal, the CLI parser."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from oracle import svdd_oracle as orc

MASK = 4


def guided_step(logits, x, grad4, dm, mcs, scale, u):
    """One step of _ddpm_update_finetune_classfier after its two net passes. logits, u: logical [B, L, 5] (any strides); x u8 [B, L];
    grad4 [B, L, 4]. -> (x_next u8 [B, L], un-guided q [B, L, 5], guided weights w [B, L, 5])."""
    x = np.ascontiguousarray(x, np.uint8)
    lp = orc.subs_logp(np.ascontiguousarray(logits, np.float32), x)
    q = (np.exp(lp.astype(np.float64)).astype(np.float32) * np.float32(dm)).astype(np.float32)       # :1350-1351
    q[..., MASK] = np.float32(mcs)                                                                   # :1352
    g5 = np.concatenate([np.asarray(grad4, np.float32), np.zeros(x.shape + (1,), np.float32)], axis=2)
    w = (q + (np.float32(scale) * g5).astype(np.float32)).astype(np.float32)                         # :1355-1357
    x_next = orc.sample_categorical_merged(w, x, np.ascontiguousarray(u, np.float32)[None])[:, 0]    # :30-34, :1358-1359
    return x_next, q, w


def ulps(a, b):
    a, b = np.asarray(a, np.float32).view(np.int32).astype(np.int64), np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return int(np.abs(a - b).max())


def tiny_cpu(golden, g):
    from tests import e2e_parity
    return e2e_parity.tiny_engine(golden("nets_tiny.npz"), int(g["L"]), int(g["S"]), "cpu")


def full_cpu(g):
    from svdd_amd import synthetic
    model, emb, head, _ = synthetic.build("dna", "cpu")
    for name, mod in (("backbone", model.backbone), ("embedding", emb), ("head", head)):
        sums = np.array([float(p.double().sum()) for p in mod.state_dict().values()])
        assert np.allclose(sums, g[name + "_param_sums"], rtol=0, atol=1e-6), name
    return model, emb, head


def _nets(golden, name):
    g = golden(name)
    return g, (tiny_cpu(golden, g) if "full" not in name else full_cpu(g))


@pytest.mark.parametrize("name", ["g27_traj_classifier.npz", "g28_traj_classifier_full.npz"])
def test_compute_gradient_equals_reference_recording(golden, name):
    """compute_gradient (pure autograd) on the engine's PyTorch mirrors, CPU fp32, against the reference's compute_gradient of the
    same states: the same function through the same CPU kernels."""
    g, (model, emb, head) = _nets(golden, name)
    worst = 0.0
    for i in range(int(g["S"])):
        oh = model.transform_samples(torch.from_numpy(g["xs"][i]).long()).float()
        mine = model.compute_gradient(oh, emb, head).numpy()
        ref = g["grad"][i]
        worst = max(worst, float(np.abs(mine - ref).max() / np.abs(ref).max()))
    print(name, "compute_gradient: max |g - g_ref| / max |g_ref| =", worst)
    assert worst <= 1e-5, worst


@pytest.mark.parametrize("name", ["g27_traj_classifier.npz", "g28_traj_classifier_full.npz"])
def test_restatement_reproduces_every_reference_step(golden, name):
    """guided_step with the reference's logits, gradient and uniforms gives its q_xs, its guided weights (negative ones included) and
    its next state at every recorded step."""
    g = golden(name)
    S, L, scale = int(g["S"]), int(g["L"]), float(g["scale"])
    assert tuple(g["u_strides"]) == (5 * L, 1, L) and tuple(g["w_strides"]) == (5 * L, 1, L)      # rand_like in [b][v][l] order
    assert int(g["n_negative"]) > 0 and int(g["n_changed"]) > 0
    sched = g["sched"]
    n_neg = 0
    for i in range(S):
        x_next, q, w = guided_step(g["logits"][i], g["xs"][i], g["grad"][i], sched[i, 5], sched[i, 4], scale, g["u"][i])
        # q: the correctly rounded exp / log of the arithmetic contract against torch's CPU ones (a few ulps at a few positions)
        assert ulps(q, g["q"][i]) <= 4, (i, ulps(q, g["q"][i]))
        assert np.abs(w - g["w"][i]).max() <= 4 * np.spacing(np.abs(g["q"][i]).max()), i
        g5 = np.concatenate([g["grad"][i], np.zeros(g["grad"][i].shape[:2] + (1,), np.float32)], axis=2)
        assert np.array_equal(g["w"][i], (g["q"][i] + (np.float32(scale) * g5).astype(np.float32)).astype(np.float32)), i   # the order
        assert np.array_equal(x_next, g["x_next"][i]), i
        if i + 1 < S:
            assert np.array_equal(g["x_next"][i], g["xs"][i + 1])
        n_neg += int((w < 0).sum())
    assert n_neg == int(g["n_negative"])


def test_c2_fixture_is_consistent():
    """g29 (B = 256, L = 200, 128 steps): the state encoding gives nested masks, and the stored guided weights are
    fl(q + fl(scale * cat(grad, 0))) bit for bit — the fp32 order the kernel implements."""
    from tests.conftest import load_golden
    g = load_golden("g29_traj_classifier_c2.npz")
    S, B, L, scale = int(g["S"]), int(g["B"]), int(g["L"]), np.float32(float(g["scale"]))
    assert g["unmask_step"].shape == (B, L) and int(g["unmask_step"].max()) <= S
    assert ((g["token"] == MASK) == (g["unmask_step"] == S)).all()
    rows = int(g["keep_rows"])
    for k, s in enumerate(g["keep_steps"]):
        g5 = np.concatenate([g["grad"][k], np.zeros((rows, L, 1), np.float32)], axis=2)
        assert np.array_equal(g["w"][k], (g["q"][k] + (scale * g5).astype(np.float32)).astype(np.float32)), int(s)
    assert int(g["n_negative"]) > 0 and 0.001 < int(g["n_changed"]) / int(g["n_masked_draws"]) < 0.1


def test_classifier_propose_rejects_bad_arguments():
    """svdd_classifier_propose returns E_ARG before touching the device."""
    from svdd_amd import _lib
    L_ = _lib.lib()
    ph = _lib.SvddRng(_lib.RNG_PHILOX, 0, None, 0, 0, 0, 0)
    one = ctypes.c_void_p(16)
    f = L_.svdd_classifier_propose

    def call(logits=one, layout=0, x=one, grad=one, B=2, L=3, rng=ph, x_next=one):
        return f(logits, layout, x, grad, 0.5, 0.5, 1.0, B, L, ctypes.byref(rng) if rng is not None else None, x_next, None, None, None)

    assert call(logits=None) == _lib.E_ARG
    assert call(x=None) == _lib.E_ARG
    assert call(grad=None) == _lib.E_ARG
    assert call(x_next=None) == _lib.E_ARG
    assert call(rng=None) == _lib.E_ARG
    assert call(B=0) == _lib.E_ARG and call(L=-1) == _lib.E_ARG
    assert call(layout=2) == _lib.E_ARG
    assert call(rng=_lib.SvddRng(7, 0, None, 0, 0, 0, 0)) == _lib.E_ARG                                   # unknown RNG kind
    assert call(rng=_lib.SvddRng(_lib.RNG_REPLAY, 0, None, 0, 0, 0, 0)) == _lib.E_ARG                     # replay without uniforms
    assert call(rng=_lib.SvddRng(_lib.RNG_REPLAY, 0, 16, 0, 0, 5, 0)) == _lib.E_ARG                       # bad uniforms layout
    assert call(rng=_lib.SvddRng(_lib.RNG_REPLAY, 0, 16, 0, 3, 0, 4)) == _lib.E_ARG                       # rows 3..4 of a 4-row batch
    assert call(B=1 << 20, L=1 << 10) == _lib.E_ARG                                                       # B L 5 >= 2^31


def test_api_surface():
    """The reference's parameter lists (diffusion_gosai.py:1064, 1332, 1362; Enformer.py:639)."""
    from svdd_amd.config import dna_config
    from svdd_amd.diffusion import Diffusion
    from svdd_amd.harness import BaseModel
    d = Diffusion(dna_config(hidden_dim=16, num_cnn_stacks=1))
    want = {
        "controlled_sample_classfier": ["pre_scorer_embedding", "pre_scorer_head", "num_steps", "eps", "eval_sp_size", "guidance_scale"],
        "controlled_sample_classifier": ["pre_scorer_embedding", "pre_scorer_head", "num_steps", "eps", "eval_sp_size", "guidance_scale"],
        "_ddpm_update_finetune_classfier": ["x", "t", "dt", "pre_scorer_embedding", "pre_scorer_head", "guidance_scale"],
        "compute_gradient": ["x", "pre_scorer_embedding", "pre_scorer_head"],
    }
    for name, params in want.items():
        assert list(inspect.signature(getattr(d, name)).parameters) == params, name
    sig = inspect.signature(d.controlled_sample_classfier).parameters
    assert sig["guidance_scale"].default is None and sig["eps"].default == 1e-5 and sig["num_steps"].default is None
    sig = inspect.signature(BaseModel.controlled_decode_classfier).parameters
    assert list(sig) == ["self", "gen_batch_num", "guidance_scale", "sample_M"] and sig["sample_M"].default == 10


def test_guidance_scale_none_and_cpu_and_sharded_are_refused():
    from svdd_amd import ops, synthetic
    model, emb, head, _ = synthetic.build("rna", "cpu", hidden_dim=16, num_cnn_stacks=1, value_channels=8, n_conv=1)
    with pytest.raises(ValueError, match="guidance_scale"):
        model.controlled_sample_classfier(emb, head, eval_sp_size=2)
    with pytest.raises(ValueError, match="guidance_scale"):
        model._ddpm_update_finetune_classfier(torch.full((2, 50), 4), torch.ones(2, 1), 0.01, emb, head, None)
    with pytest.raises(ops.SvddError):
        model.controlled_sample_classfier(emb, head, num_steps=2, eval_sp_size=2, guidance_scale=1.0)
    model._shard = (0, 2, 4, 2)
    try:
        with pytest.raises(NotImplementedError):
            model.controlled_sample_classfier(emb, head, num_steps=2, eval_sp_size=2, guidance_scale=1.0)
    finally:
        model._shard = None


def test_cli_parser_classfier():
    from svdd_amd import cli
    a = cli.build_parser("classfier").parse_args([])
    assert a.method == "classfier" and cli._guidance_scale(a) == 1.5
    a = cli.build_parser().parse_args(["--method", "classfier"])
    assert cli._guidance_scale(a) == 1.5
    a = cli.build_parser("classfier").parse_args(["--guidance_scale", "3"])
    assert cli._guidance_scale(a) == 3.0
    assert cli._guidance_scale(cli.build_parser("dps").parse_args([])) == 1e5                            # DPS keeps its default
    assert cli.SUFFIX["classfier"] == "-classfier"                                                       # decode_classfier.py:119
