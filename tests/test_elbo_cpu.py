"""CPU checks of the ELBO scoring path against the reference's own _loss runs (tests/golden/g30_elbo_tiny.npz, g31_elbo_full.npz,
recorded by tests/golden/make_golden_elbo.py):

  * the host half of replay mode: Diffusion._elbo_scalars turns the replayed torch.rand(n) into the reference's t, move_chance and w
    bit for bit (move_chance and w: the reference's torch ops on the host that runs the test, tests/elbo_ref.check_replayed_draw),
    and the masking rule on the replayed torch.rand(n, L) gives its xt;
  * the float64 restatement (tests/elbo_ref.py) on the engine's backbone run in float64 reproduces the recorded nlls and loss;
  * the LogLinear identity w = 1 / t; the numpy Philox against its published known-answer vector;
  * --eval_nll parsing."""
import numpy as np
import pytest
import torch

from tests import elbo_ref

CASES = [("g30_elbo_tiny.npz", "rand"), ("g30_elbo_tiny.npz", "short"), ("g31_elbo_full.npz", "dna_rand"),
         ("g31_elbo_full.npz", "dna_dec"), ("g31_elbo_full.npz", "rna_rand")]


def case(golden, name, c):
    g = golden(name)
    return {k[len(c) + 1:]: v for k, v in g.items() if k.startswith(c + "_")}


def cpu_model(golden, name, L):
    if name.startswith("g30"):
        from tests import e2e_parity
        return e2e_parity.tiny_engine(golden("nets_tiny.npz"), L, 8, "cpu")[0]
    from svdd_amd import synthetic
    return synthetic.build("dna" if L == 200 else "rna", "cpu")[0]


@pytest.mark.parametrize("name,c", CASES)
def test_replay_host_half_is_bit_exact(golden, name, c):
    from svdd_amd.config import Config
    from svdd_amd.diffusion import Diffusion
    r = case(golden, name, c)
    d = Diffusion(Config())
    B, L = r["x0"].shape
    torch.manual_seed(int(r["seed"]))
    for call in range(2):
        e = torch.rand(B)
        t, sigma, dsigma, mc, w = d._elbo_scalars(e)
        u = torch.rand(B, L)
        assert all(v.dtype == torch.float32 for v in (t, sigma, dsigma, mc, w))
        assert np.array_equal(dsigma.numpy().view(np.uint32), r["dsigma"][call].view(np.uint32))      # fp32 arithmetic only
        elbo_ref.check_replayed_draw(r, call, e.numpy(), u.numpy(), t.numpy(), mc.numpy().reshape(-1), w.numpy(),
                                     elbo_ref.mask(r["x0"], u.numpy(), mc.numpy()))
    assert np.array_equal(torch.rand(2).numpy(), r["next2"])


@pytest.mark.parametrize("name,c", CASES)
def test_float64_restatement_reproduces_the_recorded_loss(golden, name, c):
    """Steps 1-5 in float64 on logits of the engine's backbone module run in float64 on the recorded xt: within a float64-vs-fp32
    bar of the reference's fp32 CPU run (measured: 3.8e-7 of the largest token loss, 1.1e-7 relative on the loss; bars 1.5e-6, 4e-7)."""
    r = case(golden, name, c)
    B, L = r["x0"].shape
    model = cpu_model(golden, name, L).double()
    torch.manual_seed(int(r["seed"]))
    for call in range(2):
        t, sigma, dsigma, mc, w = elbo_ref.scalars64(torch.rand(B).numpy())
        xt = elbo_ref.mask(r["x0"], torch.rand(B, L).numpy(), mc)
        assert np.array_equal(xt, r["xt"][call])
        with torch.no_grad():
            logits = model.backbone(torch.from_numpy(xt).long(), torch.zeros(B, dtype=torch.float64)).numpy()
        nll = elbo_ref.token_nll64(logits, xt, r["x0"], w)
        ref = r["nlls"][call].astype(np.float64)
        assert np.array_equal(nll == 0, ref == 0)                          # unmasked positions: exactly 0 on both sides
        scale = np.abs(ref).max()
        assert np.abs(nll - ref).max() <= 1.5e-6 * scale, np.abs(nll - ref).max() / scale
        assert abs(elbo_ref.loss64(nll) - float(r["loss"][call])) <= 4e-7 * abs(float(r["loss"][call]))


def test_loglinear_weight_is_one_over_t(golden):
    """dsigma / expm1(sigma) = (1 - eps) / (1 - (1 - eps) t) / ((1 - eps) t / (1 - (1 - eps) t)) = 1 / t: the recorded fp32 w
    against fp32(1 / t) (measured: 1.98 ulp of 1; bar 4), and the float64 restatement to 1e-12."""
    for name, c in CASES:
        r = case(golden, name, c)
        t, w = r["t"].astype(np.float64), r["w"].astype(np.float64)
        assert np.all(np.abs(w * t - 1.0) <= 4 * 2.0 ** -23), (name, c, np.abs(w * t - 1).max())
        t64, _, _, _, w64 = elbo_ref.scalars64(np.random.default_rng(0).random(64))
        assert np.allclose(w64 * t64, 1.0, rtol=0, atol=1e-12)


def test_philox_known_answer():
    """Random123's published Philox4x32-10 known-answer vectors (ctr, key) -> output."""
    out = elbo_ref.philox4x32_10(*([np.uint32(0)] * 4), 0, 0)
    assert [int(v) for v in out] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    out = elbo_ref.philox4x32_10(*([np.uint32(0xFFFFFFFF)] * 4), 0xFFFFFFFF, 0xFFFFFFFF)
    assert [int(v) for v in out] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]


def test_philox_elbo_strata_and_identities():
    n, L, K = 5, 13, 8
    t, mc, w, u = elbo_ref.philox_elbo(77, 3, n, L, K)
    lo = 1e-3 + (1 - 1e-3) * np.repeat(np.arange(K), n) / K
    assert np.all(t >= lo.astype(np.float32)) and np.all(t <= (lo + (1 - 1e-3) / K).astype(np.float32))
    assert u.shape == (n * K, L) and np.all((u >= 0) & (u < 1))
    assert np.allclose(mc, (1 - 1e-3) * t, rtol=1e-7) and np.allclose(w * t, 1.0, rtol=3e-7)


def test_eval_nll_flag_parsing():
    from svdd_amd import cli
    for method in cli.SUFFIX:
        base = cli.build_parser(method).parse_args([])
        assert base.eval_nll == 0
        on = cli.build_parser(method).parse_args(["--eval_nll", "4"])
        assert on.eval_nll == 4
        assert {k: v for k, v in vars(on).items() if k != "eval_nll"} == {k: v for k, v in vars(base).items() if k != "eval_nll"}
    assert sorted(vars(cli.build_parser("mc").parse_args([]))) == sorted(
        ["task", "reward_name", "batch_size", "sample_M", "val_batch_num", "seed", "method", "tweedie", "alpha", "guidance_scale",
         "model", "precision", "rng", "diffusion_ckpt", "load_checkpoint_path", "reward_ckpt", "out_dir", "presample", "eval_nll"])
