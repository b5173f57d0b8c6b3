"""-m gpu: classifier guidance (reference diffusion_gosai.py:1064-1104, 1332-1371; Enformer.py:639-716; decode_classfier.py).

  * svdd_classifier_propose against the numpy restatement of the guided step (tests/test_classifier_cpu.py: guided_step), exactly:
    both logits layouts, signed weights, replay and Philox uniforms, a position count that is not a multiple of the block;
  * the reference's own runs g27 (tiny nets) / g28 (full-size nets), teacher-forced and free-running, and g29 at the C2 shape
    (B = 256, L = 200, 128 steps) on the fused gradient path;
  * zero guidance = the un-guided decode; fused vs autograd gradient; the harness, the CLI and an Enformer-shaped value net."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import svdd_oracle as orc
from tests.test_classifier_cpu import guided_step

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _bvl_u(u_logical):
    """A logical [B, L, 5] uniforms array -> the replay block [1, B, 5, L] (the reference's rand_like order)."""
    return dev(np.ascontiguousarray(np.swapaxes(u_logical, 1, 2))[None])


@pytest.fixture(scope="module")
def full_nets():
    from svdd_amd import synthetic
    return synthetic.build("dna", DEV)


def _philox_u(seed, row_offset, step, B, L):
    u = np.empty((B, L, 5), np.float32)
    for b in range(B):
        for l in range(L):
            u[b, l] = orc.philox_uniform5(seed, (row_offset + b) * L + l, step, 0)
    return u


# ------------------------------------------------------------------------------------------ the kernel alone
@pytest.mark.parametrize("layout", ["blv", "bvl"])
@pytest.mark.parametrize("rng", ["replay_bvl", "replay_blv", "philox"])
def test_kernel_equals_restatement(layout, rng):
    from svdd_amd import ops
    gen = np.random.default_rng(5 + len(layout) + len(rng))
    B, L = 7, 53                                                    # 371 positions: not a multiple of the 256-thread block
    dm, mcs, scale, seed, step, row_offset = 0.0078125, 0.61, 3.0, 12345, 17, 5
    logits = (gen.standard_normal((B, L, 5)) * 2.0).astype(np.float32)
    x = np.where(gen.random((B, L)) < 0.6, 4, gen.integers(0, 4, (B, L))).astype(np.uint8)
    x[0] = 4                                                        # an all-MASK row
    grad = (gen.standard_normal((B, L, 4)) * 0.01).astype(np.float32)   # scale * g ~ 0.03 >> q ~ 0.002: many negative weights
    lg = dev(logits) if layout == "blv" else dev(np.ascontiguousarray(np.swapaxes(logits, 1, 2))).transpose(1, 2)
    if rng == "philox":
        u = _philox_u(seed, row_offset, step, B, L)
        r = ops.Rng(seed=seed, row_offset=row_offset, step=step)
    else:
        u = gen.random((B, L, 5)).astype(np.float32)
        if rng == "replay_bvl":
            r = ops.Rng(uniforms=_bvl_u(u), uniforms_layout=ops.LAYOUT_BVL)
        else:
            r = ops.Rng(uniforms=dev(u[None]), uniforms_layout=ops.LAYOUT_BLV)
    x_next, onehot, q = ops.classifier_propose(lg, dev(x), dev(grad), dm, mcs, scale, r, want_q=True)
    torch.cuda.synchronize()
    want_x, want_q, want_w = guided_step(logits, x, grad, dm, mcs, scale, u)
    assert int((want_w[x == 4] < 0).sum()) > 50                     # the signed draw is exercised
    assert np.array_equal(x_next.cpu().numpy(), want_x)
    assert np.array_equal(onehot.cpu().numpy(), orc.transform_samples(want_x))
    assert q.stride() == lg.stride() and np.array_equal(q.cpu().numpy(), want_q)


def test_kernel_zero_scale_is_the_unguided_propose_philox():
    """Philox: the counters of svdd_propose with M = 1, so scale 0 draws what the un-guided K1 draws."""
    from svdd_amd import ops
    gen = np.random.default_rng(3)
    B, L = 64, 200
    logits = dev((gen.standard_normal((B, L, 5)) * 2.0).astype(np.float32))
    x = dev(np.where(gen.random((B, L)) < 0.7, 4, gen.integers(0, 4, (B, L))).astype(np.uint8))
    grad = dev((gen.standard_normal((B, L, 4))).astype(np.float32))
    r = ops.Rng(seed=99, row_offset=3, step=40)
    mine, _, _ = ops.classifier_propose(logits, x, grad, 0.01, 0.5, 0.0, r)
    cand, _, _ = ops.propose(logits, x, 0.01, 0.5, 1, r)
    assert torch.equal(mine, cand[:, 0])


# ------------------------------------------------------------------------------------------ the reference's runs, g27 / g28
def _engine(golden, name, full_nets):
    g = golden(name)
    if "full" in name:
        model, emb, head, _ = full_nets
        for nm, mod in (("backbone", model.backbone), ("embedding", emb), ("head", head)):
            sums = np.array([float(p.double().sum()) for p in mod.state_dict().values()])
            assert np.allclose(sums, g[nm + "_param_sums"], rtol=0, atol=1e-6), nm
        return g, model, emb, head
    from tests import e2e_parity
    return (g,) + e2e_parity.tiny_engine(golden("nets_tiny.npz"), int(g["L"]), int(g["S"]), DEV)


# measured on one MI355X: 5.5e-7 (g27, autograd) and 8.4e-7 (g28, fused) of the gradient's largest entry
@pytest.mark.parametrize("name,fused,grad_tol", [("g27_traj_classifier.npz", False, 3e-6), ("g28_traj_classifier_full.npz", True, 3e-6)])
def test_reference_run_teacher_forced_and_free_running(golden, full_nets, name, fused, grad_tol):
    """Per recorded step: the engine's gradient (g27: autograd on the GPU — the tiny net is below the kernels' shapes; g28: the fused
    gradient pass) within grad_tol of the reference's, relative to its largest entry; the kernel with the RECORDED gradient and the
    engine's logits draws the reference's next state exactly. Then the free-running decode (replay RNG) gives the reference's x_0."""
    from svdd_amd import ops
    g, model, emb, head = _engine(golden, name, full_nets)
    S, B, L, scale = int(g["S"]), int(g["B"]), int(g["L"]), float(g["scale"])
    sched = model._schedule(S, 1e-5)[0]
    worst = 0.0
    for i in range(S):
        x = dev(g["xs"][i])
        grad, was_fused = model._classifier_grad(ops.transform_samples(x), emb, head)
        assert was_fused == fused
        worst = max(worst, float(np.abs(grad.cpu().numpy() - g["grad"][i]).max() / np.abs(g["grad"][i]).max()))
        with torch.no_grad():
            logits = model._backbone_logits(x)
        x_next, _, _ = ops.classifier_propose(logits, x, dev(g["grad"][i]), sched[i, 2], sched[i, 1], scale,
                                              ops.Rng(uniforms=_bvl_u(g["u"][i]), uniforms_layout=ops.LAYOUT_BVL))
        assert np.array_equal(x_next.cpu().numpy(), g["x_next"][i]), f"step {i}"
    print(name, "gradient: max |g - g_ref| / max |g_ref| =", worst)
    assert worst <= grad_tol, worst
    keep = model.rng_mode
    model.rng_mode = "replay"
    try:
        torch.manual_seed(int(g["seed"]))
        x0 = model.controlled_sample_classfier(emb, head, num_steps=S, eval_sp_size=B, guidance_scale=scale)
    finally:
        model.rng_mode = keep
    assert model._classifier_fused_last == fused
    assert np.array_equal(x0.cpu().numpy(), g["x0"])


# ------------------------------------------------------------------------------------------ g29: the C2 shape
def test_c2_shape_against_the_reference_run(golden, full_nets):
    """g29: B = 256, L = 200, 128 steps, guidance scale 256, full-size nets, as the reference ran it — on the FUSED gradient path.
    Teacher-forced on all 128 recorded states (the uniforms replayed from torch's mt19937 stream, one rand_like per step): next states
    identical on all but <= 2 of the 127 x 256 row-steps (a near-tie of the race may flip with the gradient's fp32 summation order),
    x_0 rows >= B - 1 teacher-forced and >= B - 2 free-running (the criteria of g26)."""
    from svdd_amd import ops
    g = golden("g29_traj_classifier_c2.npz")
    S, B, L, scale = int(g["S"]), int(g["B"]), int(g["L"]), float(g["scale"])
    model, emb, head, _ = full_nets
    for nm, mod in (("backbone", model.backbone), ("embedding", emb), ("head", head)):
        sums = np.array([float(p.double().sum()) for p in mod.state_dict().values()])
        assert np.allclose(sums, g[nm + "_param_sums"], rtol=0, atol=1e-6), nm
    unmask, token = g["unmask_step"], g["token"]
    xs = [np.where(unmask < s, token, 4).astype(np.uint8) for s in range(S + 1)]
    kept = {int(s): k for k, s in enumerate(g["keep_steps"])}
    nr = int(g["keep_rows"])
    sched = model._schedule(S, 1e-5)[0]
    keep_mode = model.rng_mode
    model.rng_mode = "replay"
    rows_same, worst_g = 0, 0.0
    try:
        torch.manual_seed(int(g["seed"]))
        for i in range(S):
            x = dev(xs[i])
            with torch.no_grad():
                logits = model._prior_logits(x) if i == 0 else model._backbone_logits(x)
            grad, fused = model._classifier_grad(ops.transform_samples(x), emb, head)
            assert fused
            x_next, _, q = ops.classifier_propose(logits, x, grad, sched[i, 2], sched[i, 1], scale, model._rng(i, 1, B, L, logits),
                                                  want_q=True)
            if i in kept:
                ref = g["grad"][kept[i]]
                worst_g = max(worst_g, float(np.abs(grad[:nr].cpu().numpy() - ref).max() / np.abs(ref).max()))
                assert np.allclose(q[:nr].cpu().numpy(), g["q"][kept[i]], rtol=1e-4, atol=1e-8), i
            if i + 1 < S:
                rows_same += int((x_next.cpu().numpy() == xs[i + 1]).all(axis=1).sum())
            else:
                x_last = x_next
        x0_tf = model._noise_removal(x_last).cpu().numpy()
        torch.manual_seed(int(g["seed"]))
        x0 = model.controlled_sample_classfier(emb, head, num_steps=S, eval_sp_size=B, guidance_scale=scale).cpu().numpy()
        assert model._classifier_fused_last
    finally:
        model.rng_mode = keep_mode
    tf_rows, free_rows = int((x0_tf == g["x0"]).all(axis=1).sum()), int((x0 == g["x0"]).all(axis=1).sum())
    print("g29 classifier c2: gradient rel err", worst_g, "next states identical", rows_same, "of", (S - 1) * B,
          "x0 rows (teacher-forced)", tf_rows, "x0 rows (free-running)", free_rows)
    # measured on one MI355X: gradient 9.0e-7, all 32,512 next states identical, x_0 256 / 256 rows both ways
    assert worst_g <= 3e-6, worst_g
    assert rows_same >= (S - 1) * B - 2, rows_same
    assert tf_rows >= B - 1 and free_rows >= B - 2, (tf_rows, free_rows)


# ------------------------------------------------------------------------------------------ engine properties
@pytest.mark.parametrize("mode", ["replay", "philox"])
def test_zero_guidance_is_the_unguided_decode(full_nets, mode):
    model, emb, head, _ = full_nets
    keep = model.rng_mode, model.philox_seed
    model.rng_mode, model.philox_seed = mode, 77
    try:
        torch.manual_seed(5)
        a = model.decode_sample(num_steps=24, eval_sp_size=16)
        torch.manual_seed(5)
        b = model.controlled_sample_classfier(emb, head, num_steps=24, eval_sp_size=16, guidance_scale=0.0)
        after = torch.rand(3)
        torch.manual_seed(5)
        model.decode_sample(num_steps=24, eval_sp_size=16)
        assert torch.equal(after, torch.rand(3))                  # the same amount of torch's stream was consumed (replay)
    finally:
        model.rng_mode, model.philox_seed = keep
    assert torch.equal(a, b)


def test_fused_and_autograd_gradients_agree(full_nets):
    """fuse_nets=False: the backbone as PyTorch modules and the gradient through torch autograd (MIOpen GRU) — same function."""
    model, emb, head, _ = full_nets
    B, S, scale = 32, 32, 32.0
    gen = np.random.default_rng(1)
    x = dev(np.where(gen.random((B, 200)) < 0.5, 4, gen.integers(0, 4, (B, 200))).astype(np.uint8))
    from svdd_amd import ops
    oh = ops.transform_samples(x)
    g_f, fused = model._classifier_grad(oh, emb, head)
    assert fused
    keep = model.rng_mode, model.philox_seed
    model.rng_mode, model.philox_seed = "philox", 4
    try:
        x0_f = model.controlled_sample_classfier(emb, head, num_steps=S, eval_sp_size=B, guidance_scale=scale)
        model.fuse_nets = False
        g_a, fused = model._classifier_grad(oh, emb, head)
        assert not fused
        x0_a = model.controlled_sample_classfier(emb, head, num_steps=S, eval_sp_size=B, guidance_scale=scale)
        assert not model._classifier_fused_last
    finally:
        model.fuse_nets = True
        model.rng_mode, model.philox_seed = keep
    err = float((g_f - g_a).abs().max() / g_a.abs().max())
    rows = int((x0_f == x0_a).all(dim=1).sum())
    print("fused vs autograd gradient rel err", err, "x0 rows equal", rows, "of", B)
    assert err <= 3e-6, err                                       # measured: 8.3e-7, 32 / 32 rows
    assert rows >= B - 2, rows


def test_per_step_api_returns_the_reference_tuple(full_nets):
    model, emb, head, _ = full_nets
    B, L = 4, 200
    x = torch.full((B, L), 4, dtype=torch.int64, device=DEV)
    x[:, :50] = 2
    t = torch.full((B, 1), 0.5, device=DEV)
    x_next, x_in, q, copy_flag = model._ddpm_update_finetune_classfier(x, t, 1 / 128, emb, head, 100.0)
    assert x_next.dtype == torch.int64 and x_next.shape == (B, L) and x_in is x
    assert q.shape == (B, L, 5) and torch.equal(copy_flag, (x != 4).long())
    assert torch.equal(x_next[:, :50], x[:, :50]) and int(x_next.max()) <= 4
    mct, mcs, dm = model._step_scalars(t, 1 / 128)
    assert torch.all(q[:, 50:, 4] == np.float32(mcs)) and torch.allclose(q[:, 50:, :4].sum(-1), torch.tensor(dm, device=DEV), rtol=1e-5)


# ------------------------------------------------------------------------------------------ harness, CLI, other value nets
def _small(task, steps):
    from svdd_amd import synthetic
    from svdd_amd.config import SamplingConfig
    m = synthetic.build(task, DEV)
    m[0].config.sampling = SamplingConfig(steps=steps)
    return m


def test_harness_order_and_shapes():
    """controlled_decode_classfier keeps the reference's order — the guided batches, then gen_batch_num * sample_M baseline batches —
    and returns its 5-tuple; in Philox mode guided batch k is keyed batch_seed(base, k)."""
    from svdd_amd.harness import BaseModel, batch_seed
    model, emb, head, reward = _small("rna", 6)
    G, M, B, scale = 2, 2, 4, 1.5
    bm = BaseModel(emb, head, model, reward, B)
    torch.manual_seed(3)
    samples, vf, rm, topk, base = bm.controlled_decode_classfier(G, scale, sample_M=M)
    assert isinstance(samples, list) and len(samples) == G and samples[0].shape == (B, 50)
    assert vf.shape == (G * B,) and rm.shape == (G * B,) and topk.shape == (G * B,) and base.shape == (G * B,)
    torch.manual_seed(3)
    want = [model.controlled_sample_classfier(emb, head, eval_sp_size=B, guidance_scale=scale) for _ in range(G)]
    baseline = [model.decode_sample(eval_sp_size=B) for _ in range(G * M)]
    for a, b in zip(samples, want):
        assert torch.equal(a, b)
    with torch.no_grad():
        preds = [bm._reward(b).reshape(-1) for b in baseline]
    assert torch.equal(base, torch.cat(preds[:G]))
    assert torch.equal(topk, torch.topk(torch.cat(preds), G * B).values)
    model.rng_mode, model.philox_seed = "philox", 11
    try:
        s2 = bm.controlled_decode_classfier(1, scale, sample_M=1)[0]
        model.philox_seed = batch_seed(11, 0)
        one = model.controlled_sample_classfier(emb, head, eval_sp_size=B, guidance_scale=scale)
    finally:
        model.rng_mode, model.philox_seed = "replay", 0
    assert torch.equal(s2[0], one)


def test_cli_decode_classfier_writes_reference_npz(tmp_path):
    """decode_classfier.py (reference :108-119) in a child process: ./log/dna-HepG2-classfier.npz with decoding / baseline."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "decode_classfier.py"), "--batch_size", "8", "--val_batch_num", "1",
                        "--sample_M", "2"], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    z = np.load(tmp_path / "log" / "dna-HepG2-classfier.npz")
    assert set(z.files) == {"decoding", "baseline"} and z["decoding"].shape == (8,) and z["baseline"].shape == (8,)
    assert np.isfinite(z["decoding"]).all() and np.isfinite(z["baseline"]).all()


def test_enformer_shaped_value_net_takes_the_autograd_path():
    from svdd_amd.enformer_value import EnformerTrunk
    from svdd_amd.value_nets import ConvHead
    model, _, _, _ = _small("dna", 4)
    torch.manual_seed(2)
    emb = EnformerTrunk(n_conv=4, channels=384, n_transformers=1, n_heads=2, key_len=16).to(DEV).eval()
    head = ConvHead(1, 768).to(DEV).eval()
    x0 = model.controlled_sample_classfier(emb, head, eval_sp_size=3, guidance_scale=50.0)
    assert model._classifier_fused_last is False
    assert x0.shape == (3, 200) and x0.dtype == torch.int64 and int(x0.min()) >= 0 and int(x0.max()) <= 3
