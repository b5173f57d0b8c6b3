"""-m gpu: ELBO scoring of clean sequences (reference diffusion_gosai.py:1660-1669, 738-749, 1709-1779; svdd_elbo_mask /
svdd_elbo_nll, ABI 13).

  * replay: the reference's own _loss runs (g30 tiny nets, g31 full-size nets at L = 200 and 50): t, move_chance, w and xt bit for bit,
    the zero pattern of nlls, masked nlls and loss within a bar, the generator's end state, two consecutive calls;
  * the kernels through the C ABI into sentinel-filled buffers: svdd_elbo_nll against svdd_subs_logp restated, both layouts; the
    Philox draws of svdd_elbo_mask against the numpy restatement (tests/elbo_ref.py);
  * Philox invariance under row_offset splits and chunk_rows, strata, the masked fraction; f16x3 against fp32; the DiT backbone;
  * the harness, the CLI and the refused configurations."""
import ctypes

import numpy as np
import pytest
import torch

from tests import elbo_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 0x5A                                               # sentinel byte: fp32 0x5A5A5A5A, fp64 likewise, never a kernel result


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def case(golden, name, c):
    g = golden(name)
    return {k[len(c) + 1:]: v for k, v in g.items() if k.startswith(c + "_")}


@pytest.fixture(scope="module")
def nets():
    from svdd_amd import synthetic
    from tests.conftest import load_golden
    from tests import e2e_parity
    out = {200: synthetic.build("dna", DEV)[0], 50: synthetic.build("rna", DEV)[0]}
    out["tiny"] = e2e_parity.tiny_engine(load_golden("nets_tiny.npz"), 50, 8, DEV)[0]
    return out


def model_for(nets, name, L):
    m = nets["tiny"] if name.startswith("g30") else nets[L]
    m.rng_mode, m.precision, m.elbo_trace, m.row_offset = "replay", "f32", None, 0
    return m


# ------------------------------------------------------------------------------------------ replay: the reference's runs
# t, move_chance, w and xt: tests/elbo_ref.check_replayed_draw (bit for bit on the host that runs the test; the recording host's torch
# exp rounds one ulp differently on some inputs). Measured on one MI355X (masked token losses relative to the row's largest; loss
# relative): g30 tiny nets 3.2e-7 / 9.6e-8, g31 full-size fp32 kernels 1.5e-6 / 9.5e-8; bars 5e-6 / 3e-7
@pytest.mark.parametrize("name,c", [("g30_elbo_tiny.npz", "rand"), ("g30_elbo_tiny.npz", "short"), ("g31_elbo_full.npz", "dna_rand"),
                                    ("g31_elbo_full.npz", "dna_dec"), ("g31_elbo_full.npz", "rna_rand")])
def test_replay_reproduces_the_reference_loss(golden, nets, name, c):
    r = case(golden, name, c)
    B, L = r["x0"].shape
    m = model_for(nets, name, L)
    x0 = dev(r["x0"].astype(np.int64))
    mask = torch.ones(B, L, device=DEV)
    torch.manual_seed(int(r["seed"]))
    one = m._loss(x0, mask)
    assert np.array_equal(torch.rand(2).numpy(), r["next1"])                   # the generator is where the reference left it
    torch.manual_seed(int(r["seed"]))
    m.elbo_trace = []
    outs = [m._loss(x0, mask), m._loss(x0, mask)]
    trace, m.elbo_trace = m.elbo_trace, None
    assert np.array_equal(torch.rand(2).numpy(), r["next2"])
    assert torch.equal(one.nlls, outs[0].nlls)
    torch.manual_seed(int(r["seed"]))
    draws = [(torch.rand(B).numpy(), torch.rand(B, L).numpy()) for _ in range(2)]     # the replayed stream, for the mask rule
    for call, (out, tr) in enumerate(zip(outs, trace)):
        elbo_ref.check_replayed_draw(r, call, *draws[call], tr["t"].numpy(), tr["move_chance"].numpy().reshape(-1), tr["w"].numpy(),
                                     tr["xt"].cpu().numpy())
        nlls, ref = out.nlls.cpu().numpy().astype(np.float64), r["nlls"][call].astype(np.float64)
        assert out.nlls.dtype == torch.float32 and out.token_mask is mask
        assert np.array_equal(nlls == 0, ref == 0)
        assert np.all(nlls >= 0)                                              # unmasked positions are +0 (the reference: -0.0)
        rowmax = np.abs(ref).max(1, keepdims=True)
        err = (np.abs(nlls - ref) / np.maximum(rowmax, 1e-30)).max()
        assert err <= 5e-6, err
        assert abs(float(out.loss) - float(r["loss"][call])) <= 3e-7 * abs(float(r["loss"][call]))


def test_sequence_nll_replay_is_consecutive_forward_passes(golden, nets):
    """sequence_nll(n_draws = 2) in replay mode = the mean of the row sums of two consecutive _forward_pass_diffusion calls."""
    r = case(golden, "g31_elbo_full.npz", "rna_rand")
    m = model_for(nets, "g31", 50)
    x0 = dev(r["x0"].astype(np.int64))
    torch.manual_seed(int(r["seed"]))
    seq = m.sequence_nll(x0, n_draws=2, chunk_rows=24)
    assert np.array_equal(torch.rand(2).numpy(), r["next2"])
    torch.manual_seed(int(r["seed"]))
    a, b = (m._forward_pass_diffusion(x0).double().cpu().numpy() for _ in range(2))
    sa, sb = np.cumsum(a, axis=1)[:, -1], np.cumsum(b, axis=1)[:, -1]
    assert seq.dtype == torch.float64 and np.array_equal(seq.cpu().numpy(), (sa + sb) / 2)


# ------------------------------------------------------------------------------------------ the kernels alone (C ABI, sentinels)
def _guarded(shape, dtype, guard):
    """A buffer of `shape` with `guard` rows of sentinel bytes before and after -> (whole, interior view)."""
    rows, rest = shape[0], tuple(shape[1:])
    whole = torch.empty((rows + 2 * guard,) + rest, dtype=dtype, device=DEV)
    whole.view(torch.uint8).fill_(SENT)
    return whole, whole[guard:guard + rows]


def _untouched(whole, guard):
    head, tail = whole[:guard], whole[whole.shape[0] - guard:]
    return bool((head.contiguous().view(torch.uint8) == SENT).all()) and bool((tail.contiguous().view(torch.uint8) == SENT).all())


@pytest.mark.parametrize("layout", ["blv", "bvl"])
def test_nll_kernel_equals_subs_logp_restated(layout):
    from svdd_amd import _lib, ops
    gen = np.random.default_rng(11 + len(layout))
    n, L, K, G = 13, 71, 3, 2                                          # 71 positions: not a multiple of the wave
    R = n * K
    logits = (gen.standard_normal((R, L, 5)) * 3.0).astype(np.float32)
    x0 = gen.integers(0, 4, (n, L)).astype(np.uint8)
    xt = np.where(gen.random((R, L)) < 0.55, 4, np.tile(x0, (K, 1))).astype(np.uint8)
    xt[0] = 4                                                          # an all-MASK row
    xt[1] = x0[1]                                                      # an all-clean row
    w = (1.0 / (gen.random(R) * 0.999 + 1e-3)).astype(np.float32)
    lg = dev(logits) if layout == "blv" else dev(np.ascontiguousarray(np.swapaxes(logits, 1, 2))).transpose(1, 2)
    lg_c, lay = ops.layout_of(lg)
    lp = ops.subs_logp(lg, dev(xt)).cpu().numpy()
    want = np.where(xt == 4, (-np.take_along_axis(lp, x0.astype(np.int64)[np.arange(R) % n][..., None], -1)[..., 0]) * w[:, None],
                    np.float32(0.0)).astype(np.float32)
    nll_w, nll = _guarded((R, L), torch.float32, G)
    rs_w, rs = _guarded((R + 1,), torch.float64, G)                     # one extra row: nothing past R is written
    sm_w, sm = _guarded((n + 1,), torch.float64, G)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    x0_d, xt_d, w_d = dev(x0), dev(xt), dev(w)
    rc = _lib.lib().svdd_elbo_nll(lg_c.data_ptr(), lay, xt_d.data_ptr(), x0_d.data_ptr(), w_d.data_ptr(), n, L, K, nll.data_ptr(),
                                  rs.data_ptr(), sm.data_ptr(), err.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == _lib.OK
    torch.cuda.synchronize()
    got = nll.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))   # bit for bit, +0 at unmasked positions
    sums = np.cumsum(want.astype(np.float64), axis=1)[:, -1]            # position order in fp64
    assert np.array_equal(rs[:R].cpu().numpy(), sums)
    acc = sums[:n].copy()
    for k in range(1, K):
        acc = acc + sums[k * n:(k + 1) * n]
    assert np.array_equal(sm[:n].cpu().numpy(), acc / K)
    assert int(err[0]) == 0
    assert _untouched(nll_w, G) and _untouched(rs_w, G) and _untouched(sm_w, G)
    assert bool((rs[R:].contiguous().view(torch.uint8) == SENT).all()) and bool((sm[n:].contiguous().view(torch.uint8) == SENT).all())


@pytest.mark.parametrize("n,L,K,row_offset", [(37, 53, 3, 5), (4, 200, 32, (1 << 32) + 7)])
def test_philox_mask_equals_restatement(n, L, K, row_offset):
    from svdd_amd import _lib, ops
    seed = 0x1234_5678_9ABC_DEF0
    gen = np.random.default_rng(n)
    x0 = gen.integers(0, 4, (n, L)).astype(np.uint8)
    t_ref, mc_ref, w_ref, u = elbo_ref.philox_elbo(seed, row_offset, n, L, K)
    xt_ref = np.where(u < mc_ref[:, None], 4, np.tile(x0, (K, 1))).astype(np.uint8)
    G, R = 3, n * K
    xt_w, xt = _guarded((R, L), torch.uint8, G)
    outs = [_guarded((R,), dt, G) for dt in (torch.float32, torch.float32, torch.float32, torch.int32)]
    rs = ops.Rng(seed=seed, row_offset=row_offset).c_struct()
    x0_d = dev(x0)
    rc = _lib.lib().svdd_elbo_mask(x0_d.data_ptr(), n, L, K, 1e-3, ctypes.byref(rs), None, xt.data_ptr(),
                                   *(o[1].data_ptr() for o in outs), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == _lib.OK
    torch.cuda.synchronize()
    t, mc, w, cnt = (o[1].cpu().numpy() for o in outs)
    assert np.array_equal(t, t_ref) and np.array_equal(mc, mc_ref) and np.array_equal(w, w_ref)
    assert np.array_equal(xt.cpu().numpy(), xt_ref)
    assert np.array_equal(cnt, (xt_ref == 4).sum(1))
    assert _untouched(xt_w, G) and all(_untouched(o[0], G) for o in outs)


def test_replay_mask_kernel_and_refusals():
    from svdd_amd import _lib, ops
    gen = np.random.default_rng(3)
    n, L, K = 6, 33, 2
    x0 = gen.integers(0, 4, (n, L)).astype(np.uint8)
    u = gen.random((K * n, L)).astype(np.float32)
    mc = gen.random(K * n).astype(np.float32)
    xt, t, _, _, cnt = ops.elbo_mask(dev(x0), K, ops.Rng(uniforms=dev(u)), move_chance=dev(mc), want_count=True)
    want = np.where(u < mc[:, None], 4, np.tile(x0, (K, 1)))
    assert t is None and np.array_equal(xt.cpu().numpy(), want) and np.array_equal(cnt.cpu().numpy(), (want == 4).sum(1))
    L_ = _lib.lib()
    one = dev(np.zeros(64, np.uint8)).data_ptr()
    rs_rep, rs_phi = ops.Rng(uniforms=dev(u)).c_struct(), ops.Rng(seed=1).c_struct()
    assert L_.svdd_elbo_mask(one, n, L, K, 1e-3, ctypes.byref(rs_rep), None, one, None, None, None, None, None) == _lib.E_ARG
    assert L_.svdd_elbo_mask(one, n, L, K, 1e-3, ctypes.byref(rs_rep), one, one, one, None, None, None, None) == _lib.E_ARG
    assert L_.svdd_elbo_mask(one, n, L, K, 1e-3, ctypes.byref(rs_phi), one, one, None, None, None, None, None) == _lib.E_ARG
    assert L_.svdd_elbo_mask(one, n, L, 65536, 1e-3, ctypes.byref(rs_phi), None, one, None, None, None, None, None) == _lib.E_ARG
    assert L_.svdd_elbo_mask(one, n, L, K, 0.0, ctypes.byref(rs_phi), None, one, None, None, None, None, None) == _lib.E_ARG
    assert L_.svdd_elbo_nll(one, 2, one, one, one, n, L, K, None, one, None, None, None) == _lib.E_ARG          # layout
    assert L_.svdd_elbo_nll(one, 0, one, one, one, n, L, K, None, None, None, None, None) == _lib.E_ARG         # row_sum NULL
    # a token > 3 in x0 is refused: the device flag, raised as SVDD_E_ARG by the wrapper
    x_bad = x0.copy()
    x_bad[2, 5] = 4
    logits = dev(gen.standard_normal((K * n, L, 5)).astype(np.float32))
    with pytest.raises(ops.SvddError, match="token > 3"):
        ops.elbo_nll(logits, dev(np.full((K * n, L), 4, np.uint8)), dev(x_bad), dev(np.ones(K * n, np.float32)), K)


# ------------------------------------------------------------------------------------------ Philox through the public API
def test_philox_sequence_nll_invariance_strata_and_masked_fraction(nets):
    m = model_for(nets, "g31", 200)
    m.rng_mode, m.philox_seed = "philox", 2024
    gen = np.random.default_rng(8)
    B, K = 12, 4
    x0 = dev(gen.integers(0, 4, (B, 200)))
    full = m.sequence_nll(x0, n_draws=K)
    assert torch.equal(full, m.sequence_nll(x0, n_draws=K, chunk_rows=8))            # 2 sequences x 4 draws per launch
    m.row_offset = 5
    tail = m.sequence_nll(x0[5:], n_draws=K, chunk_rows=12)
    m.row_offset = 0
    assert torch.equal(full[5:], tail) and torch.equal(full[:5], m.sequence_nll(x0[:5], n_draws=K))
    assert bool(torch.isfinite(full).all()) and bool((full > 0).all())
    # one t per stratum of each sequence; the masked fraction against the mean move_chance over >= 1e5 positions
    from svdd_amd import ops
    n, L, K2 = 64, 200, 8
    xt, t, mc, w, cnt = ops.elbo_mask(dev(gen.integers(0, 4, (n, L)).astype(np.uint8)), K2, ops.Rng(seed=99), want_count=True)
    t = t.cpu().numpy().reshape(K2, n)
    lo = 1e-3 + (1 - 1e-3) * np.arange(K2)[:, None] / K2                  # draw k of every sequence in [lo_k, lo_k + (1 - eps) / K)
    assert np.all(t >= lo.astype(np.float32)) and np.all(t <= (lo + (1 - 1e-3) / K2).astype(np.float32))
    mc = mc.cpu().numpy().astype(np.float64)
    masked, expect = float(cnt.sum()), float(mc.sum() * L)
    sd = float(np.sqrt((mc * (1 - mc)).sum() * L))
    assert abs(masked - expect) <= 5 * sd, (masked, expect, sd)            # 5 sigma of the binomial sum (102,400 positions)
    assert int((xt == 4).sum()) == int(cnt.sum())


# measured on one MI355X: f16x3 sequence NLL within 1.2e-7 (relative) of fp32 at B = 16, L = 200, 2 draws; bar 4e-7
def test_precision_f16x3_agrees_with_f32(nets):
    m = model_for(nets, "g31", 200)
    m.rng_mode, m.philox_seed = "philox", 7
    x0 = dev(np.random.default_rng(9).integers(0, 4, (16, 200)))
    ref = m.sequence_nll(x0, n_draws=2)
    m.precision = "f16x3"
    try:
        lp = m.sequence_nll(x0, n_draws=2)
    finally:
        m.precision = "f32"
    rel = float(((lp - ref).abs() / ref.abs()).max())
    assert rel <= 4e-7, rel


def test_dit_backbone_matches_torch_restatement():
    """The DiT path (BLV logits from the SDPA module) against torch ops in the reference's order on the same xt (measured: 6.9e-8 of the largest token loss; bar 2e-7)."""
    from svdd_amd.config import dit_config
    from svdd_amd.diffusion import Diffusion
    torch.manual_seed(5)
    m = Diffusion(dit_config(length=40, hidden_size=64, cond_dim=32, n_blocks=2, n_heads=4, dropout=0.0)).to(DEV).eval()
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn_like(p) * 0.2)                            # the zero-initialised output maps carry signal
    m.rng_mode, m.philox_seed, m.elbo_trace = "philox", 3, []
    x0 = torch.randint(0, 4, (6, 40), device=DEV)
    nll = m._forward_pass_diffusion(x0)
    tr = m.elbo_trace[0]
    with torch.no_grad():
        logits = m.backbone(tr["xt"].long(), torch.zeros(6, device=DEV)).float()
        logits[..., 4] += -1000000.0
        logits = logits - torch.logsumexp(logits, dim=-1, keepdim=True)
        lp = logits.gather(-1, x0[..., None]).squeeze(-1)
        want = torch.where(tr["xt"] == 4, -lp * tr["w"][:, None], torch.zeros_like(lp))
    assert torch.equal(nll == 0, want == 0) and float((nll - want).abs().max() / want.abs().max()) <= 2e-7


# ------------------------------------------------------------------------------------------ harness, CLI, refusals
def test_harness_evaluate_nll_and_cli(tmp_path):
    from svdd_amd import cli, synthetic
    from svdd_amd.harness import BaseModel
    model, emb, head, reward = synthetic.build("rna", DEV)
    model.config.sampling.steps = 8
    model.rng_mode, model.philox_seed = "philox", 5
    bm = BaseModel(emb, head, model, reward, 4).to(DEV).eval()
    out = bm.controlled_decode(gen_batch_num=2, sample_M=2)
    dec = bm.evaluate_nll(out[0], n_draws=2)
    base = bm.evaluate_nll(bm.baseline_samples, n_draws=2)
    assert dec.shape == (8,) and base.shape == (8,) and len(bm.baseline_samples) == 2
    assert bool(torch.isfinite(dec).all()) and bool(torch.isfinite(base).all())
    assert torch.equal(dec, model.sequence_nll(torch.cat(out[0]), n_draws=2))
    path, _ = cli.main("mc", ["--task", "rna", "--batch_size", "2", "--sample_M", "2", "--val_batch_num", "1", "--rng", "philox",
                              "--out_dir", str(tmp_path), "--eval_nll", "2"])
    z = np.load(path)
    assert sorted(z.files) == ["baseline", "baseline_nll", "decoding", "decoding_nll"]
    assert z["decoding_nll"].shape == (2,) and np.isfinite(z["baseline_nll"]).all()
    path0, _ = cli.main("mc", ["--task", "rna", "--batch_size", "2", "--sample_M", "2", "--val_batch_num", "1", "--rng", "philox",
                               "--out_dir", str(tmp_path / "off")])
    assert sorted(np.load(path0).files) == ["baseline", "decoding"]


def test_refused_configurations(nets):
    from svdd_amd import ops
    m = model_for(nets, "g31", 50)
    x0 = torch.randint(0, 4, (2, 50), device=DEV)
    for attr, val, match in (("time_conditioning", True, "time-conditioned"), ("T", 4, "T = 0")):
        old = getattr(m, attr)
        setattr(m, attr, val)
        try:
            with pytest.raises(NotImplementedError, match=match):
                m.sequence_nll(x0)
        finally:
            setattr(m, attr, old)
    for attr in ("importance_sampling", "change_of_variables"):
        setattr(m.config.training, attr, True)
        try:
            with pytest.raises(NotImplementedError, match="importance_sampling"):
                m._loss(x0, torch.ones(2, 50, device=DEV))
        finally:
            setattr(m.config.training, attr, False)
    with pytest.raises(ops.SvddError, match="GPU tensor"):
        m.sequence_nll(x0.cpu())
    with pytest.raises(TypeError):
        m._loss(x0, None)                                                  # as the reference: loss * None
    with pytest.raises(ops.SvddError, match="token > 3"):
        m.sequence_nll(torch.full((2, 50), 4, device=DEV))
    m.rng_mode = "philox"
    with pytest.raises(ValueError, match="n_draws"):
        m.sequence_nll(x0, n_draws=9, chunk_rows=8)
    m.rng_mode = "replay"
    from svdd_amd import synthetic
    cpu_model = synthetic.build("rna", "cpu")[0]
    with pytest.raises(ops.SvddError, match="GPU only"):
        cpu_model.sequence_nll(x0)
