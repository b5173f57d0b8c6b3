"""-m gpu: every entry point of the reward net's gradient pass (csrc/svdd_gru_train.hip and the gated convolution of
csrc/svdd_nets.hip; what FusedValueNet.mean_score_input_grad launches) on its own through the C ABI, against the float64
restatement of the operation in tests/grad_ref.py, at the shapes that cross the boundaries the kernels have: grid caps (a second
grid-stride pass), ragged last tiles, L = 50 (several sequences per tile), degenerate lengths.

Every output sits in a sentinel-filled buffer with guard space on both sides: the guards must be intact, every element the contract
says is written must have lost the sentinel, and a second launch must give the same bits.

Bars are computed here from the references, never from the kernel: bar = margin x max|ref32 - ref64| on the same inputs, floored at
2 x 2^-23 x max|ref64| (grad_ref.bar), where ref32 is the fp32 restatement in the kernels' stated arithmetic: the two activation
formulas of the GRU, and every matrix product on ONE fp32 accumulator advanced in a dependent chain of 4-wide steps, as the MFMA
chains of the kernels are. (With torch's blocked CPU sgemm in its place, which keeps 8 - 16 partial sums per element and so lacks
the error growth any single-accumulator chain of 320 / 384 terms has, two of 446 comparisons came out at 1.04 and 1.10 of their
bar: conv_gated (4, 50) and dx from da (300, 7). The term was added to ref32, not to the margin; every bar stays far
below the 2e-5 / 2e-4 tests/test_fused_gpu.py holds the same quantities to.) margin 4: one
reduction plus element-wise work (stem pair, gated convolution, gi, dx from da, bb_layer_bwd); margin 8: a hardware transcendental
or chained steps (GRU forward and BPTT, tail_grad, bb_layer_fwd, the whole pass). ReLU kinks are excluded by conditions on the
float64 reference alone, under caps (grad_ref.near_kink / tail_kink_rows / tail_kink_seqs); tests/test_grad_ref_cpu.py shows the
caps hold for these inputs. Exact comparisons stay exact. One line `ERR <name> <err> bar <bar>` is printed per comparison."""
import pytest
import torch

from svdd_amd import _lib
from svdd_amd.fused import pack_conv, pack_gru, pack_gru_bwd
from tests import grad_ref as R
from tests.kernel_harness import DEV, _dev, _p, _report, _st, _twice

pytestmark = pytest.mark.gpu


# -------------------------------------------------------------------------------------------------------------------- stem
@pytest.mark.parametrize("n,L", R.STEM_CASES)
def test_reward_stem_and_its_transpose(n, L):
    """svdd_reward_stem_f32 / svdd_reward_stem_bwd_f32. (1, 7): the 15 taps are wider than the sequence; (3, 50), (331, 50): rows % 4
    != 0; (83, 200) = 16,600 and (331, 50) = 16,550 rows: a second grid-stride pass (4,096 workgroups x 4 rows); neighbouring
    sequences sit 1e3 apart (even ones near 1, odd ones near 1e3, each level compared under a bar of its own), so a tap read
    across a sequence boundary is an error of 1e2 under a bar of 1e-6. The zero pattern of the
    output is the float64 ReLU decision except where the pre-activation is within 1e-6 of its terms' magnitude of zero."""
    lib = _lib.lib()
    x, w, b, g = R.stem_inputs(n, L)
    wk = _dev(w.permute(2, 1, 0).reshape(-1, 64))                      # [(t, c)][co]
    xd, bd = _dev(x), _dev(b)
    (out,) = _twice("svdd_reward_stem_f32", lambda o: lib.svdd_reward_stem_f32(xd.data_ptr(), wk.data_ptr(), bd.data_ptr(), o, n, L, 15, _st()),
                    [n * L * 64])
    got = out.cpu(n, L, 64)
    par = torch.arange(n) % 2                                           # each level of magnitude under its own bar
    r64, r32 = R.ref64(R.stem, x, w, b), R.ref32(R.stem, x, w, b)
    for k in range(min(n, 2)):
        _report(f"stem n={n} L={L} level={k}", got, r64, r32, 4, keep=par == k)
    pre = R.ref64(R.stem_pre, x, w, b)
    kink = R.near_kink(pre, R.ref64(R.stem_terms, x, w, b))
    assert float(kink.double().mean()) <= R.STEM_KINK_CAP
    assert torch.equal((got > 0)[~kink], (pre > 0)[~kink]), "stem: ReLU decisions away from any kink differ from float64"
    gm = torch.where(pre > 0, g, torch.zeros_like(g))                   # the gradient at the pre-activation
    gd = _dev(gm)
    (dx,) = _twice("svdd_reward_stem_bwd_f32", lambda o: lib.svdd_reward_stem_bwd_f32(gd.data_ptr(), wk.data_ptr(), o, n, L, 15, _st()), [n * L * 4])
    r64, r32 = R.ref64(R.stem_bwd, gm, w), R.ref32(R.stem_bwd, gm, w)
    for k in range(min(n, 2)):
        _report(f"stem_bwd n={n} L={L} level={k}", dx.cpu(n, L, 4), r64, r32, 4, keep=par == k)


# ------------------------------------------------------------------------------------------------------- gated convolution
@pytest.mark.parametrize("n,L", [(1, 200), (7, 200), (300, 200), (1, 50), (3, 50), (4, 50), (5, 50), (9, 50), (161, 50)])
def test_conv1d_cl_gated(n, L):
    """svdd_conv1d_cl_gated_f32: gate > 0 ? conv^T(g) + f_prev : 0. L = 200: one sequence per tile; L = 50: four, with 1, 3, 4, 5 (a
    ragged second tile), 9 and 161 sequences. gate given / NULL x f_prev NULL / a separate tensor / the input itself (what
    mean_score_input_grad passes): the aliased call gives the bits of the separate one. The gate is an input: no exclusion, the
    zero pattern is exact."""
    lib = _lib.lib()
    gen = R._gen(6, n, L)
    g = torch.randn(n, L, 64, generator=gen)
    gate = torch.randn(n, L, 64, generator=gen)
    gate[0, 0, :8] = torch.tensor([0.0, -0.0, 1e-45, -1e-45, 1e-38, -1e-38, 1.0, -1.0])[:8]
    w5 = torch.randn(64, 64, 5, generator=gen) * 0.1
    wt = _dev(pack_conv(w5.flip(2).transpose(0, 1).contiguous()))
    gd, gated, copy = _dev(g), _dev(gate), _dev(g).clone()
    for use_gate in (True, False):
        res = {}
        for fp in ("none", "separate", "aliased"):
            fptr = {"none": None, "separate": copy.data_ptr(), "aliased": gd.data_ptr()}[fp]
            (y,) = _twice("svdd_conv1d_cl_gated_f32",
                          lambda o: lib.svdd_conv1d_cl_gated_f32(gd.data_ptr(), wt.data_ptr(), o, n, L, 64, 64, 5, 1, fptr, _p(gated) if use_gate else None, _st()),
                          [n * L * 64])
            res[fp] = y
            args = (g, w5, None if fp == "none" else g, gate if use_gate else None)
            got = y.cpu(n, L, 64)
            _report(f"conv_gated n={n} L={L} gate={int(use_gate)} f_prev={fp}", got, R.ref64(R.conv_gated, *args), R.ref32(R.conv_gated, *args), 4)
            if use_gate:
                shut = ~(gate > 0)
                assert bool((got.view(torch.int32)[shut] == 0).all()), "a shut gate must store +0.0"
        assert torch.equal(res["aliased"].bits(), res["separate"].bits())


# --------------------------------------------------------------------------------------------------------------------- GRU
# every n at one L (tiles of 16 sequences with 1 - 15 live rows), every L at one ragged n, and (41, 200) = 8,200 rows: beyond
# gru_xproj_kernel's cap (512 tiles x 16 rows) with a last tile of 8 rows
GRU_CASES = [(n, 7) for n in (1, 15, 16, 17, 37, 300)] + [(17, L) for L in (1, 2, 50, 200)] + [(41, 200)]


def _gru_forward(lib, mod, x, n, L, two):
    wpack, bpack = (_dev(t) for t in pack_gru(mod))
    xd = _dev(x)
    if two:
        return _twice("svdd_gru_bidir_train2_f32",
                      lambda gi, o, s: lib.svdd_gru_bidir_train2_f32(xd.data_ptr(), wpack.data_ptr(), bpack.data_ptr(), gi, o, s, n, L, _st()),
                      [2 * n * L * 192, 2 * n * L * 64, 2 * n * L * 256])
    return _twice("svdd_gru_bidir_train_f32",
                  lambda o, s: lib.svdd_gru_bidir_train_f32(xd.data_ptr(), wpack.data_ptr(), bpack.data_ptr(), o, s, n, L, _st()),
                  [2 * n * L * 64, 2 * n * L * 256])


@pytest.mark.parametrize("n,L", GRU_CASES)
def test_gru_train_and_train2_forward(n, L):
    """svdd_gru_bidir_train_f32 and svdd_gru_bidir_train2_f32 against float64: the hidden states, each of the four saved planes
    (r, z, n, W_hn h + b_hn) and train2's gi = b + W_i x (b: b_i + b_h for r and z, b_in for n). out and save of train2 are the bits
    of train."""
    lib = _lib.lib()
    mod, x, _ = R.gru_inputs(n, L)
    w = R.gru_weights_of(mod)
    o1, s1 = _gru_forward(lib, mod, x, n, L, False)
    gi, o2, s2 = _gru_forward(lib, mod, x, n, L, True)
    assert torch.equal(o1.bits(), o2.bits()) and torch.equal(s1.bits(), s2.bits())
    r64, r32 = R.ref64(R.gru, x, w), R.ref32(R.gru, x, w)
    for tag, o, s in (("train", o1, s1), ("train2", o2, s2)):
        _report(f"gru_{tag} out n={n} L={L}", o.cpu(2, n, L, 64), r64["out"], r32["out"], 8)
        sv = s.cpu(2, n, L, 4, 64)
        for k, plane in enumerate(("r", "z", "n", "hn")):
            _report(f"gru_{tag} save.{plane} n={n} L={L}", sv[:, :, :, k], r64["save"][:, :, :, k], r32["save"][:, :, :, k], 8)
    _report(f"gru_train2 gi n={n} L={L}", gi.cpu(2, n * L, 192), r64["gi"], r32["gi"], 4)


def _gru_backward_checks(lib, tag, mod, x, gout, out_t, save_t, n, L):
    """Both BPTT entry points on the given out / save (fp32 CPU tensors), against float64 BPTT of the same out / save."""
    w = R.gru_weights_of(mod)
    wb = _dev(pack_gru_bwd(mod))
    god, od, sd, xd = _dev(gout), _dev(out_t), _dev(save_t), _dev(x)
    r64, r32 = R.ref64(R.gru_bwd, gout, out_t, save_t, w), R.ref32(R.gru_bwd, gout, out_t, save_t, w)
    (dx,) = _twice("svdd_gru_bidir_bwd_f32", lambda o: lib.svdd_gru_bidir_bwd_f32(god.data_ptr(), od.data_ptr(), sd.data_ptr(), wb.data_ptr(), o, n, L, _st()),
                   [2 * n * L * 64])
    dxc = dx.cpu(2, n, L, 64)
    for d in range(2):
        _report(f"gru_bwd{tag} dx[{d}] n={n} L={L}", dxc[d], r64["dx"][d], r32["dx"][d], 8)
    for use_gate in (True, False):
        da, g = _twice("svdd_gru_bidir_bwd2_f32",
                       lambda a, o: lib.svdd_gru_bidir_bwd2_f32(god.data_ptr(), od.data_ptr(), sd.data_ptr(), wb.data_ptr(), a, xd.data_ptr() if use_gate else None,
                                                                o, n, L, _st()), [2 * n * L * 192, n * L * 64])
        dac, gc = da.cpu(2, n * L, 192), g.cpu(n * L, 64)
        gate = x.reshape(n * L, 64) if use_gate else None
        t = f"gru_bwd2{tag} gate={int(use_gate)}"
        _report(f"{t} da n={n} L={L}", dac, r64["da"], r32["da"], 8)
        # the second launch as a function of its own input, the kernel's da: one reduction
        _report(f"{t} dx_from_da n={n} L={L}", gc, R.ref64(R.gru_dx_gate, dac, w, gate), R.ref32(R.gru_dx_gate, dac, w, gate), 4)
        # ... and the pair end to end
        want64, want32 = r64["dx"][0] + r64["dx"][1], r32["dx"][0] + r32["dx"][1]
        if use_gate:
            want64, want32 = (torch.where(x > 0, v, torch.zeros_like(v)) for v in (want64, want32))
            assert bool((gc.view(torch.int32)[~(gate > 0)] == 0).all()), "a shut gate must store +0.0"
        _report(f"{t} g n={n} L={L}", gc.view(n, L, 64), want64, want32, 8)


@pytest.mark.parametrize("n,L", GRU_CASES + [(83, 200)])
def test_gru_bptt_on_the_kernels_own_forward(n, L):
    """svdd_gru_bidir_bwd_f32 (dx per direction) and svdd_gru_bidir_bwd2_f32 (da, and the gated sum, gate given / NULL) as functions of
    their inputs: fed with the forward kernel's own out / save, compared with float64 BPTT of those very values. (83, 200) = 16,600
    rows: beyond gru_dx_gate_kernel's cap (1,024 tiles x 16 rows)."""
    lib = _lib.lib()
    mod, x, gout = R.gru_inputs(n, L)
    _, o, s = _gru_forward(lib, mod, x, n, L, True)
    _gru_backward_checks(lib, "", mod, x, gout, o.cpu(2, n, L, 64), s.cpu(2, n, L, 4, 64), n, L)


@pytest.mark.parametrize("n,L", [(17, 7), (37, 7), (17, 200)])
def test_gru_bptt_on_the_reference_forward(n, L):
    """The same fed with the float64 reference's out / save rounded to fp32: BPTT alone, without the forward kernel's rounding."""
    mod, x, gout = R.gru_inputs(n, L)
    fw = R.ref64(R.gru, x, R.gru_weights_of(mod))
    _gru_backward_checks(_lib.lib(), "@ref", mod, x, gout, fw["out"].float(), fw["save"].float(), n, L)


# -------------------------------------------------------------------------------------------------------------------- tail
@pytest.mark.parametrize("n,L", R.TAIL_CASES)
def test_reward_tail_grad(n, L):
    """svdd_reward_tail_grad_f32 with a non-trivial LayerNorm affine. rows % 16 in {1, 7, 6, 8}; (41, 200) = 8,200 rows: a second
    pass beyond 512 workgroups x 16 rows; n L never a power of two except (1, 1) (the 1 / (n L) seed). g_fwd and g_bwd are the same
    bits. A row with a float64 pre-activation within 1e-5 of zero is excluded (cap 0.5 % of rows)."""
    lib = _lib.lib()
    h, w1, b1, gam, bet, weff = R.tail_inputs(n, L)
    hd, w1d, b1d, gd, bd, wd = (_dev(t) for t in (h, w1, b1, gam, bet, weff))
    g0, g1 = _twice("svdd_reward_tail_grad_f32",
                    lambda a, b: lib.svdd_reward_tail_grad_f32(hd[0].data_ptr(), hd[1].data_ptr(), w1d.data_ptr(), b1d.data_ptr(), gd.data_ptr(), bd.data_ptr(),
                                                               wd.data_ptr(), 1e-5, n, L, a, b, _st()), [n * L * 64, n * L * 64])
    assert torch.equal(g0.bits(), g1.bits())
    args = (h[0], h[1], w1, b1, gam, bet, weff, 1e-5)
    (r64, z), (r32, _) = R.ref64(R.tail_grad, *args), R.ref32(R.tail_grad, *args)
    kink = R.tail_kink_rows(z)
    assert float(kink.double().mean()) <= R.TAIL_ROW_CAP
    _report(f"tail_grad n={n} L={L}", g0.cpu(n, L, 64), r64, r32, 8, keep=~kink)


# ---------------------------------------------------------------------------------------------------------- backbone layer
@pytest.mark.parametrize("C", R.BB_CHANNELS)
@pytest.mark.parametrize("rows,rps", R.BB_CASES)
def test_bb_layer_fwd_and_bwd(rows, rps, C):
    """svdd_bb_layer_fwd_f32 / svdd_bb_layer_bwd_f32 at 64, 128 and 256 channels (the three instantiations) with a time bias that
    differs between sequences; 32,771 rows enter a second grid-stride pass (8,192 workgroups x 4 rows) whose stride 7 rows per
    sequence do not divide. Every optional-pointer combination the header allows; what a combination does not write stays untouched.
    Mask bytes are exactly 0 / 1 and equal the float64 decision except within 1e-6 of the terms' magnitude of zero (cap 0.1 %)."""
    lib = _lib.lib()
    d = R.bb_inputs(rows, rps, C)
    dd = {k: _dev(v) for k, v in d.items()}
    N = rows * C
    combos = [(True, True), (True, False), (False, True)] if rows < 30000 else [(True, True)]
    for with_y, with_ln in combos:
        f_out, mask, hn = _twice(
            "svdd_bb_layer_fwd_f32",
            lambda fo, mk, h: lib.svdd_bb_layer_fwd_f32(_p(dd["y"]) if with_y else None, _p(dd["bias"]) if with_y else None, _p(dd["f_prev"]),
                                                        _p(dd["tb"]) if with_ln else None, _p(dd["gamma"]) if with_ln else None,
                                                        _p(dd["beta"]) if with_ln else None, 1e-5, fo, mk, h, rows, rps, C, _st()),
            [N, (N, torch.uint8), N], written=[with_y, with_y, with_ln])
        args = (d["y"] if with_y else None, d["bias"], d["f_prev"], d["tb"], d["gamma"] if with_ln else None, d["beta"], 1e-5, rps)
        r64, r32 = R.ref64(R.bb_layer_fwd, *args), R.ref32(R.bb_layer_fwd, *args)
        t = f"bb_fwd C={C} rows={rows} rps={rps} y={int(with_y)} ln={int(with_ln)}"
        if with_y:
            _report(f"{t} f_out", f_out.cpu(rows, C), r64["f_out"], r32["f_out"], 8)
            mk = mask.cpu(rows, C)
            assert int(mk.max()) <= 1
            kink = R.near_kink(r64["pre"], d["y"].double().abs() + d["bias"].double().abs())
            assert float(kink.double().mean()) <= R.MASK_KINK_CAP
            assert torch.equal(mk.bool()[~kink], r64["mask"][~kink])
        if with_ln:
            _report(f"{t} hn", hn.cpu(rows, C), r64["hn"], r32["hn"], 8)
    for with_mask in ((True, False) if rows < 30000 else (True,)):
        g_out, gt = _twice(
            "svdd_bb_layer_bwd_f32",
            lambda go, gt_: lib.svdd_bb_layer_bwd_f32(_p(dd["g_hn"]), _p(dd["f_prev"]), _p(dd["tb"]), _p(dd["gamma"]), 1e-5, _p(dd["g_in"]),
                                                      _p(dd["mask_prev"]) if with_mask else None, go, gt_ if with_mask else None, rows, rps, C, _st()),
            [N, N], written=[True, with_mask])
        args = (d["g_hn"], d["f_prev"], d["tb"], d["gamma"], 1e-5, d["g_in"], d["mask_prev"] if with_mask else None, rps)
        r64, r32 = R.ref64(R.bb_layer_bwd, *args), R.ref32(R.bb_layer_bwd, *args)
        t = f"bb_bwd C={C} rows={rows} rps={rps} mask={int(with_mask)}"
        go = g_out.cpu(rows, C)
        _report(f"{t} g_out", go, r64["g_out"], r32["g_out"], 4)
        if with_mask:
            gtc = gt.cpu(rows, C)
            _report(f"{t} gt_out", gtc, r64["gt_out"], r32["gt_out"], 4)
            assert torch.equal(gtc.view(torch.int32), torch.where(d["mask_prev"].bool(), go, torch.zeros_like(go)).view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------- sum gate
@pytest.mark.parametrize("count", [4, 1028, 4194304 + 8])
def test_sum_gate_exact(count):
    """svdd_sum_gate_f32 = where(f > 0, a + b, 0) in fp32, bit for bit, with zeros, negative zeros and denormals of either sign in f
    (-0.0 and +0.0 gate shut, a positive denormal is > 0). 4,194,312 floats: a second pass beyond 4,096 workgroups x 256 x 4."""
    lib = _lib.lib()
    gen = R._gen(7, count)
    a, b, f = (torch.randn(count, generator=gen) for _ in range(3))
    special = torch.tensor([0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, 1.17549435e-38, -1.17549435e-38])
    pos = torch.randint(0, count, (max(4, count // 16),), generator=gen)
    f[pos] = special[torch.arange(pos.numel()) % 8]
    f[:4], f[-4:] = special[:4], special[2:6]
    ad, bd, fd = _dev(a), _dev(b), _dev(f)
    (g,) = _twice("svdd_sum_gate_f32", lambda o: lib.svdd_sum_gate_f32(ad.data_ptr(), bd.data_ptr(), fd.data_ptr(), o, count, _st()), [count])
    want = R.sum_gate(a, b, f)
    assert torch.equal(g.cpu().view(torch.int32), want.view(torch.int32))
    print(f"ERR sum_gate count={count} 0.000e+00 bar 0.0e+00")


# ---------------------------------------------------------------------------------------------------------- the whole pass
@pytest.mark.parametrize("task,B", R.PASS_CASES)
def test_mean_score_input_grad_vs_float64_with_pinned_tower_decisions(task, B):
    """FusedValueNet.mean_score_input_grad (16 launches, no autograd) against the float64 reference composed from grad_ref, with the
    tower's ReLU decisions pinned to the ones the kernels took (read from the activations the pass keeps with keep_grad_pass). A
    sequence with a tail pre-activation within 2e-6 of zero is excluded (cap max(1, 5 % of B)). Also the tower activations and the
    GRU outputs of the same call. ("dna", 41) = 8,200 rows and ("rna", 165) = 8,250 rows cross the tail's and gru_xproj's caps."""
    from svdd_amd import synthetic
    model, _, _, reward = synthetic.build(task, DEV)
    L = model.config.model.length
    fn = model.reward_callable(reward)
    assert fn.grad_ok(L)
    x = R.pass_input(task, B, L)
    plain = fn.mean_score_input_grad(_dev(x))
    assert fn.last_grad_pass is None                                   # off by default
    fn.keep_grad_pass = True
    try:
        got = fn.mean_score_input_grad(_dev(x))
        kept = fn.last_grad_pass
    finally:
        fn.keep_grad_pass, fn.last_grad_pass = False, None
    torch.cuda.synchronize()
    assert torch.equal(got, plain) and kept["grad"] is got
    fs = [f.cpu() for f in kept["fs"]]
    masks = [(f > 0) for f in fs]
    p = R.params_of(fn)
    r64, r32 = R.ref64(R.value_grad, x, p, masks), R.ref32(R.value_grad, x, p, masks)
    t = f"pass {task} B={B}"
    for k, f in enumerate(fs):
        _report(f"{t} fs[{k}]", f, r64["fs"][k], r32["fs"][k], 8)
    _report(f"{t} gru_out", kept["out"].cpu(), r64["out"], r32["out"], 8)
    kink = R.tail_kink_seqs(r64["z"])
    assert int(kink.sum()) <= R.seq_cap(B), int(kink.sum())
    _report(f"{t} g_tail", kept["g_tail"].cpu(), r64["g_tail"], r32["g_tail"], 8, keep=~kink)
    _report(f"{t} grad", got.cpu(), r64["grad"], r32["grad"], 8, keep=~kink)
