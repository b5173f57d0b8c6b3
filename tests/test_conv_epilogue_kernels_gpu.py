"""-m gpu: svdd_conv1d_cl_f32 (the generic kernel's four instantiations, the nine statically scheduled ones, the fused epilogue with its
four `act` values and the optional LayerNorm, forward and — on the flipped / transposed pack — backward-data) and
svdd_epilogue_ln_f32, each on its own through the C ABI against the float64 restatements of tests/bb_grad_ref.py. ReLU is continuous
in the forward direction: no element is excluded from any comparison.

Every output sits in a sentinel-filled buffer with guard space on both sides (tests/kernel_harness.py): guards intact, exactly the
contract's elements written, a second launch the same bits. Bars: kernel_harness._report on ref32 = the same function in chained
fp32 (bb_grad_ref: one accumulator per output, 2-wide steps in the kernels' channel and tap order, the bias added to the finished
sum), margin 4 for the convolution and for f_out (one reduction plus element-wise work), margin 8 for hn (a LayerNorm with a hardware
rsqrt behind it). Every svdd_conv1d_cl_f32 bar is capped by the flat tolerance tests/test_fused_gpu.py holds the same output to —
2e-5 for y (generic, static, dynamic, backward-data), 5e-5 for hn, absolute — so a bar here can only be tighter. svdd_epilogue_ln_f32
has no older test of its own; its caps are the same two figures times max(1, max|ref64|) (rows of offset 100 have an ulp of 7.6e-6).
One line `ERR <name> <err> bar <bar>` per comparison."""
import functools
import itertools

import pytest
import torch

from svdd_amd import _lib
from svdd_amd.fused import pack_conv
from tests import bb_grad_ref as B
from tests import grad_ref as R
from tests import net_ref as N
from tests.kernel_harness import DEV, _dev, _p, _report, _st, _twice

pytestmark = pytest.mark.gpu
FLAT_Y, FLAT_HN = 2e-5, 5e-5                            # tests/test_fused_gpu.py: test_conv1d_cl_kernel_vs_torch / _fused_epilogue


def _cap(flat, r64):
    """svdd_epilogue_ln_f32 only: the flat figure relative to the scale of the output."""
    return flat * max(1.0, float(r64.abs().max()))


def _conv(xd, wp, n, L, cin, cout, T, dil, bias=None, f_prev=None, act=-1, ln=None, name="svdd_conv1d_cl_f32"):
    """One guarded, twice-launched call -> (y, hn | None) as CPU tensors [n, L, cout]; ln = (tb | None, gamma, beta) or None."""
    lib = _lib.lib()
    tb, gm, bt = ln if ln is not None else (None, None, None)

    def launch(y, hn=None):
        return lib.svdd_conv1d_cl_f32(xd.data_ptr(), wp.data_ptr(), y, n, L, cin, cout, T, dil, _p(bias), _p(f_prev), act, _p(tb), _p(gm), _p(bt), hn, _st())
    bufs = _twice(name, launch, [n * L * cout] * (1 if ln is None else 2))
    return bufs[0].cpu(n, L, cout), (bufs[1].cpu(n, L, cout) if ln is not None else None)


def _conv_inputs(key, n, L, cin, cout, T):
    g = R._gen(31, *key)
    return torch.randn(n, L, cin, generator=g), torch.randn(cout, cin, T, generator=g) / (cin * T) ** 0.5, g


# --------------------------------------------------------------------------------------------------------- generic kernel
# (L, dilation, n). 37 x 16: the taps +-3, +-4 of nine are dead and a ragged second tile of six sequences ; 50 x 64: only the centre
# tap lives ; 1, 7, 112: n is no multiple of the 224, 32, 2 sequences of a tile (a partly filled last tile and rows beyond the batch) ;
# 112 / 113: 224 // L changes from 2 to 1 ; 224: the whole tile, no padding row
GENERIC_SHAPES = [(37, 16, 7), (50, 64, 5), (1, 1, 225), (7, 2, 33), (112, 3, 3), (113, 3, 3), (200, 5, 3), (224, 7, 2)]


@pytest.mark.parametrize("L,dil,n", GENERIC_SHAPES)
@pytest.mark.parametrize("cin,cout", [(64, 64), (64, 128), (128, 64), (128, 128)])
def test_conv1d_cl_generic_kernel(cin, cout, L, dil, n):
    """conv1d_cl_kernel<cin, cout> (act = -1; svdd_conv1d_set_dynamic(1) keeps the shapes that have a static kernel on it too) with
    1, 3, 5 and 9 taps: y exactly [n, L, cout] written, against conv_dilated."""
    lib = _lib.lib()
    lib.svdd_conv1d_set_dynamic(1)
    try:
        for T in (1, 3, 5, 9):
            x, w, _ = _conv_inputs((cin, cout, L, dil, n, T), n, L, cin, cout, T)
            y, _ = _conv(_dev(x), _dev(pack_conv(w)), n, L, cin, cout, T, dil)
            r64, r32 = R.ref64(B.conv_dilated, x, w, dil), R.ref32(B.conv_dilated, x, w, dil)
            _report(f"conv generic {cin}->{cout} T={T} dil={dil} L={L} n={n}", y, r64, r32, 4, cap=FLAT_Y)
    finally:
        lib.svdd_conv1d_set_dynamic(0)


# --------------------------------------------------------------------------------------------------------- static kernels
STATIC = [(128, 9, d, L, n) for d in (1, 4, 16, 64) for L, n in ((200, 1), (200, 5), (50, 1), (50, 6))] + \
         [(64, 5, 1, L, n) for L, n in ((200, 1), (200, 5), (50, 1), (50, 6))]


@pytest.mark.parametrize("C,T,dil,L,n", STATIC)
def test_conv1d_cl_static_kernels_and_fused_epilogue(C, T, dil, L, n):
    """conv1d_cl_static_kernel<C, C, T, dil, L>: act -1 (raw; bias and f_prev, if passed, are not read), and act 0 / 1 / 2 with bias
    and f_prev each present and NULL, without LayerNorm, with it and tb, with it and tb NULL. n = 6 at L = 50: the last tile holds 2
    of 4 sequences. y carries the same bits with and without the LayerNorm; the generic kernel on the same problem meets the same bar."""
    lib = _lib.lib()
    x, w, g = _conv_inputs((C, T, dil, L, n), n, L, C, C, T)
    bias, tb, beta = (torch.randn(C, generator=g) for _ in range(3))
    gamma, fp = torch.rand(C, generator=g) + 0.5, torch.randn(n, L, C, generator=g)
    xd, wp, bd, tbd, gd, btd, fpd = (_dev(t) for t in (x, pack_conv(w), bias, tb, gamma, beta, fp))
    c64, c32 = R.ref64(B.conv_dilated, x, w, dil), R.ref32(B.conv_dilated, x, w, dil)
    tag = f"conv static {C}x{T} dil={dil} L={L} n={n}"
    raw, _ = _conv(xd, wp, n, L, C, C, T, dil)
    _report(f"{tag} act=-1", raw, c64, c32, 4, cap=FLAT_Y)
    raw2, _ = _conv(xd, wp, n, L, C, C, T, dil, bias=bd, f_prev=fpd)
    assert torch.equal(raw2.view(torch.int32), raw.view(torch.int32)), "act -1 read its bias / f_prev"
    lib.svdd_conv1d_set_dynamic(1)
    try:
        dyn, _ = _conv(xd, wp, n, L, C, C, T, dil)
    finally:
        lib.svdd_conv1d_set_dynamic(0)
    _report(f"{tag} act=-1 dynamic", dyn, c64, c32, 4, cap=FLAT_Y)
    for act, with_b, with_f in itertools.product((0, 1, 2), (True, False), (True, False)):
        b, f = (bias if with_b else None), (fp if with_f else None)
        y0 = None
        for ln in ("none", "tb", "no_tb"):
            t = tb if ln == "tb" else None
            lnd = None if ln == "none" else (tbd if ln == "tb" else None, gd, btd)
            y, hn = _conv(xd, wp, n, L, C, C, T, dil, bias=bd if with_b else None, f_prev=fpd if with_f else None, act=act, ln=lnd)
            gm, bt = (None, None) if ln == "none" else (gamma, beta)
            f64, h64 = R.ref64(B.epilogue, c64, b, f, t, gm, bt, act)
            f32, h32 = B.epilogue(c32, b, f, t, gm, bt, act)
            t2 = f"{tag} act={act} bias={int(with_b)} f_prev={int(with_f)} ln={ln}"
            _report(f"{t2} y", y, f64, f32, 4, cap=FLAT_Y)
            if ln == "none":
                y0 = y
            else:
                assert torch.equal(y.view(torch.int32), y0.view(torch.int32)), "y differs with and without the LayerNorm"
                _report(f"{t2} hn", hn, h64, h32, 8, cap=FLAT_HN)


# ----------------------------------------------------------------------------------------------------------- backward-data
@functools.lru_cache(maxsize=None)
def _backbone_packs():
    """The dilated convolutions of a 20-distinct-layer CNNModel with the (forward, backward-data, dilation) packs the engine's own
    helper makes (CNNModel._conv_packs, what forward2 hands fused.DilatedConvFunction)."""
    from svdd_amd import backbone, config
    torch.manual_seed(12)
    cnn = N.distinct_layers(backbone.CNNModel(config.dna_config().model, alphabet_size=5).eval(), 12).to(DEV)
    return [c.weight.detach().cpu() for c in cnn.convs], cnn._conv_packs()


@functools.lru_cache(maxsize=None)
def _tower_packs():
    """The reward tower's folded 64 -> 64 x 5 weights and the transposed packs FusedValueNet._grad_pack makes for its backward."""
    from svdd_amd import synthetic
    model, _, _, reward = synthetic.build("dna", DEV)
    fn = model.reward_callable(reward)
    return [w.detach().float().cpu() for w in fn._folded_ws], fn._grad_pack()[1]


@pytest.mark.parametrize("L,n", [(200, 2), (50, 6), (113, 2)])
@pytest.mark.parametrize("which", ["bb_dil4", "bb_dil64", "tower"])
def test_conv1d_cl_backward_data_on_the_engines_pack(which, L, n):
    """The kernel on the flipped / transposed pack the engine uses for a convolution's backward-data pass, against the transpose
    reference (conv_dilated_t): 128 -> 128 x 9 at dilation 4 and 64, 64 -> 64 x 5. L = 200 / 50: static kernels ; 113: the generic one."""
    if which == "tower":
        ws, packs_t = _tower_packs()
        w, wpt, dil = ws[1], packs_t[1], 1
    else:
        ws, packs = _backbone_packs()
        i = {"bb_dil4": 9, "bb_dil64": 17}[which]
        w, (_, wpt, dil) = ws[i], packs[i]
        assert dil == {"bb_dil4": 4, "bb_dil64": 64}[which]
    cout, cin, T = w.shape
    g = torch.randn(n, L, cout, generator=R._gen(32, cout, T, dil, L, n))
    dx, _ = _conv(_dev(g), wpt, n, L, cout, cin, T, dil)
    r64, r32 = R.ref64(B.conv_dilated_t, g, w, dil), R.ref32(B.conv_dilated_t, g, w, dil)
    _report(f"conv backward-data {which} L={L} n={n}", dx, r64, r32, 4, cap=FLAT_Y)


# ------------------------------------------------------------------------------------------------------ svdd_epilogue_ln_f32
def _epilogue(yd, rows, C, act, bias, f_prev, tb, gamma, beta, with_f, with_hn):
    """One guarded, twice-launched svdd_epilogue_ln_f32 call -> (f_out | None, hn | None) [rows, C] on the CPU. A NULL output's buffer
    is not handed to the kernel and must keep its sentinel, as must every guard."""
    lib = _lib.lib()
    f_out, hn = _twice("svdd_epilogue_ln_f32",
                       lambda fo, h: lib.svdd_epilogue_ln_f32(yd.data_ptr(), _p(bias), _p(f_prev), _p(tb), _p(gamma), _p(beta), fo if with_f else None,
                                                              h if with_hn else None, rows, C, act, _st()),
                       [rows * C, rows * C], written=[with_f, with_hn])
    return (f_out.cpu(rows, C) if with_f else None), (hn.cpu(rows, C) if with_hn else None)


def _epilogue_case(tag, d, dd, rows, C, act, with_b, with_p, with_tb, with_f, with_hn):
    pick = lambda src, k, on: src[k] if on else None   # noqa: E731
    f, hn = _epilogue(dd["y"], rows, C, act, pick(dd, "bias", with_b), pick(dd, "f_prev", with_p), pick(dd, "tb", with_tb),
                      pick(dd, "gamma", with_hn), pick(dd, "beta", with_hn), with_f, with_hn)
    args = (d["y"], pick(d, "bias", with_b), pick(d, "f_prev", with_p), pick(d, "tb", with_tb), pick(d, "gamma", with_hn), pick(d, "beta", with_hn), act)
    (f64, h64), (f32, h32) = R.ref64(B.epilogue, *args), R.ref32(B.epilogue, *args)
    t = f"{tag} act={act} bias={int(with_b)} f_prev={int(with_p)} tb={int(with_tb)}"
    if with_f:
        _report(f"{t} f_out", f, f64, f32, 4, cap=_cap(FLAT_Y, f64))
    if with_hn:
        _report(f"{t} hn", hn, h64, h32, 8, cap=_cap(FLAT_HN, h64))


def _epilogue_inputs(rows, C, offset=0.0):
    g = R._gen(33, rows, C)
    d = dict(y=torch.randn(rows, C, generator=g) + offset, f_prev=torch.randn(rows, C, generator=g), bias=torch.randn(C, generator=g),
             tb=torch.randn(C, generator=g), gamma=torch.rand(C, generator=g) + 0.5, beta=torch.randn(C, generator=g) * 0.3)
    return d, {k: _dev(v) for k, v in d.items()}


OUTPUTS = [(True, True), (True, False), (False, True)]


@pytest.mark.parametrize("rows", [1, 3, 5, 16384, 16385, 40001])
@pytest.mark.parametrize("C", [64, 128, 256])
def test_epilogue_ln(C, rows):
    """epilogue_ln_kernel<C / 64>. Only at rows 1, 3, 5 (a last block of one to three waves): act 0 / 1 / 2 x every permitted NULL
    combination of bias, f_prev, tb, f_out, hn (hn given: gamma and beta given). 16,384 rows fill the 4,096 blocks x 4 waves exactly,
    16,385 and 40,001 enter the grid-stride loop (40,001: a third, ragged pass); there THREE combinations run, one act each (run time:
    the float64 reference of 10 M elements): everything given, then hn alone without the optional inputs, then f_out alone with tb
    NULL. The sentinel check holds every row of those written."""
    d, dd = _epilogue_inputs(rows, C)
    tag = f"epilogue C={C} rows={rows}"
    if rows <= 5:
        for act, with_b, with_p, with_tb, (with_f, with_hn) in itertools.product((0, 1, 2), (True, False), (True, False), (True, False), OUTPUTS):
            _epilogue_case(tag, d, dd, rows, C, act, with_b, with_p, with_tb, with_f, with_hn)
    else:
        act = (C // 64 + rows) % 3
        _epilogue_case(tag, d, dd, rows, C, act, True, True, True, True, True)
        _epilogue_case(tag, d, dd, rows, C, (act + 1) % 3, False, False, False, False, True)
        _epilogue_case(tag, d, dd, rows, C, (act + 2) % 3, True, True, False, True, False)


@pytest.mark.parametrize("C", [64, 128, 256])
def test_epilogue_ln_rows_with_a_common_offset_and_a_constant_row(C):
    """Rows of 100 + N(0, 1): a one-pass variance (E[v^2] - mean^2) would lose four digits here, the kernel's two-pass one does not.
    And a constant row (variance 0): hn = beta through the eps path, finite."""
    rows = 7
    d, dd = _epilogue_inputs(rows, C, offset=100.0)
    tag = f"epilogue offset C={C}"
    _epilogue_case(tag, d, dd, rows, C, 2, False, False, False, True, True)
    _epilogue_case(tag, d, dd, rows, C, 0, True, True, True, True, True)
    d["y"][2] = 3.0
    dd["y"] = _dev(d["y"])
    f, hn = _epilogue(dd["y"], rows, C, 2, None, None, None, dd["gamma"], dd["beta"], True, True)
    assert torch.equal(hn[2].view(torch.int32), d["beta"].view(torch.int32)), "a constant row: hn is not beta"
    _epilogue_case(tag + " const", d, dd, rows, C, 2, False, False, False, True, True)
