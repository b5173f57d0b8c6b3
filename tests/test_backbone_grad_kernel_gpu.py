"""-m gpu: svdd_backbone_cnn_grad_f32 (the whole backbone's input gradient in one launch; every DPS step at L > 104) on its own through
the C ABI, against the float64 restatement of tests/bb_grad_ref.py, at every length where its tap schedule, its masking of the
padding rows or its reversed dilation table does something else than at L = 200, and at other layer counts than 20.

The kernel takes the ReLU decisions, x-hat and 1 / sigma as INPUTS: given those, dx is a linear function of dlogits, so the float64
reference is evaluated on the very state one real svdd_backbone_cnn_save_f32 launch left (decoded from its lane-private layout, the
fp32 values converted exactly) and NO element is excluded from any comparison: there is no kink once the decisions are inputs.

Bars: tests/kernel_harness._report with margin 8 (a whole chained pass, the rule at the top of tests/test_grad_kernels_gpu.py) on
ref32 = the same function in chained fp32 (one accumulator per element, the kernel's step width and order), capped by the
5e-5 x max(1, max|ref64|) that tests/test_fused_gpu.py holds the same gradient to, so a bar here can only be tighter. At n = 37 the
chained fp32 restatement is computed for the first 3 sequences only and serves as the pool the bar is taken from; all 37 are compared
with float64. dx sits in a sentinel-filled buffer with guard space on both sides; two launches give the same bits; every input — the
saved arrays reach the kernel through a const_cast — keeps its bits. One line `ERR <name> <err> bar <bar>` per comparison.

Other layer counts re-concatenate slices of the 20-layer packs; the layers kept are chosen with DIFFERENT dilations ((64), (4, 64),
(1, 1, 4, 16, 64)) so that a dilation table read in the wrong order shows at every count."""
import ctypes
import functools

import pytest
import torch

from svdd_amd import _lib, fused
from tests import bb_grad_ref as B
from tests import grad_ref as R
from tests import net_ref as N
from tests.kernel_harness import DEV, _dev, _report, _st, _twice

pytestmark = pytest.mark.gpu
NL = 20
S1, SL = 4 * 128 * 32, 4 * 9 * 128 * 32                 # floats of the 1x1's tiles / of one conv layer's tiles
LAYERS = {1: (16,), 2: (8, 16), 5: (0, 4, 8, 12, 16)}   # dilations (64), (4, 64), (1, 1, 4, 16, 64)
POOL = 3                                                # sequences the chained fp32 restatement is computed for at large n


@functools.lru_cache(maxsize=None)
def _cnn():
    from svdd_amd import backbone, config
    torch.manual_seed(11)
    cnn = N.distinct_layers(backbone.CNNModel(config.dna_config().model, alphabet_size=5).eval(), 11).to(DEV)
    for p in cnn.parameters():
        p.requires_grad_(False)
    assert len(cnn.convs) == NL
    return cnn, fused.pack_backbone(cnn), fused.pack_backbone_grad(cnn)


@functools.lru_cache(maxsize=None)
def _packs(layers):
    """The operand images of both entries for the backbone made of `layers` (None: all 20), cut out of the 20-layer packs: forward
    tiles = the layers in order, then W_f1 ; vec = row 0, the layers' rows, the last row ; tiles_bwd = W_f1^T, then the layers in
    reverse ; gamma = the layers' rows -> (dict of device tensors + dil, natural-layout weights)."""
    cnn, pk, pkg = _cnn()
    if layers is None:
        return dict(pk, **pkg), B.weights_of(cnn)
    ks = list(layers)
    tb = pkg["tiles_bwd"]
    assert pk["tiles"].numel() == NL * SL + S1 and tb.numel() == S1 + NL * SL
    d = dict(table0=pk["table0"], w2=pk["w2"], dil=[pk["dil"][k] for k in ks],
             tiles=torch.cat([pk["tiles"][k * SL:(k + 1) * SL] for k in ks] + [pk["tiles"][NL * SL:]]).contiguous(),
             vec=torch.cat([pk["vec"][:1]] + [pk["vec"][1 + k:2 + k] for k in ks] + [pk["vec"][NL + 1:]]).contiguous(),
             tiles_bwd=torch.cat([tb[:S1]] + [tb[S1 + (NL - 1 - k) * SL:S1 + (NL - k) * SL] for k in reversed(ks)]).contiguous(),
             gamma=pkg["gamma"][ks].contiguous())
    return d, B.weights_of(cnn, ks)


def _dil(pk):
    return (ctypes.c_int * len(pk["dil"]))(*pk["dil"])


def _save(pk, tok, n, L):
    """One svdd_backbone_cnn_save_f32 launch -> (xhat [n, nl, 56, 512], rstd [n, nl, 208], mask [n, nl + 2, 512] int64) on the device;
    the xhat slots the kernel never writes stay zero."""
    nl = len(pk["dil"])
    out = torch.zeros(n, L, 5, device=DEV)
    xhat, rstd = torch.zeros(n, nl, 56, 512, device=DEV), torch.zeros(n, nl, 208, device=DEV)
    mask = torch.zeros(n, nl + 2, 512, dtype=torch.int64, device=DEV)
    _lib.check(_lib.lib().svdd_backbone_cnn_save_f32(tok.data_ptr(), pk["table0"].data_ptr(), pk["tiles"].data_ptr(), pk["vec"].data_ptr(),
                                                     pk["w2"].data_ptr(), out.data_ptr(), n, L, nl, _dil(pk), xhat.data_ptr(), rstd.data_ptr(),
                                                     mask.data_ptr(), _st()), "svdd_backbone_cnn_save_f32")
    torch.cuda.synchronize()
    return xhat, rstd, mask


def _grad(pk, dl, state, n, L):
    """dx of one (twice-launched, guarded) svdd_backbone_cnn_grad_f32 call as a CPU tensor [n, L, 5]."""
    xhat, rstd, mask = state
    assert dl.shape == (n, L, 5) and xhat.shape[0] == rstd.shape[0] == mask.shape[0] == n and all(t.is_contiguous() for t in (dl, xhat, rstd, mask))
    lib, nl, dil = _lib.lib(), len(pk["dil"]), _dil(pk)
    (dx,) = _twice("svdd_backbone_cnn_grad_f32",
                   lambda o: lib.svdd_backbone_cnn_grad_f32(dl.data_ptr(), pk["tiles_bwd"].data_ptr(), pk["gamma"].data_ptr(), pk["w2"].data_ptr(),
                                                            pk["table0"].data_ptr(), xhat.data_ptr(), rstd.data_ptr(), mask.data_ptr(), o, n, L, nl,
                                                            dil, _st()), [n * L * 5])
    return dx.cpu(n, L, 5)


def _bits(t):
    return t.contiguous().view(torch.int64 if t.element_size() == 8 else torch.int32)


@functools.lru_cache(maxsize=None)
def _case(L, n, layers):
    """Tokens, the saved state of one real forward launch and Gaussian dlogits (the last of two or more sequences: all zero)."""
    pk, w = _packs(layers)
    tok = _dev(N.tokens(n, L, 3))
    dl = torch.randn(n, L, 5, generator=R._gen(41, L, n, len(pk["dil"])))
    if n > 1:
        dl[n - 1] = 0.0
    return pk, w, _save(pk, tok, n, L), dl


def _check(L, n, layers):
    pk, w, state, dl = _case(L, n, layers)
    nl = len(pk["dil"])
    dld = _dev(dl)
    inputs = {"dlogits": dld, "xhat": state[0], "rstd": state[1], "mask": state[2], "tiles_bwd": pk["tiles_bwd"], "gamma": pk["gamma"],
              "w2": pk["w2"], "table0": pk["table0"]}
    before = {k: _bits(v).clone() for k, v in inputs.items()}
    got = _grad(pk, dld, state, n, L)
    for k, v in inputs.items():
        assert torch.equal(_bits(v), before[k]), f"{k} was modified by the launch"
    masks = B.decode_masks(state[2].cpu(), L)
    assert torch.equal(masks, fused.decode_backbone_masks(state[2], L).cpu()), "the header's mask layout is not decode_backbone_masks'"
    xh, rs = B.decode_xhat(state[0].cpu(), L), state[1].cpu()[:, :, :L].contiguous()
    assert bool(torch.isfinite(xh).all()) and bool((rs > 0).all())
    r64 = R.ref64(B.backbone_grad, dl, masks, xh, rs, w, w["dil"])
    m = min(n, POOL)
    r32 = R.ref32(B.backbone_grad, dl[:m], masks[:m], xh[:m], rs[:m], w, w["dil"])
    tag = f"bb_grad L={L} n={n} nl={nl}"
    cap = 5e-5 * max(1.0, float(r64.abs().max()))
    if m == n:
        _report(tag, got, r64, r32, 8, cap=cap)
    else:
        _report(tag, got, r64, None, 8, cap=cap, pool=(r64[:m], r32))
    assert float(r64.abs().max()) > 1e-3                                # the gradient is not trivially small
    if n > 1:
        assert bool((got[n - 1] == 0).all()), "a sequence with zero dlogits has a non-zero dx"


# 105: the smallest legal L, dilation 64 leaves taps 0, +-1 ; 128: tap +-2 of dilation 64 dead ; 129: alive for one row ; 193: the
# same for tap +-3 ; 200: production ; 207: an odd last row, one padding row ; 208: a full tile, only the zero rows at -1 and 208
# bound the taps
@pytest.mark.parametrize("L,n", [(105, 3), (128, 1), (129, 3), (193, 2), (200, 3), (200, 37), (207, 2), (208, 2)])
def test_backbone_grad_vs_float64_on_the_saved_state(L, n):
    _check(L, n, None)


@pytest.mark.parametrize("L", [200, 105])
@pytest.mark.parametrize("k", sorted(LAYERS))
def test_backbone_grad_other_layer_counts(k, L):
    """nlayers in {1, 2, 5}: the reversed dilation table and the (nl + 1) x 36 schedule at other lengths than 20."""
    _check(L, 2, LAYERS[k])


@pytest.mark.parametrize("L", [105, 200, 207])
def test_backbone_grad_structure_bit_exact(L):
    """Permuting the sequences (dlogits and saved state together) permutes dx ; dx of [a; b] in one launch is dx of a and of b launched
    alone ; and, at L < 208, the rows >= L of the saved state are outside the contract (the header: "values of the zero padding"):
    other finite values in xhat / rstd there and every mask bit of those rows set leave dx's bits alone."""
    n = 3
    pk, _, state, dl = _case(L, n, None)
    dld = _dev(dl)
    base = _grad(pk, dld, state, n, L)
    perm = torch.tensor([2, 0, 1], device=DEV)
    got = _grad(pk, dld[perm].contiguous(), tuple(t[perm].contiguous() for t in state), n, L)
    assert torch.equal(_bits(got), _bits(base[perm.cpu()])), "a permutation of the sequences does not permute dx"
    parts = [_grad(pk, dld[a:b].contiguous(), tuple(t[a:b].contiguous() for t in state), b - a, L) for a, b in ((0, 1), (1, 3))]
    assert torch.equal(_bits(torch.cat(parts)), _bits(base)), "dx of a batch differs from dx of its parts launched alone"
    row, _, valid = B.save_layout()
    pad = valid & (row >= L)
    assert int(pad.sum()) == (208 - L) * 128
    gen = R._gen(42, L)
    xhat, rstd, mask = (t.clone() for t in state)
    xhat[:, :, pad.to(DEV)] = _dev(torch.randn(n, NL, int(pad.sum()), generator=gen) * 3.0)
    rstd[:, :, L:] = _dev(torch.rand(n, NL, 208 - L, generator=gen) * 4.0 + 0.25)
    words = torch.zeros(512, dtype=torch.int64)
    for s in range(56):
        words |= (row[s] >= L).long() << s                              # rows >= 208 too; bits 56 .. 63 stay zero
    mask |= _dev(words)
    got = _grad(pk, dld, (xhat, rstd, mask), n, L)
    assert torch.equal(_bits(got), _bits(base)), "dx depends on the saved state of rows >= L"
