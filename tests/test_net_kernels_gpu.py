"""-m gpu: every entry point of the inference nets (the one-launch backbone, the value net's tower, windows, GRU and tail, and their
split-precision twins; 99 % of a decode's time at the headline configuration) on its own through the C ABI, against the float64
restatement of the operation in tests/net_ref.py, at the shapes that cross the boundaries the launchers of csrc/svdd_nets.hip have.

The backbone has 20 DISTINCT layers (net_ref.distinct_layers): a random-init CNNModel holds 5 groups of 4 equal ones, and a kernel or
packer that takes a layer's weight tiles or bias for its neighbour's inside a group would compute the right answer on it.

Every output sits in a sentinel-filled buffer with guard space on both sides (tests/kernel_harness.py): the guards must be intact,
every element the contract names must be written and no other, and a second launch must give the same bits. Forward results are
continuous in their inputs: no element is excluded from any comparison of this file.

Large batches are built from at most 32 distinct sequences in shuffled order (net_ref.replicated): the references are computed once
per distinct sequence, and every copy must equal its first occurrence bit for bit (the header: a row's result is the same bits
wherever it is evaluated), which also shows that nothing leaks between the sequences of one tile.

Bars are computed here from the references, never from the kernel.
  fp32 kernels: grad_ref.bar(8, ref32, ref64), margin 8 because every operation of this file chains steps or uses a hardware
    transcendental (the towers and the backbone chain layers, the GRU steps, the tail has a LayerNorm's rsqrt in front of two
    products); a bar above the flat tolerance tests/test_fused_gpu.py holds the quantity to (2e-5; the tail 1e-5) is replaced by it.
    Integer outputs (svdd_candidate_windows) and same-bits comparisons are exact.
  lp kernels: against the true float64 reference, bar = min(the tolerance of tests/test_lp_gpu.py, 4 x max|ref_lp - ref64|) (floored
    at 2 ulp of the scale as grad_ref.bar is), ref_lp
    being ref32 with the operands of every matrix product rounded as the header states for the mode; the margin covers the order of
    accumulation and roundings that fall the other way. Logits take TOL_LOGITS and scores TOL_SCORES; tower activations and GRU states
    are O(1) like the logits and take TOL_LOGITS (the x3 GRU: the 5e-5 of test_gru_lp_vs_fp64).
One line `ERR <name> <err> bar <bar>` is printed per comparison."""
import ctypes
import functools

import pytest
import torch

from svdd_amd import _lib, fused
from tests import grad_ref as R
from tests import net_ref as N
from tests.bb_grad_ref import save_layout as _save_layout
from tests.kernel_harness import DEV, _dev, _p, _report, _st, _twice

pytestmark = pytest.mark.gpu
FLAT = 2e-5                                    # tests/test_fused_gpu.py
TOL_LOGITS = {"f16x3": 1e-4, "bf16x3": 1e-4, "f16": 2e-2, "bf16": 1e-1}        # tests/test_lp_gpu.py
TOL_SCORES = {"f16x3": 1e-4, "bf16x3": 1e-4, "f16": 2e-3, "bf16": 1e-2}
TOL_GRU = dict(TOL_LOGITS, f16x3=5e-5, bf16x3=5e-5)
MODES = ("f16x3", "bf16x3", "f16", "bf16")


def _rep(name, got, r64, r32, cap=FLAT, pool=None):
    _report(name, got, r64, r32, 8, cap=cap, pool=pool)


def _rep_lp(name, got, r64, rlp, tol, pool=None):
    err = float((got.double() - r64).abs().max())
    p64, plp = pool if pool else (r64, rlp)
    b = min(tol, max(4.0 * float((plp.double() - p64).abs().max()), 2.0 * R.FP32_EPS * float(p64.abs().max())))   # (grad_ref.bar's floor)
    print(f"ERR {name} {err:.3e} bar {b:.1e}")
    assert err <= b, (name, err, b)


def _firsts(name, got, idx, d):
    """got [n, ...] (CPU) laid out by idx: every copy equals the first occurrence of its row bit for bit -> the d first occurrences."""
    first = torch.full((d,), -1, dtype=torch.long)
    for r in range(idx.numel() - 1, -1, -1):
        first[idx[r]] = r
    assert int(first.min()) >= 0
    bits = got.contiguous().view(torch.int16 if got.element_size() == 2 else torch.int32)
    same = (bits == bits[first[idx]]).flatten(1).all(dim=1)
    assert bool(same.all()), f"{name}: row {int((~same).nonzero()[0])} differs from the first occurrence of the same sequence"
    return got[first]


def _count(k):
    return torch.tensor([k], dtype=torch.int32, device=DEV)


def _rows_mask(n, per_row, rows):
    """Bool [n * per_row]: the elements of the listed rows."""
    m = torch.zeros(n, per_row, dtype=torch.bool)
    m[torch.as_tensor(rows, dtype=torch.long)] = True
    return m.reshape(-1)


# --------------------------------------------------------------------------------------------------------------- backbone
@functools.lru_cache(maxsize=None)
def _cnn():
    """A 20-layer H = 128 backbone with 20 distinct layers, its fp32 operand images, and its natural-layout weights with the time
    biases the kernel is handed."""
    from svdd_amd import backbone, config
    torch.manual_seed(5)
    cnn = N.distinct_layers(backbone.CNNModel(config.dna_config().model, alphabet_size=5).eval(), 7).to(DEV)
    pk = fused.pack_backbone(cnn)
    return cnn, pk, N.backbone_params(cnn, pk["vec"][1:-1, 1])


@functools.lru_cache(maxsize=None)
def _bb_ref(L, d):
    tok = N.tokens(d, L, 0)
    p = _cnn()[2]
    return tok, R.ref64(N.backbone, N.onehot5(tok), p), R.ref32(N.backbone, N.onehot5(tok), p)


def _bb_batch(n, L, dmax=N.MAX_DISTINCT):
    d, idx = N.replicated(n, L, dmax)
    tok, r64, r32 = _bb_ref(L, d)
    return d, idx, tok[idx].contiguous(), r64, r32


def _bb_launch(pk, xd, n, L, count=None, row_idx=None, scatter=0):
    lib, nl = _lib.lib(), len(pk["dil"])
    dil = (ctypes.c_int * nl)(*pk["dil"])
    return lambda o: lib.svdd_backbone_cnn_f32(xd.data_ptr(), pk["table0"].data_ptr(), pk["tiles"].data_ptr(), pk["vec"].data_ptr(),
                                               pk["w2"].data_ptr(), o, n, L, nl, dil, _p(count), _p(row_idx), scatter, _st())


# every L at a ragged n (208: a full tile; 105: the smallest one-sequence tile; 104: two per tile; 33, 9, 1: shorter than the dilations
# 64 / 16: dead taps), every n at L = 200 (257, 300: a tail round after a full round of CUs) and at L = 50 (5: a ragged last tile;
# 1100: the two-size plan of csrc/svdd_spt.h)
BB_CASES = [(7, L) for L in (208, 200, 187, 105, 104, 50, 33, 9, 1)] + [(1, 200), (257, 200), (300, 200), (5, 50), (1100, 50)]


@pytest.mark.parametrize("n,L", BB_CASES)
def test_backbone_f32(n, L):
    """svdd_backbone_cnn_f32 with one workgroup per tile (SVDD_OPT_BACKBONE_SPLIT 1), and svdd_set_backbone_packing(1) on the same
    inputs: same bits."""
    _, pk, _ = _cnn()
    d, idx, tok, r64, r32 = _bb_batch(n, L)
    xd = _dev(tok)
    lib = _lib.lib()
    prev = _lib.set_option(_lib.OPT_BACKBONE_SPLIT, 1)
    try:
        (out,) = _twice("svdd_backbone_cnn_f32", _bb_launch(pk, xd, n, L), [n * L * 5])
        lib.svdd_set_backbone_packing(1)
        (full,) = _twice("svdd_backbone_cnn_f32 packing=1", _bb_launch(pk, xd, n, L), [n * L * 5])
    finally:
        lib.svdd_set_backbone_packing(0)
        _lib.set_option(_lib.OPT_BACKBONE_SPLIT, prev)
    assert torch.equal(out.bits(), full.bits()), "always-full tiles give other bits"
    _rep(f"backbone n={n} L={L}", _firsts("backbone", out.cpu(n, L, 5), idx, d), r64, r32)


@pytest.mark.parametrize("n,L", [(1, 200), (7, 105), (33, 208), (64, 200), (300, 200)])
def test_backbone_f32_on_several_workgroups_per_sequence(n, L):
    """SVDD_OPT_BACKBONE_SPLIT 1 / 2 / 4 and automatic: the same bits, against float64, and no group barrier timed out. (300: the tail
    round of 44 sequences behind a full round goes to the split kernel.)"""
    _, pk, _ = _cnn()
    d, idx, tok, r64, r32 = _bb_batch(n, L)
    xd = _dev(tok)
    fused._backbone_split_workspace(torch.device(DEV))
    outs = {}
    try:
        for split in (1, 2, 4, 0):
            _lib.set_option(_lib.OPT_BACKBONE_SPLIT, split)
            (outs[split],) = _twice(f"svdd_backbone_cnn_f32 split={split}", _bb_launch(pk, xd, n, L), [n * L * 5])
    finally:
        _lib.set_option(_lib.OPT_BACKBONE_SPLIT, 0)
    err = ctypes.c_int(-1)
    _lib.check(_lib.lib().svdd_backbone_split_status(ctypes.byref(err)), "svdd_backbone_split_status")
    assert err.value == 0
    for split in (2, 4, 0):
        assert torch.equal(outs[split].bits(), outs[1].bits()), f"split {split} gives other bits"
    _rep(f"backbone split n={n} L={L}", _firsts("backbone split", outs[4].cpu(n, L, 5), idx, d), r64, r32)


@pytest.mark.parametrize("n,L,k", [(77, 200, 31), (77, 50, 31), (77, 50, 30), (9, 104, 3)])
def test_backbone_f32_count_and_row_idx(n, L, k):
    """count < n alone, with row_idx (compact rows), and with out_scatter: the rows the header says are written hold the float64
    logits of their sequence, every other row of `out` keeps the sentinel — the rest of the last tile too (31 = 7 tiles of four + 3)."""
    _, pk, _ = _cnn()
    d, idx, tok, r64, r32 = _bb_batch(n, L)
    xd, cnt = _dev(tok), _count(k)
    rows = torch.randperm(n, generator=R._gen(16, n, L))[:k].sort().values
    rd = _dev(rows.to(torch.int32))
    (ref,) = _twice("svdd_backbone_cnn_f32", _bb_launch(pk, xd, n, L), [n * L * 5])
    for tag, ridx, scatter, src, dst in (("count", None, 0, torch.arange(k), torch.arange(k)), ("row_idx", rd, 0, rows, torch.arange(k)),
                                         ("scatter", rd, 1, rows, rows)):
        (out,) = _twice(f"svdd_backbone_cnn_f32 {tag}", _bb_launch(pk, xd, n, L, cnt, ridx, scatter), [n * L * 5],
                        written=[_rows_mask(n, L * 5, dst)])
        got = out.cpu(n, L, 5)[dst]
        d2 = idx[src]                                            # the distinct sequence every written row holds
        assert torch.equal(got.view(torch.int32), ref.cpu(n, L, 5)[src].view(torch.int32)), f"{tag}: other bits than the dense launch"
        _rep(f"backbone {tag} n={n} L={L} k={k}", got, r64[d2], r32[d2])


@pytest.mark.parametrize("n,L", [(3, 200), (37, 105), (5, 208)])
def test_backbone_save_f32(n, L):
    """svdd_backbone_cnn_save_f32: the inference kernel's bits in `out`, and xhat / rstd / mask written over exactly the extents the
    header states: mask [n][nl + 2][512] u64 in full (bits 56 .. 63 zero), rstd [n][nl][208] in full (all 208 rows of the tile,
    whatever L is), xhat [n][nl][56][512] in every slot whose row is < 208 and in no other (bb_grad_ref.save_layout). rstd and xhat of the L
    live rows, xhat brought back to [row][channel] by the stated index map, equal float64's 1 / sqrt(var + eps) and LayerNorm'd value
    before the affine map. (The ReLU decisions in mask are discontinuous in the inputs: their values are held by the gradient test of
    tests/test_fused_gpu.py, which decodes them and pins a float64 forward to them.) The same bits on a second launch.
    No older test holds rstd or xhat to a flat tolerance, and neither is of order one (both reach several units): the cap that replaces
    a larger bar is here 2e-5 times the largest float64 value, the flat 2e-5 taken relative to the scale, not the absolute 2e-5 of
    the logits. The rstd bars come out at 4 - 6e-6 and the xhat bars at 4e-5 = 8 x max|ref32 - ref64| (profiles/net_kernels_fp64.txt)."""
    _, pk, p = _cnn()
    d, idx, tok, r64, r32 = _bb_batch(n, L)
    xd = _dev(tok)
    lib, nl = _lib.lib(), len(pk["dil"])
    dil = (ctypes.c_int * nl)(*pk["dil"])
    prev = _lib.set_option(_lib.OPT_BACKBONE_SPLIT, 1)
    try:
        (ref,) = _twice("svdd_backbone_cnn_f32", _bb_launch(pk, xd, n, L), [n * L * 5])
    finally:
        _lib.set_option(_lib.OPT_BACKBONE_SPLIT, prev)
    row, col, valid = _save_layout()
    assert int(valid.sum()) == 208 * 128                          # every (row, channel) of the tile has exactly one slot
    out, xhat, rstd, mask = _twice(
        "svdd_backbone_cnn_save_f32",
        lambda o, xh, rs, mk: lib.svdd_backbone_cnn_save_f32(xd.data_ptr(), pk["table0"].data_ptr(), pk["tiles"].data_ptr(), pk["vec"].data_ptr(),
                                                             pk["w2"].data_ptr(), o, n, L, nl, dil, xh, rs, mk, _st()),
        [n * L * 5, n * nl * 56 * 512, n * nl * 208, n * (nl + 2) * 512 * 2],          # (the u64 mask as pairs of 32-bit words)
        written=[True, valid[None].expand(n * nl, 56, 512), True, True])
    assert torch.equal(out.bits(), ref.bits()), "save: other logits than svdd_backbone_cnn_f32"
    _rep(f"backbone_save out n={n} L={L}", _firsts("save", out.cpu(n, L, 5), idx, d), r64, r32)
    hi_word = mask.bits().cpu().view(n, nl + 2, 512, 2)[..., 1]   # little endian: bits 32 .. 63
    assert bool(((hi_word >> 24) == 0).all()), "mask: a bit beyond the 56 slots is set"

    def stats(onehot, p):
        f = torch.relu(R.conv_same(onehot, p["w_first"], p["b_first"], bias_first=True))
        xs, rs = [], []
        for i, dl in enumerate(p["dil"]):
            xh, r1 = R._ln_stats(f + p["tbs"][i], p["eps"])
            xs.append(xh)
            rs.append(r1[:, :, 0])
            f = torch.relu(N.conv_chunked(xh * p["gammas"][i] + p["betas"][i], p["ws"][i], dl) + p["bs"][i]) + f
        return torch.stack(xs, dim=1), torch.stack(rs, dim=1)    # [d, nl, L, 128], [d, nl, L]
    oh = N.onehot5(_bb_ref(L, d)[0])
    (x64, s64), (x32, s32) = R.ref64(stats, oh, p), R.ref32(stats, oh, p)
    got = _firsts("save rstd", rstd.cpu(n, nl, 208)[:, :, :L].contiguous(), idx, d)
    _rep(f"backbone_save rstd n={n} L={L}", got, s64, s32, cap=FLAT * float(s64.abs().max()))
    img = torch.zeros(n, nl, 208, 128)
    img[:, :, row[valid], col[valid]] = xhat.cpu(n, nl, 56, 512)[:, :, valid]
    got = _firsts("save xhat", img[:, :, :L].contiguous(), idx, d)
    _rep(f"backbone_save xhat n={n} L={L}", got, x64, x32, cap=FLAT * float(x64.abs().max()))


# ------------------------------------------------------------------------------------------------------------ backbone lp
@functools.lru_cache(maxsize=None)
def _bb_lp(mode):
    cnn = _cnn()[0]
    pk = fused.pack_backbone_lp(cnn, mode)
    return pk, N.backbone_params(cnn, pk["vec"][1:-1, 1], pk["lscale"])


@functools.lru_cache(maxsize=None)
def _bb_ref_lp(mode, L, d):
    tok = N.tokens(d, L, 0)
    return N.ref_lp(mode, N.backbone, N.onehot5(tok), _bb_lp(mode)[1])


def _bb_lp_launch(pk, xd, n, L, count=None, row_idx=None, scatter=0):
    lib, nl = _lib.lib(), len(pk["dil"])
    dil = (ctypes.c_int * nl)(*pk["dil"])
    return lambda o: lib.svdd_backbone_cnn_lp(xd.data_ptr(), pk["table0"].data_ptr(), pk["tiles"].data_ptr(), pk["vec"].data_ptr(),
                                              pk["lscale"].data_ptr(), pk["w2"].data_ptr(), o, n, L, nl, dil, pk["prec"], _p(count), _p(row_idx),
                                              scatter, _st())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,L", [(19, 200), (9, 128), (7, 105), (37, 50)])
def test_backbone_lp(mode, n, L):
    """svdd_backbone_cnn_lp, 20 distinct layers, SVDD_OPT_BACKBONE_LP_VERSION 1 and 22 (default), and 21 / 23 where one sequence fills
    a tile (the same bits as 22)."""
    pk, _ = _bb_lp(mode)
    d, idx, tok, r64, _ = _bb_batch(n, L, 8)
    rlp = _bb_ref_lp(mode, L, d)
    xd = _dev(tok)
    outs = {}
    try:
        for v in (22, 1) + ((21, 23) if L > 104 else ()):
            _lib.set_option(_lib.OPT_BACKBONE_LP_VERSION, v)
            (outs[v],) = _twice(f"svdd_backbone_cnn_lp v{v}", _bb_lp_launch(pk, xd, n, L), [n * L * 5])
    finally:
        _lib.set_option(_lib.OPT_BACKBONE_LP_VERSION, 22)
    for v in (21, 23):
        if v in outs:
            assert torch.equal(outs[v].bits(), outs[22].bits()), f"version {v} gives other bits than 22"
    for v in (22, 1):
        _rep_lp(f"backbone_lp {mode} v{v} n={n} L={L}", _firsts("backbone_lp", outs[v].cpu(n, L, 5), idx, d), r64, rlp, TOL_LOGITS[mode])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,L,k", [(77, 200, 31), (77, 50, 31)])
def test_backbone_lp_count_and_row_idx(mode, n, L, k):
    """count / row_idx / out_scatter as for the fp32 kernel, at the default SVDD_OPT_BACKBONE_LP_VERSION only (the row bookkeeping is
    the version's own: L = 200 takes the transposed-accumulator kernel, L = 50 the round-2 one). Versions 21 / 23 are held to 22 bit
    for bit in test_backbone_lp, and 22 to float64."""
    pk, _ = _bb_lp(mode)
    d, idx, tok, r64, _ = _bb_batch(n, L, 8)
    rlp = _bb_ref_lp(mode, L, d)
    xd, cnt = _dev(tok), _count(k)
    rows = torch.randperm(n, generator=R._gen(16, n, L))[:k].sort().values
    rd = _dev(rows.to(torch.int32))
    (ref,) = _twice("svdd_backbone_cnn_lp", _bb_lp_launch(pk, xd, n, L), [n * L * 5])
    for tag, ridx, scatter, src, dst in (("count", None, 0, torch.arange(k), torch.arange(k)), ("row_idx", rd, 0, rows, torch.arange(k)),
                                         ("scatter", rd, 1, rows, rows)):
        (out,) = _twice(f"svdd_backbone_cnn_lp {tag}", _bb_lp_launch(pk, xd, n, L, cnt, ridx, scatter), [n * L * 5],
                        written=[_rows_mask(n, L * 5, dst)])
        got = out.cpu(n, L, 5)[dst]
        assert torch.equal(got.view(torch.int32), ref.cpu(n, L, 5)[src].view(torch.int32)), f"{tag}: other bits than the dense launch"
        _rep_lp(f"backbone_lp {mode} {tag} n={n} L={L} k={k}", got, r64[idx[src]], rlp[idx[src]], TOL_LOGITS[mode])


# ------------------------------------------------------------------------------------------------------------------ tower
@functools.lru_cache(maxsize=None)
def _tower(nl, L, d, resmask):
    stem_w, b, ws = N.tower_inputs(nl, 0)
    tok = N.tokens(d, L, 1)
    args = (N.onehot4(tok), stem_w, b, ws, resmask)
    return tok, (stem_w, b, ws), R.ref64(N.tower, *args), R.ref32(N.tower, *args)


def _tower_launch(tiles, bias, ohd, n, L, nl, resmask, count=None):
    lib = _lib.lib()
    return lambda o: lib.svdd_conv_tower_f32(ohd.data_ptr(), tiles.data_ptr(), bias.data_ptr(), o, n, L, nl, resmask, _p(count), _st())


# L: 208 (a full tile), 105 / 104 (one / two sequences per tile), 1; n ragged against 208 // L sequences per tile
TOWER_SHAPES = [(3, 208), (5, 200), (3, 105), (5, 104), (9, 50), (11, 37), (417, 1), (300, 200)]


# ... and residual patterns other than the net's own, one layer and eight (the entry point's limits) at three of the shapes
TOWER_CASES = [(n, L, 5, 31) for n, L in TOWER_SHAPES] + [(n, L, nl, res) for n, L in ((5, 200), (9, 50), (5, 104))
                                                          for nl, res in ((5, 0b01010), (5, 0), (1, 1), (1, 0), (8, 0b10110101))]


@pytest.mark.parametrize("n,L,nl,resmask", TOWER_CASES)
def test_conv_tower_f32(n, L, nl, resmask):
    """svdd_conv_tower_f32 with svdd_set_tower_version 1, 2, 3 (the same bits), residual_mask patterns other than the net's own, and
    nlayers 1 and 8, the entry point's limits. Then count < n: the rows behind count L keep the sentinel."""
    d, idx = N.replicated(n, L)
    tok, (stem_w, b, ws), r64, r32 = _tower(nl, L, d, resmask)
    tiles, bias, ohd = _dev(fused.pack_tower(stem_w, ws)), _dev(b), _dev(N.onehot4(tok[idx]))
    lib = _lib.lib()
    outs = []
    try:
        for v in (3, 1, 2):
            lib.svdd_set_tower_version(v)
            outs.append(_twice(f"svdd_conv_tower_f32 v{v}", _tower_launch(tiles, bias, ohd, n, L, nl, resmask), [n * L * 64])[0])
        k = max(1, (2 * n) // 3)
        if k < n:
            for v in (3, 1, 2):
                lib.svdd_set_tower_version(v)
                (part,) = _twice(f"svdd_conv_tower_f32 v{v} count", _tower_launch(tiles, bias, ohd, n, L, nl, resmask, _count(k)), [n * L * 64],
                                 written=[_rows_mask(n, L * 64, torch.arange(k))])
                assert torch.equal(part.bits()[:k * L * 64], outs[0].bits()[:k * L * 64])
    finally:
        lib.svdd_set_tower_version(0)
    for o in outs[1:]:
        assert torch.equal(o.bits(), outs[0].bits()), "tower versions differ"
    _rep(f"tower n={n} L={L} nl={nl} res={resmask:#x}", _firsts("tower", outs[0].cpu(n, L, 64), idx, d), r64, r32)


def _window_cases(L):
    """x [B, L], cand [B, M, L]: no change; a change at position 0 / at L - 1 / at both; changes 27 and 28 rows from a tile edge on either
    side (the 16-aligned window gains or loses a tile there); many changes."""
    g = R._gen(17, L)
    pos = [[], [0], [L - 1], [0, L - 1], [16 + 27], [16 + 28], [16 + 26], [L // 2], [max(0, 96 - 28)], [max(0, 96 - 27)], [min(L - 1, 101)],
           sorted(torch.randperm(L, generator=g)[:9].tolist()), [5, 6, 7], []]
    M = 7
    B = len(pos) // M
    x = torch.randint(0, 5, (B, L), generator=g).to(torch.uint8)
    cand = x[:, None, :].repeat(1, M, 1)
    for c, ps in enumerate(pos):
        for q in sorted(set(q for q in ps if q < L)):
            cand[c // M, c % M, q] = (int(cand[c // M, c % M, q]) + 1 + c % 4) % 5
    return x, cand.contiguous(), M


@pytest.mark.parametrize("L", [200, 208, 105, 50, 16, 1])
def test_candidate_windows_exact(L):
    """svdd_candidate_windows against net_ref.windows, integers; flags given and NULL; n = 14 candidates: n % 4 != 0."""
    x, cand, M = _window_cases(L)
    B = x.shape[0]
    n = B * M
    lib, xd, cd = _lib.lib(), _dev(x), _dev(cand)
    for margin in (27, 0, 5):
        want_w, want_f = N.windows(cand, x, margin)
        win, flags = _twice("svdd_candidate_windows", lambda w, f: lib.svdd_candidate_windows(cd.data_ptr(), xd.data_ptr(), B, L, M, margin, w, f, _st()),
                            [(2 * n, torch.int32), (n, torch.int32)])
        assert torch.equal(win.cpu(n, 2), want_w), (win.cpu(n, 2).tolist(), want_w.tolist())
        assert torch.equal(flags.cpu(), want_f)
        (win2,) = _twice("svdd_candidate_windows flags=NULL", lambda w: lib.svdd_candidate_windows(cd.data_ptr(), xd.data_ptr(), B, L, M, margin, w, None, _st()),
                         [(2 * n, torch.int32)])
        assert torch.equal(win2.bits(), win.bits())
    print(f"ERR candidate_windows L={L} 0.000e+00 bar 0.0e+00")


@pytest.mark.parametrize("L", [105, 200, 208])
def test_conv_tower_windows_f32(L):
    """svdd_conv_tower_windows_f32: every row of every candidate against the float64 tower of the candidate; outside its window a row
    is the parent's bits, the whole output the bits of svdd_conv_tower_f32 on the candidates; with live_idx / count workgroup i writes
    rows [i L, (i + 1) L) and nothing behind count L is touched. Versions 1, 2, 3."""
    x, cand, M = _window_cases(L)
    B = x.shape[0]
    n = B * M
    stem_w, b, ws = N.tower_inputs(5, 0)
    tiles, bias = _dev(fused.pack_tower(stem_w, ws)), _dev(b)
    oh = N.onehot4(cand.view(n, L))
    args = (oh, stem_w, b, ws, 31)
    r64, r32 = R.ref64(N.tower, *args), R.ref32(N.tower, *args)
    win, _ = N.windows(cand, x, fused.TOWER_WINDOW_MARGIN)
    lib, ohd, wd, pod = _lib.lib(), _dev(oh), _dev(win), _dev(N.onehot4(x))
    live = torch.tensor([12, 3, 0, 8, 13, 5], dtype=torch.int32)
    k = 4
    try:
        for v in (3, 1, 2):
            lib.svdd_set_tower_version(v)
            (parent,) = _twice("svdd_conv_tower_f32 parents", _tower_launch(tiles, bias, pod, B, L, 5, 31), [B * L * 64])
            (full,) = _twice("svdd_conv_tower_f32 candidates", _tower_launch(tiles, bias, ohd, n, L, 5, 31), [n * L * 64])
            pb = parent.body()

            def launch(o, nn=n, li=None, cnt=None):
                return lib.svdd_conv_tower_windows_f32(ohd.data_ptr(), tiles.data_ptr(), bias.data_ptr(), wd.data_ptr(), pb.data_ptr(), o, nn, L, M, 5, 31,
                                                       _p(li), _p(cnt), _st())
            (out,) = _twice(f"svdd_conv_tower_windows_f32 v{v}", launch, [n * L * 64])
            got, par = out.cpu(n, L, 64), parent.cpu(B, L, 64)
            assert torch.equal(out.bits(), full.bits()), "windows: other bits than the full tower"
            for c in range(n):
                outside = torch.ones(L, dtype=torch.bool)
                outside[int(win[c, 0]):int(win[c, 1])] = False
                assert torch.equal(got[c][outside].view(torch.int32), par[c // M][outside].view(torch.int32)), f"candidate {c}: a row outside its window"
            _rep(f"tower_windows v{v} L={L}", got, r64, r32)
            ld = _dev(live)
            (comp,) = _twice(f"svdd_conv_tower_windows_f32 v{v} live_idx", lambda o: launch(o, len(live), ld, _count(k)), [n * L * 64],
                             written=[_rows_mask(n, L * 64, torch.arange(k))])
            assert torch.equal(comp.cpu(n, L, 64)[:k].view(torch.int32), got[live[:k].long()].view(torch.int32))
    finally:
        lib.svdd_set_tower_version(0)


# --------------------------------------------------------------------------------------------------------------------- GRU
@functools.lru_cache(maxsize=None)
def _gru(L, d):
    """nn.GRU weights x 2 (saturating gates), non-negative inputs (as after the tower's ReLU), float64 and fp32 restatements."""
    mod, x, _ = R.gru_inputs(d, L)
    with torch.no_grad():
        for prm in mod.parameters():
            prm.mul_(2.0)
    w = R.gru_weights_of(mod)
    return mod, x, w, R.ref64(N.gru_out, x, w), R.ref32(N.gru_out, x, w)


def _by_dir(t):
    """[2, n, L, 64] -> [n, 2, L, 64] (rows first, for the per-row checks)."""
    return t.transpose(0, 1).contiguous()


# every n at one L (tiles of 16 sequences with 1 - 15 live rows), every L at one ragged n, the headline shape, and mode 2 where the
# launcher takes it (n >= 256)
GRU_CASES = ([(n, 7, m) for n in (1, 15, 16, 17, 300) for m in (0, 1)] + [(17, L, m) for L in (1, 2, 50, 200) for m in (0, 1)] +
             [(2560, 200, 0), (2560, 200, 2), (300, 7, 2), (300, 50, 2), (2560, 7, 1)])


@pytest.mark.parametrize("n,L,mode", GRU_CASES)
def test_gru_bidir_f32(n, L, mode):
    """svdd_gru_bidir_f32 in svdd_gru_set_mode 0 / 1 / 2: all sequences against float64; count < n leaves the rest untouched."""
    d, idx = N.replicated(n, L)
    mod, x, w, r64, r32 = _gru(L, d)
    wpack, bpack = (_dev(t) for t in fused.pack_gru(mod))
    xd = _dev(x[idx])
    lib = _lib.lib()
    k = max(1, (2 * n) // 3)
    both = torch.zeros(2, n, L * 64, dtype=torch.bool)
    both[:, :k] = True
    try:
        lib.svdd_gru_set_mode(mode)
        (out,) = _twice(f"svdd_gru_bidir_f32 mode={mode}", lambda o: lib.svdd_gru_bidir_f32(xd.data_ptr(), wpack.data_ptr(), bpack.data_ptr(), o, n, L, None, _st()),
                        [2 * n * L * 64])
        if k < n:
            cnt = _count(k)
            (part,) = _twice(f"svdd_gru_bidir_f32 mode={mode} count", lambda o: lib.svdd_gru_bidir_f32(xd.data_ptr(), wpack.data_ptr(), bpack.data_ptr(), o, n, L,
                                                                                                     cnt.data_ptr(), _st()), [2 * n * L * 64], written=[both])
            assert torch.equal(part.body().view(2, n, -1)[:, :k], out.body().view(2, n, -1)[:, :k])
    finally:
        lib.svdd_gru_set_mode(0)
    got = _firsts("gru", _by_dir(out.cpu(2, n, L, 64)), idx, d)
    _rep(f"gru mode={mode} n={n} L={L}", got, _by_dir(r64), _by_dir(r32))


# -------------------------------------------------------------------------------------------------------------------- tail
@pytest.mark.parametrize("T", [1, 2, 3, 4])
@pytest.mark.parametrize("n,L", [(1, 1), (5, 17), (6, 200), (7, 200), (64, 17), (303, 1), (41, 200)])
def test_value_tail_f32(n, L, T):
    """svdd_value_tail_f32 on pack_tail's operands (the LayerNorm affine folded by the packer) against the float64 tail of the natural
    weights; n % 4 = 1, 2, 3, 0; count < n. A launch has n T outputs — one number at (1, 1, 1), whose |ref32 - ref64| says nothing
    about the arithmetic's error — so the references are computed for 32 sequences of the case's generator, the launch takes the
    first min(n, 32) of them, and the bar is the one of all 32."""
    d, idx = N.replicated(n, L)
    h, w1, b1, gam, bet, w_eff, b_eff = N.tail_inputs(N.MAX_DISTINCT, L, T)
    args = (h[0], h[1], w1, b1, gam, bet, w_eff, b_eff)
    r64, r32 = R.ref64(N.tail, *args), R.ref32(N.tail, *args)
    wp, bf = (_dev(t) for t in fused.pack_tail(w1, b1, gam, bet))
    hd, wd, bd = _dev(h[:, idx]), _dev(w_eff), _dev(b_eff)
    lib = _lib.lib()

    def launch(o, cnt=None):
        return lib.svdd_value_tail_f32(hd[0].data_ptr(), hd[1].data_ptr(), wp.data_ptr(), bf.data_ptr(), wd.data_ptr(), bd.data_ptr(), o, n, L, T, _p(cnt), _st())
    (out,) = _twice("svdd_value_tail_f32", launch, [n * T])
    k = max(1, (2 * n) // 3)
    if k < n:
        cnt = _count(k)
        (part,) = _twice("svdd_value_tail_f32 count", lambda o: launch(o, cnt), [n * T], written=[_rows_mask(n, T, torch.arange(k))])
        assert torch.equal(part.bits()[:k * T], out.bits()[:k * T])
    _rep(f"tail n={n} L={L} T={T}", _firsts("tail", out.cpu(n, T), idx, d), r64[:d], r32[:d], cap=1e-5 * max(1.0, float(r64.abs().max())),
         pool=(r64, r32))


# ---------------------------------------------------------------------------------------------------------- the whole net
@pytest.mark.parametrize("n,L", [(37, 200), (5, 50), (300, 50)])
def test_value_net_scores_vs_float64(n, L):
    """FusedValueNet (tower, GRU and tail kernels in a row, BatchNorm folded by the module) against the float64 restatement of the whole
    net on the natural weights: the scores are below 0.1 with a spread of a few 1e-3 between sequences, of which the flat 2e-5 they
    were held to is a visible fraction; the bar here comes out near 2e-7."""
    from svdd_amd.value_nets import ConvGRUTrunk, ConvHead
    torch.manual_seed(44)
    emb, head = N.distinct_layers(ConvGRUTrunk().eval(), 9), ConvHead(1, 64).eval()
    p = N.value_params(emb, head)
    d, idx = N.replicated(n, L)
    oh = N.onehot4(N.tokens(d, L, 2))
    r64, r32 = R.ref64(N.value_net, oh, p), R.ref32(N.value_net, oh, p)
    fv = fused.FusedValueNet(emb.to(DEV), head.to(DEV)).to(DEV).eval()
    assert fv.tower_ok and fv.tail_ok
    with torch.no_grad():
        got = fv(_dev(oh[idx])).reshape(n, 1).cpu()
        assert torch.equal(got, fv(_dev(oh[idx])).reshape(n, 1).cpu())
    _rep(f"value_net n={n} L={L}", _firsts("value_net", got, idx, d), r64, r32)


# ------------------------------------------------------------------------------------------- split-precision value net
def _planes(buf, n, L, P):
    """[n, L, P, 64] 16-bit planes -> hi + lo as fp32 [n, L, 64]."""
    return buf.cpu(n, L, P, 64).float().sum(dim=2)


def _tower_lp_launch(tiles, bias, inv, tokd, n, L, nl, resmask, prec, count=None):
    lib = _lib.lib()
    return lambda o: lib.svdd_conv_tower_lp(tokd.data_ptr(), tiles.data_ptr(), bias.data_ptr(), inv.data_ptr(), o, n, L, nl, resmask, _p(count), prec, _st())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,L", [(3, 208), (5, 200), (3, 105), (5, 104), (9, 50), (11, 37), (417, 1)])
def test_conv_tower_lp(mode, n, L):
    """svdd_conv_tower_lp: the 16-bit plane outputs compared as hi + lo with the float64 tower; count < n."""
    dtype, parts = fused.LP_DTYPES[mode]
    d, idx = N.replicated(n, L, 8)
    tok, (stem_w, b, ws), r64, _ = _tower(5, L, d, 31)
    tiles, inv = (_dev(t) for t in fused.pack_tower_lp(stem_w, ws, mode))
    rlp = N.ref_lp(mode, N.tower, N.onehot4(tok), stem_w, b, ws, 31, inv.cpu())
    bias, tokd, prec = _dev(b), _dev(tok[idx]), _lib.PRECISIONS[mode]
    (out,) = _twice("svdd_conv_tower_lp", _tower_lp_launch(tiles, bias, inv, tokd, n, L, 5, 31, prec), [(n * L * parts * 64, dtype)])
    k = max(1, (2 * n) // 3)
    (part,) = _twice("svdd_conv_tower_lp count", _tower_lp_launch(tiles, bias, inv, tokd, n, L, 5, 31, prec, _count(k)), [(n * L * parts * 64, dtype)],
                     written=[_rows_mask(n, L * parts * 64, torch.arange(k))])
    assert torch.equal(part.bits()[:k * L * parts * 64], out.bits()[:k * L * parts * 64])
    _firsts("tower_lp planes", out.cpu(n, L * parts * 64), idx, d)
    _rep_lp(f"tower_lp {mode} n={n} L={L}", _firsts("tower_lp", _planes(out, n, L, parts), idx, d), r64, rlp, TOL_LOGITS[mode])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("L", [105, 200, 208])
def test_conv_tower_windows_lp(mode, L):
    """svdd_conv_tower_windows_lp: as the fp32 windows kernel — float64 on every row, the parent's bits outside the window, the full lp
    tower's bits everywhere, live_idx / count."""
    dtype, parts = fused.LP_DTYPES[mode]
    x, cand, M = _window_cases(L)
    B = x.shape[0]
    n = B * M
    stem_w, b, ws = N.tower_inputs(5, 0)
    tiles, inv = (_dev(t) for t in fused.pack_tower_lp(stem_w, ws, mode))
    oh = N.onehot4(cand.view(n, L))
    r64 = R.ref64(N.tower, oh, stem_w, b, ws, 31)
    rlp = N.ref_lp(mode, N.tower, oh, stem_w, b, ws, 31, inv.cpu())
    win, _ = N.windows(cand, x, fused.TOWER_WINDOW_MARGIN)
    lib, bias, cd, xd, wd, prec = _lib.lib(), _dev(b), _dev(cand), _dev(x), _dev(win), _lib.PRECISIONS[mode]
    row = L * parts * 64
    (parent,) = _twice("svdd_conv_tower_lp parents", _tower_lp_launch(tiles, bias, inv, xd, B, L, 5, 31, prec), [(B * row, dtype)])
    (full,) = _twice("svdd_conv_tower_lp candidates", _tower_lp_launch(tiles, bias, inv, cd, n, L, 5, 31, prec), [(n * row, dtype)])
    pb = parent.body()

    def launch(o, li=None, cnt=None):
        return lib.svdd_conv_tower_windows_lp(cd.data_ptr(), tiles.data_ptr(), bias.data_ptr(), inv.data_ptr(), wd.data_ptr(), pb.data_ptr(), o, n, L, M, 5, 31,
                                              _p(li), _p(cnt), prec, _st())
    (out,) = _twice("svdd_conv_tower_windows_lp", launch, [(n * row, dtype)])
    assert torch.equal(out.bits(), full.bits()), "windows: other bits than the full tower"
    got, par = out.cpu(n, L, parts * 64).view(torch.int16), parent.cpu(B, L, parts * 64).view(torch.int16)
    for c in range(n):
        outside = torch.ones(L, dtype=torch.bool)
        outside[int(win[c, 0]):int(win[c, 1])] = False
        assert torch.equal(got[c][outside], par[c // M][outside]), f"candidate {c}: a row outside its window"
    _rep_lp(f"tower_windows_lp {mode} L={L}", _planes(out, n, L, parts), r64, rlp, TOL_LOGITS[mode])
    live, k = torch.tensor([12, 3, 0, 8, 13, 5], dtype=torch.int32), 4
    ld = _dev(live)
    (comp,) = _twice("svdd_conv_tower_windows_lp live_idx", lambda o: launch(o, ld, _count(k)), [(n * row, dtype)],
                     written=[_rows_mask(n, row, torch.arange(k))])
    assert torch.equal(comp.cpu(n, L, parts * 64).view(torch.int16)[:k], got[live[:k].long()])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,L", [(1, 7), (17, 7), (300, 7), (17, 1), (17, 50), (16, 200), (300, 50)])
def test_gru_bidir_lp(mode, n, L):
    """svdd_gru_bidir_lp from the fp32 input and from 16-bit planes (the reference then takes hi + lo as its input); count < n."""
    dtype, parts = fused.LP_DTYPES[mode]
    d, idx = N.replicated(n, L, 8)
    mod, x, w, r64, _ = _gru(L, d)
    wp, bp, inv = (_dev(t) for t in fused.pack_gru_lp(mod, mode))
    rlp = N.ref_lp(mode, N.gru_out_lp, x, w, inv.cpu())
    lib, prec, xd = _lib.lib(), _lib.PRECISIONS[mode], _dev(x[idx])
    k = max(1, (2 * n) // 3)
    both = torch.zeros(2, n, L * 64, dtype=torch.bool)
    both[:, :k] = True

    def launch(o, x32, x16, cnt=None):
        return lib.svdd_gru_bidir_lp(_p(x32), _p(x16), wp.data_ptr(), bp.data_ptr(), inv.data_ptr(), o, n, L, _p(cnt), prec, _st())
    (out,) = _twice("svdd_gru_bidir_lp", lambda o: launch(o, xd, None), [2 * n * L * 64])
    if k < n:
        cnt = _count(k)
        (part,) = _twice("svdd_gru_bidir_lp count", lambda o: launch(o, xd, None, cnt), [2 * n * L * 64], written=[both])
        assert torch.equal(part.body().view(2, n, -1)[:, :k], out.body().view(2, n, -1)[:, :k])
    _rep_lp(f"gru_lp {mode} n={n} L={L}", _firsts("gru_lp", _by_dir(out.cpu(2, n, L, 64)), idx, d), _by_dir(r64), _by_dir(rlp), TOL_GRU[mode])
    planes = fused._split16(x, dtype, parts).permute(0, 1, 3, 2).contiguous()              # [d, L, P, 64]
    xq = planes.float().sum(dim=2)
    q64, qlp = R.ref64(N.gru_out, xq, w), N.ref_lp(mode, N.gru_out_lp, xq, w, inv.cpu())
    pd = _dev(planes[idx])
    (out16,) = _twice("svdd_gru_bidir_lp x16", lambda o: launch(o, None, pd), [2 * n * L * 64])
    _rep_lp(f"gru_lp {mode} x16 n={n} L={L}", _firsts("gru_lp x16", _by_dir(out16.cpu(2, n, L, 64)), idx, d), _by_dir(q64), _by_dir(qlp), TOL_GRU[mode])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,L,T", [(1, 1, 1), (5, 17, 2), (6, 200, 3), (7, 200, 4), (64, 17, 1), (41, 200, 1)])
def test_value_tail_lp(mode, n, L, T):
    """svdd_value_tail_lp. TOL_SCORES is an absolute tolerance set at the value net's score magnitude (< 0.1): on scores of order 1
    from a single row the one-pass f16 arithmetic itself — kernel and ref_lp agreed to four digits, 3.065e-3 — is beyond it. So every
    mode runs on weights drawn at the default initialisation's scale and collapsed as the net collapses them (net_ref.tail_inputs,
    net_scale), and the x3 modes, whose error stays below the cap there, ALSO on the order-one inputs of test_value_tail_f32.
    References and bar over 32 sequences as in test_value_tail_f32."""
    d, idx = N.replicated(n, L)
    lib, prec = _lib.lib(), _lib.PRECISIONS[mode]
    for net_scale in ((True, False) if mode in ("f16x3", "bf16x3") else (True,)):
        h, w1, b1, gam, bet, w_eff, b_eff = N.tail_inputs(N.MAX_DISTINCT, L, T, net_scale=net_scale)
        args = (h[0], h[1], w1, b1, gam, bet, w_eff, b_eff)
        wp, bf, inv = fused.pack_tail_lp(w1, b1, gam, bet, mode)
        r64, rlp = R.ref64(N.tail, *args), N.ref_lp(mode, N.tail, *args, 1e-5, inv)
        wp, bf, hd, wd, bd = _dev(wp), _dev(bf), _dev(h[:, idx]), _dev(w_eff), _dev(b_eff)

        def launch(o, cnt=None):
            return lib.svdd_value_tail_lp(hd[0].data_ptr(), hd[1].data_ptr(), wp.data_ptr(), bf.data_ptr(), wd.data_ptr(), bd.data_ptr(), float(inv), o, n, L, T,
                                          _p(cnt), prec, _st())
        (out,) = _twice("svdd_value_tail_lp", launch, [n * T])
        k = max(1, (2 * n) // 3)
        if k < n:
            cnt = _count(k)
            (part,) = _twice("svdd_value_tail_lp count", lambda o: launch(o, cnt), [n * T], written=[_rows_mask(n, T, torch.arange(k))])
            assert torch.equal(part.bits()[:k * T], out.bits()[:k * T])
        _rep_lp(f"tail_lp {mode} {'net' if net_scale else 'unit'}-scale n={n} L={L} T={T}", _firsts("tail_lp", out.cpu(n, T), idx, d), r64[:d], rlp[:d],
                TOL_SCORES[mode], pool=(r64, rlp))
