"""-m gpu: the net kernels that put SEVERAL sequences into one workgroup tile (L <= 104) at every packing and length class. The
fp32 backbone interleaves the s sequences of a tile position-major and multiplies every dilation by s; its tap liveness, zero padding,
entry body (2 / 4 / 7 row-tile slots) and the slots a wave half owns all come from s L; the towers, the round-2 lp backbone and the
generic convolution stack the sequences and keep a tap inside its sequence by a position test per row. The other files run this
code at L = 104, 50, 37, 33, 9, 1 with full tiles or the planner's choice; here: every length of short_lengths_ref.SHORT_LENS
(tests/test_short_lengths_cpu.py proves which classes they reach) at the forced packings packs(L) = {1, 2, 3, 4, smax - 1, smax}
(svdd_set_backbone_packing(-s)), batches of at most 32 distinct sequences in shuffled order (every copy equals its first occurrence
bit for bit: nothing leaks between the sequences of a tile), every output in sentinel-guarded buffers, every launch twice.
  per L
    backbone        svdd_backbone_cnn_f32, 20 distinct layers. Forced s, n = 2 s + 1 (two full tiles and one sequence) and, s >= 3,
                    2 s - 1 (the last tile lacks exactly one): s = 1 against net_ref.backbone in float64, bar(8, ref32, ref64) capped at
                    2e-5; every other s, full tiles (packing 1) and the planner (packing 0): the bits of s = 1. A batch larger than the
                    CU count (the planner takes several per tile): the same; then count = k < n, count with row_idx, with out_scatter,
                    at packing 0 (the plan is made on the device) and at the largest s, k such that the last live tile is ragged:
                    exactly the rows the header names hold the plain launch's bits, every other element keeps the sentinel.
                    A forced s = 1 (and the planner on these small batches) runs the one-sequence form backbone_kernel<true>: it is
                    the reference, not a case. So also: packing 0 with a device-side count k <= CUs (what a work-skipping launch with
                    few live rows is) — the workgroups plan ONE sequence per tile from L = 9 up and backbone_kernel<false> runs
                    tiles of L rows (il = 1, nt = ceil(L / 16)) — count = n, count = k < n, row_idx, out_scatter: the bits of s = 1
    backbone_lp     svdd_backbone_cnn_lp in f16x3 / bf16x3 / f16 / bf16, SVDD_OPT_BACKBONE_LP_VERSION 22 (interleaved) and 1 (stacked):
                    the same packings and batches against float64 under test_net_kernels_gpu._rep_lp's bar; inside a version every
                    packing the same bits; count / row_idx / out_scatter at the default packing, on the large batch and on the
                    small device-side count
    tower           svdd_conv_tower_f32 versions 1 / 2 / 3 (same bits) against net_ref.tower, n = 2 (208 // L) + 1 and (208 // L) - 1,
                    count < n; at L = 104, 50, 33 the other residual masks and layer counts of TOWER_CASES too
    tower_lp        svdd_conv_tower_lp in the four modes, hi + lo against float64, count < n
  L = 104, 69, 33   two tile sizes in one launch: an n whose plan (the numpy restatement of csrc/svdd_spt.h at this device's CU
                    count) has n1 > 0 and s1 != s2, host-side plan and device-side plan (count = n): the bits of s = 1
  per L in CONV_LENS  svdd_conv1d_cl_f32 on the generic kernel (svdd_conv1d_set_dynamic(1)), cin = cout 64 / 128, 9 and 5 taps,
                    dilations 1, 4, 16, 64, n = 2 (224 // L) + 1, against bb_grad_ref.conv_dilated, margin 4, cap 2e-5
No element is excluded from any comparison. Bars come from the references (profiles/short_length_sweep_fp64.txt holds a run's
lines); what each check catches is on record in profiles/short_tile_teeth.txt (tools/stem_tower_teeth.py, family `short*`)."""
import functools

import pytest
import torch

from svdd_amd import _lib, fused
from tests import bb_grad_ref as B
from tests import grad_ref as R
from tests import net_ref as N
from tests import short_lengths_ref as S
from tests.kernel_harness import _dev, _report, _twice
from tests.test_conv_epilogue_kernels_gpu import FLAT_Y, _conv, _conv_inputs
from tests.test_net_kernels_gpu import (MODES, TOL_LOGITS, TOWER_CASES, _bb_launch, _bb_lp, _bb_lp_launch, _bb_ref, _bb_ref_lp, _cnn,
                                        _count, _firsts, _planes, _rep, _rep_lp, _rows_mask, _tower, _tower_launch, _tower_lp_launch)

pytestmark = pytest.mark.gpu


def _exact(name):
    print(f"ERR {name} 0.000e+00 bar 0.0e+00")


@functools.lru_cache(maxsize=None)
def _ncu():
    return _lib.device_info()[1]


def _distinct(L, rows=S.TILE_ROWS):
    """Distinct sequences of length L: as many as the largest small batch (two full tiles and one sequence), at most 32."""
    return min(N.MAX_DISTINCT, 2 * (rows // L) + 1)


def _batch(n, L, D):
    """-> (d, idx): n rows from the first d = min(n, D) distinct sequences, shuffled."""
    return N.replicated(n, L, D)


def _small_batches(L):
    """[(n, [s ..])]: every n of the forced packings with the packings that run on it."""
    by = {}
    for s in S.packs(L):
        for n in S.batch_sizes(s):
            by.setdefault(n, []).append(s)
    return sorted(by.items())


def _large(L):
    """(n, k): a batch beyond the CU count and a live count whose last tile is ragged at the device's plan and at full tiles."""
    k = S.ragged_count(L, _ncu())
    assert k is not None and k % (S.TILE_ROWS // L), (L, _ncu())
    s1, n1, s2 = S.plan_tiles(k, L, _ncu(), 9)
    assert s2 > 1 and (k - n1 * s1) % s2, "the planner's last live tile is not ragged"
    return k + S.TILE_ROWS // L + 1, k


def _indexed(n, k, L):
    """The three ways a launch names k < n live rows: (tag, row_idx, scatter, source rows, written rows)."""
    rows = torch.randperm(n, generator=R._gen(16, n, L))[:k].sort().values
    rd = _dev(rows.to(torch.int32))
    return (("count", None, 0, torch.arange(k), torch.arange(k)), ("row_idx", rd, 0, rows, torch.arange(k)), ("scatter", rd, 1, rows, rows))


# --------------------------------------------------------------------------------------------------------- backbone, fp32
@pytest.mark.parametrize("L", S.SHORT_LENS)
def test_backbone_f32(L):
    _, pk, _ = _cnn()
    D = _distinct(L)
    tok, r64, r32 = _bb_ref(L, D)
    lib, smax = _lib.lib(), S.TILE_ROWS // L
    nb, k = _large(L)
    try:
        for n, forced in _small_batches(L) + [(nb, [smax])]:
            d, idx = _batch(n, L, D)
            xd = _dev(tok[idx])
            lib.svdd_set_backbone_packing(-1)
            (one,) = _twice("svdd_backbone_cnn_f32 s=1", _bb_launch(pk, xd, n, L), [n * L * 5])
            _rep(f"backbone L={L} s=1 n={n}", _firsts("backbone", one.cpu(n, L, 5), idx, d), r64[:d], r32[:d], pool=(r64, r32))
            for s in [-s for s in forced if s > 1] + [1, 0]:
                lib.svdd_set_backbone_packing(s)
                (out,) = _twice(f"svdd_backbone_cnn_f32 packing={s}", _bb_launch(pk, xd, n, L), [n * L * 5])
                assert torch.equal(out.bits(), one.bits()), f"L = {L}, n = {n}: packing {s} gives other bits than one sequence per tile"
            _exact(f"backbone L={L} n={n} s={forced}, full, planner == s=1")
        # n = nb: count / row_idx / out_scatter on the device's plan and on full tiles
        plain = one.cpu(nb, L, 5)
        for s in (0, -smax):
            lib.svdd_set_backbone_packing(s)
            for tag, ridx, scatter, src, dst in _indexed(nb, k, L):
                (out,) = _twice(f"svdd_backbone_cnn_f32 packing={s} {tag}", _bb_launch(pk, xd, nb, L, _count(k), ridx, scatter), [nb * L * 5],
                                written=[_rows_mask(nb, L * 5, dst)])
                assert torch.equal(out.cpu(nb, L, 5)[dst].view(torch.int32), plain[src].view(torch.int32)), \
                    f"L = {L}, packing {s}, {tag}: other bits than the dense launch"
        _exact(f"backbone L={L} n={nb} k={k} count / row_idx / scatter, planner and s={smax} == dense")
        # a device-side count of at most one round of rows: backbone_kernel<false> on the tile size the workgroups plan (one sequence)
        n0, k0 = 2 * smax + 1, S.small_count(L, _ncu())
        s0 = S.small_spt(L, _ncu())
        assert k0 <= _ncu() and k0 < n0 and s0 == (1 if L >= 9 else 16 // L)
        d, idx = _batch(n0, L, D)
        xd = _dev(tok[idx])
        lib.svdd_set_backbone_packing(-1)
        (one,) = _twice("svdd_backbone_cnn_f32 s=1", _bb_launch(pk, xd, n0, L), [n0 * L * 5])
        plain = one.cpu(n0, L, 5)
        lib.svdd_set_backbone_packing(0)
        if n0 <= _ncu():
            (out,) = _twice("svdd_backbone_cnn_f32 device plan, count = n", _bb_launch(pk, xd, n0, L, _count(n0)), [n0 * L * 5])
            assert torch.equal(out.bits(), one.bits()), f"L = {L}: the device's plan of {n0} rows gives other bits than the one-sequence form"
        for tag, ridx, scatter, src, dst in _indexed(n0, k0, L):
            (out,) = _twice(f"svdd_backbone_cnn_f32 device plan {tag}", _bb_launch(pk, xd, n0, L, _count(k0), ridx, scatter), [n0 * L * 5],
                            written=[_rows_mask(n0, L * 5, dst)])
            assert torch.equal(out.cpu(n0, L, 5)[dst].view(torch.int32), plain[src].view(torch.int32)), \
                f"L = {L}, device plan of {k0} rows ({s0} per tile), {tag}: other bits than the one-sequence form"
        _exact(f"backbone L={L} n={n0} device count {n0 if n0 <= _ncu() else k0} / {k0} ({s0} per tile), row_idx, scatter == s=1")
    finally:
        lib.svdd_set_backbone_packing(0)


@pytest.mark.parametrize("L", S.TWO_SIZE_LENS)
def test_backbone_f32_two_tile_sizes(L):
    """One launch that mixes two tile sizes, planned on the host and (count = n) by the workgroups themselves."""
    _, pk, _ = _cnn()
    n = S.two_size_batch(L, _ncu())
    assert n is not None
    s1, n1, s2 = S.plan_tiles(n, L, _ncu(), 9)
    assert n1 > 0 and s1 != s2 and S.plan_num_tiles((s1, n1, s2), n) > n1, f"L = {L}: the plan of n = {n} has one tile size"
    D = _distinct(L)
    tok, r64, r32 = _bb_ref(L, D)
    d, idx = _batch(n, L, D)
    xd = _dev(tok[idx])
    lib = _lib.lib()
    try:
        lib.svdd_set_backbone_packing(-1)
        (one,) = _twice("svdd_backbone_cnn_f32 s=1", _bb_launch(pk, xd, n, L), [n * L * 5])
        lib.svdd_set_backbone_packing(0)
        (host,) = _twice("svdd_backbone_cnn_f32 host plan", _bb_launch(pk, xd, n, L), [n * L * 5])
        (dev,) = _twice("svdd_backbone_cnn_f32 device plan", _bb_launch(pk, xd, n, L, _count(n)), [n * L * 5])
    finally:
        lib.svdd_set_backbone_packing(0)
    _rep(f"backbone two sizes L={L} n={n} plan={s1}x{n1}+{s2}", _firsts("backbone", one.cpu(n, L, 5), idx, d), r64[:d], r32[:d], pool=(r64, r32))
    assert torch.equal(host.bits(), one.bits()), f"L = {L}, n = {n}: the host's two-size plan gives other bits than one sequence per tile"
    assert torch.equal(dev.bits(), one.bits()), f"L = {L}, n = {n}: the device's two-size plan gives other bits than one sequence per tile"
    _exact(f"backbone two sizes L={L} n={n} host plan, device plan == s=1")


# ----------------------------------------------------------------------------------------------------------- backbone, lp
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("L", S.SHORT_LENS)
def test_backbone_lp(L, mode):
    pk, _ = _bb_lp(mode)
    D = _distinct(L)
    tok, r64, _ = _bb_ref(L, D)
    rlp = _bb_ref_lp(mode, L, D)
    lib = _lib.lib()
    nb, k = _large(L)
    try:
        for v in (22, 1):
            _lib.set_option(_lib.OPT_BACKBONE_LP_VERSION, v)
            for n, forced in _small_batches(L):
                d, idx = _batch(n, L, D)
                xd = _dev(tok[idx])
                lib.svdd_set_backbone_packing(-1)
                (one,) = _twice(f"svdd_backbone_cnn_lp v{v} s=1", _bb_lp_launch(pk, xd, n, L), [n * L * 5])
                _rep_lp(f"backbone_lp {mode} v{v} L={L} s=1 n={n}", _firsts("backbone_lp", one.cpu(n, L, 5), idx, d), r64[:d], rlp[:d], TOL_LOGITS[mode], pool=(r64, rlp))
                for s in [-s for s in forced if s > 1] + [1, 0]:
                    lib.svdd_set_backbone_packing(s)
                    (out,) = _twice(f"svdd_backbone_cnn_lp v{v} packing={s}", _bb_lp_launch(pk, xd, n, L), [n * L * 5])
                    assert torch.equal(out.bits(), one.bits()), f"L = {L}, {mode}, v{v}, n = {n}: packing {s} gives other bits than one sequence per tile"
            # the default packing on a batch beyond the CU count: dense, then count / row_idx / out_scatter
            lib.svdd_set_backbone_packing(0)
            d, idx = _batch(nb, L, D)
            xd = _dev(tok[idx])
            (dense,) = _twice(f"svdd_backbone_cnn_lp v{v}", _bb_lp_launch(pk, xd, nb, L), [nb * L * 5])
            plain = dense.cpu(nb, L, 5)
            _rep_lp(f"backbone_lp {mode} v{v} L={L} n={nb}", _firsts("backbone_lp", plain, idx, d), r64[:d], rlp[:d], TOL_LOGITS[mode], pool=(r64, rlp))
            for tag, ridx, scatter, src, dst in _indexed(nb, k, L):
                (out,) = _twice(f"svdd_backbone_cnn_lp v{v} {tag}", _bb_lp_launch(pk, xd, nb, L, _count(k), ridx, scatter), [nb * L * 5],
                                written=[_rows_mask(nb, L * 5, dst)])
                assert torch.equal(out.cpu(nb, L, 5)[dst].view(torch.int32), plain[src].view(torch.int32)), \
                    f"L = {L}, {mode}, v{v}, {tag}: other bits than the dense launch"
            # a device-side count of at most one round of rows (the workgroups plan the tile size), against the forced s = 1
            n0, k0 = 2 * (S.TILE_ROWS // L) + 1, S.small_count(L, _ncu())
            d, idx = _batch(n0, L, D)
            xd = _dev(tok[idx])
            lib.svdd_set_backbone_packing(-1)
            (one,) = _twice(f"svdd_backbone_cnn_lp v{v} s=1", _bb_lp_launch(pk, xd, n0, L), [n0 * L * 5])
            plain = one.cpu(n0, L, 5)
            lib.svdd_set_backbone_packing(0)
            for tag, ridx, scatter, src, dst in _indexed(n0, k0, L):
                (out,) = _twice(f"svdd_backbone_cnn_lp v{v} device plan {tag}", _bb_lp_launch(pk, xd, n0, L, _count(k0), ridx, scatter), [n0 * L * 5],
                                written=[_rows_mask(n0, L * 5, dst)])
                assert torch.equal(out.cpu(n0, L, 5)[dst].view(torch.int32), plain[src].view(torch.int32)), \
                    f"L = {L}, {mode}, v{v}, device plan of {k0} rows, {tag}: other bits than one sequence per tile"
            _exact(f"backbone_lp {mode} v{v} L={L} packings {S.packs(L)}, full, planner == s=1; count / row_idx / scatter == dense, n={nb} and n={n0}")
    finally:
        lib.svdd_set_backbone_packing(0)
        _lib.set_option(_lib.OPT_BACKBONE_LP_VERSION, 22)


# ------------------------------------------------------------------------------------------------------------------ tower
def _tower_batches(L):
    smax = S.TILE_ROWS // L
    return [2 * smax + 1] + ([smax - 1] if smax - 1 >= 1 else [])


def _tower_f32(L, nl, resmask):
    D = _distinct(L)
    tok, (stem_w, b, ws), r64, r32 = _tower(nl, L, D, resmask)
    tiles, bias = _dev(fused.pack_tower(stem_w, ws)), _dev(b)
    lib = _lib.lib()
    for n in _tower_batches(L):
        d, idx = _batch(n, L, D)
        ohd = _dev(N.onehot4(tok[idx]))
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
                    assert torch.equal(part.bits()[:k * L * 64], outs[0].bits()[:k * L * 64]), f"L = {L}, n = {n}, v{v}: count = {k} gives other bits"
        finally:
            lib.svdd_set_tower_version(0)
        for o in outs[1:]:
            assert torch.equal(o.bits(), outs[0].bits()), f"L = {L}, n = {n}: tower versions differ"
        _rep(f"tower L={L} n={n} nl={nl} res={resmask:#x}", _firsts("tower", outs[0].cpu(n, L, 64), idx, d), r64[:d], r32[:d], pool=(r64, r32))


@pytest.mark.parametrize("L", S.SHORT_LENS)
def test_conv_tower_f32(L):
    _tower_f32(L, 5, 31)


@pytest.mark.parametrize("nl,resmask", sorted({(nl, res) for _, _, nl, res in TOWER_CASES if (nl, res) != (5, 31)}))
@pytest.mark.parametrize("L", S.TOWER_MASK_LENS)
def test_conv_tower_f32_other_masks(L, nl, resmask):
    _tower_f32(L, nl, resmask)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("L", S.SHORT_LENS)
def test_conv_tower_lp(L, mode):
    dtype, parts = fused.LP_DTYPES[mode]
    D = _distinct(L)
    tok, (stem_w, b, ws), r64, _ = _tower(5, L, D, 31)
    tiles, inv = (_dev(t) for t in fused.pack_tower_lp(stem_w, ws, mode))
    rlp = N.ref_lp(mode, N.tower, N.onehot4(tok), stem_w, b, ws, 31, inv.cpu())
    bias, prec = _dev(b), _lib.PRECISIONS[mode]
    row = L * parts * 64
    for n in _tower_batches(L):
        d, idx = _batch(n, L, D)
        tokd = _dev(tok[idx])
        (out,) = _twice("svdd_conv_tower_lp", _tower_lp_launch(tiles, bias, inv, tokd, n, L, 5, 31, prec), [(n * row, dtype)])
        k = max(1, (2 * n) // 3)
        if k < n:
            (part,) = _twice("svdd_conv_tower_lp count", _tower_lp_launch(tiles, bias, inv, tokd, n, L, 5, 31, prec, _count(k)), [(n * row, dtype)],
                             written=[_rows_mask(n, row, torch.arange(k))])
            assert torch.equal(part.bits()[:k * row], out.bits()[:k * row]), f"L = {L}, {mode}, n = {n}: count = {k} gives other bits"
        _firsts("tower_lp planes", out.cpu(n, row), idx, d)
        _rep_lp(f"tower_lp {mode} L={L} n={n}", _firsts("tower_lp", _planes(out, n, L, parts), idx, d), r64[:d], rlp[:d], TOL_LOGITS[mode], pool=(r64, rlp))


# ----------------------------------------------------------------------------------------------------- generic convolution
@pytest.mark.parametrize("C", (64, 128))
@pytest.mark.parametrize("L", S.CONV_LENS)
def test_conv1d_cl_generic_kernel(L, C):
    lib = _lib.lib()
    n = 2 * (S.CONV_TILE_ROWS // L) + 1
    D = _distinct(L, S.CONV_TILE_ROWS)
    d, idx = _batch(n, L, D)
    lib.svdd_conv1d_set_dynamic(1)
    try:
        for T in (9, 5):
            for dil in S.DILS:
                x, w, _ = _conv_inputs((77, C, L, dil, T), d, L, C, C, T)
                y, _ = _conv(_dev(x[idx]), _dev(fused.pack_conv(w)), n, L, C, C, T, dil)
                r64, r32 = R.ref64(B.conv_dilated, x, w, dil), R.ref32(B.conv_dilated, x, w, dil)
                _report(f"conv generic {C}->{C} T={T} dil={dil} L={L} n={n}", _firsts("conv", y, idx, d), r64, r32, 4, cap=FLAT_Y)
    finally:
        lib.svdd_conv1d_set_dynamic(0)
