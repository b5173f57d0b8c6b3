"""-m gpu: the kernels that put ONE sequence into one workgroup (104 < L <= 208) at every length class. Each of them decides per
16-row tile, from L, which rows are sequence and which are zero padding, which (row tile, tap) pairs are dead and which rows may be
written; the other files run them at L = 105, 120, 128, 137, 187, 193, 200 and 208. Here: LENS = 105 .. 120 (every residue mod 16; 112:
whole tiles of padding; 113: one live row in the last tile) + 128, 129, 144, 177, 192, 193, 199, 207 (tests/lengths_ref.py, whose
conditions tests/test_lengths_cpu.py checks), three distinct sequences unless stated, every output in sentinel-guarded buffers,
every launch twice with the same bits.
  per L in LENS
    backbone        svdd_backbone_cnn_f32 (split 1) against net_ref.backbone in float64, bar(8, ref32, ref64) capped at 2e-5; the same
                    bits from split 2 / 4 / automatic, svdd_set_backbone_packing(1) and svdd_backbone_cnn_save_f32; no group time-out
    backbone_lp     svdd_backbone_cnn_lp in f16x3 / bf16x3 / f16 / bf16 against float64 under test_net_kernels_gpu._rep_lp's bar;
                    SVDD_OPT_BACKBONE_LP_VERSION 21 / 22 / 23 the same bits
    stem            svdd_backbone_incr4_f32 (10 and 12 carried layers) and svdd_backbone_incr3_f32 (12; items <= 2 and <= 1), five
                    rows, three incremental forwards on change sets built from L; after each: logits and every carried plane equal
                    a fresh first = 1 forward and the one-launch kernel bit for bit, `items` equals the numpy rule, nothing outside
                    the items' tiles changed, no row >= L and no guard written; the rows >= L hold NaN before every forward
    tower           svdd_conv_tower_f32, versions 1 / 2 / 3 (same bits), against net_ref.tower in float64
    windows         the integers of svdd_candidate_windows / _tight / svdd_candidate_parts against the numpy rules;
                    svdd_conv_tower_windows_f32 on aligned and on tight windows (versions 1 / 2 / 3) and svdd_conv_tower_parts_f32
                    (gap 70 and gap L + 1) torch.equal to the whole tower on the candidates; rows outside a window are the parent's
                    bits; with live_idx / count nothing behind count is written
    windows_lp      svdd_conv_tower_windows_lp on aligned windows, f16x3 and bf16: the bits of svdd_conv_tower_lp on the candidates
  L = 200 and 112   the incr4 chain with x, x_prev and x_prev2 at odd byte offsets (backbone_list_kernel's byte compare although
                    L % 8 == 0): the items, planes and logits of the aligned run
  per L in SWEEP_LENS (105, 113, 192, 200, 208), one case each
    stem, single changes (L rows, row r changes position r) and pairs (L - 1 rows, every separation once): logits == one-launch,
    planes == a fresh forward, plane by plane; tower, single changes and pairs (one parent, L / L - 1 candidates): tight windows and
    parts == the whole tower.
No element is excluded from any comparison. Bars come from the references (profiles/length_sweep_fp64.txt holds a run's lines);
what each check catches is on record in profiles/stem_tower_teeth.txt (tools/stem_tower_teeth.py)."""
import ctypes

import numpy as np
import pytest
import torch

from svdd_amd import _lib, fused
from tests import incr3_ref as R3
from tests import incr4_ref as R4
from tests import lengths_ref as G
from tests import net_ref as N
from tests.bb_grad_ref import save_layout as _save_layout
from tests.incr_harness import Stem, check_order, distinct_pack, one_launch
from tests.kernel_harness import DEV, SENT32, _Buf, _dev, _p, _st, _twice
from tests.test_net_kernels_gpu import (TOL_LOGITS, _bb_launch, _bb_lp, _bb_lp_launch, _bb_ref, _bb_ref_lp, _cnn, _count, _rep, _rep_lp,
                                        _rows_mask, _tower, _tower_launch, _tower_lp_launch)
from tests.test_tower_parts_cpu import part_rule, tile_layers
from tests.test_tower_tight_windows_gpu import _aligned, _first_last, _tight

pytestmark = pytest.mark.gpu
NSEQ = 3


def _exact(name):
    print(f"ERR {name} 0.000e+00 bar 0.0e+00")


# --------------------------------------------------------------------------------------------------------------- backbone
@pytest.mark.parametrize("L", G.LENS)
def test_backbone_forward(L):
    _, pk, _ = _cnn()
    n = NSEQ
    tok, r64, r32 = _bb_ref(L, n)
    xd = _dev(tok)
    lib, nl = _lib.lib(), len(pk["dil"])
    dil = (ctypes.c_int * nl)(*pk["dil"])
    fused._backbone_split_workspace(torch.device(DEV))
    outs = {}
    try:
        for split in (1, 2, 4, 0):
            _lib.set_option(_lib.OPT_BACKBONE_SPLIT, split)
            (outs[split],) = _twice(f"svdd_backbone_cnn_f32 split={split}", _bb_launch(pk, xd, n, L), [n * L * 5])
        _lib.set_option(_lib.OPT_BACKBONE_SPLIT, 1)
        lib.svdd_set_backbone_packing(1)
        (outs["packing"],) = _twice("svdd_backbone_cnn_f32 packing=1", _bb_launch(pk, xd, n, L), [n * L * 5])
    finally:
        lib.svdd_set_backbone_packing(0)
        _lib.set_option(_lib.OPT_BACKBONE_SPLIT, 0)
    err = ctypes.c_int(-1)
    _lib.check(lib.svdd_backbone_split_status(ctypes.byref(err)), "svdd_backbone_split_status")
    assert err.value == 0, "a group barrier of the split kernel timed out"
    _, _, valid = _save_layout()
    outs["save"] = _twice(
        "svdd_backbone_cnn_save_f32",
        lambda o, xh, rs, mk: lib.svdd_backbone_cnn_save_f32(xd.data_ptr(), pk["table0"].data_ptr(), pk["tiles"].data_ptr(), pk["vec"].data_ptr(),
                                                             pk["w2"].data_ptr(), o, n, L, nl, dil, xh, rs, mk, _st()),
        [n * L * 5, n * nl * 56 * 512, n * nl * 208, n * (nl + 2) * 512 * 2],
        written=[True, valid[None].expand(n * nl, 56, 512), True, True])[0]
    _rep(f"backbone L={L}", outs[1].cpu(n, L, 5), r64, r32)
    for k in (2, 4, 0, "packing", "save"):
        assert torch.equal(outs[k].bits(), outs[1].bits()), f"L = {L}: {k} gives other bits than split 1"
    _exact(f"backbone L={L} split 2/4/auto, packing, save == split 1")


@pytest.mark.parametrize("mode", ("f16x3", "bf16x3", "f16", "bf16"))
@pytest.mark.parametrize("L", G.LENS)
def test_backbone_lp(L, mode):
    pk, _ = _bb_lp(mode)
    n = NSEQ
    tok, r64, _ = _bb_ref(L, n)
    rlp = _bb_ref_lp(mode, L, n)
    xd = _dev(tok)
    outs = {}
    try:
        for v in (22, 21, 23):
            _lib.set_option(_lib.OPT_BACKBONE_LP_VERSION, v)
            (outs[v],) = _twice(f"svdd_backbone_cnn_lp v{v}", _bb_lp_launch(pk, xd, n, L), [n * L * 5])
    finally:
        _lib.set_option(_lib.OPT_BACKBONE_LP_VERSION, 22)
    _rep_lp(f"backbone_lp {mode} L={L}", outs[22].cpu(n, L, 5), r64, rlp, TOL_LOGITS[mode])
    for v in (21, 23):
        assert torch.equal(outs[v].bits(), outs[22].bits()), f"L = {L}, {mode}: version {v} gives other bits than 22"
    _exact(f"backbone_lp {mode} L={L} v21, v23 == v22")


# ------------------------------------------------------------------------------------------------------- incremental stem
@pytest.fixture(scope="module")
def cnn_pack():
    return distinct_pack()


def _expected(entry, prev, new, L, dil, lead, D, max_item):
    """items [D][n][S] of the numpy rule, and the number of leading layers whose items are tight."""
    if entry == "svdd_backbone_incr4_f32":
        return torch.from_numpy(R4.expected_items(prev, new, L, dil, lead, D, max_item)[0]), lead
    return torch.from_numpy(R3.expected_items(prev, new, L, dil, D, max_item)[0]), 0


def _chain(pk, entry, L, depth, max_item, offsets=(0, 0, 0), changes=None, rows=G.ROWS, sweep=False):
    """One full forward and the incremental forwards of `changes` on `rows` rows, every check of the module docstring after each.
    offsets: byte offsets of x, x_prev and x_prev2 inside their buffers. sweep: the planes are compared plane by plane and the
    repeated launch is the whole chain again (the planes are too large to keep copies of). -> per forward (logits, items, planes)."""
    states = G.stem_states(L, changes, rows)
    st, fresh = (Stem(entry, pk, rows, L, depth, max_item) for _ in range(2))
    if any(offsets):
        st.x_prev, st.x_prev2 = (_Buf(rows * L, torch.uint8, offset=o) for o in offsets[1:])
        st.tok = (st.x_prev, st.x_prev2)
        assert st.x_prev.ptr % 2 == offsets[1] % 2 and st.x_prev2.ptr % 2 == offsets[2] % 2
    xbuf = _Buf(rows * L, torch.uint8, offset=offsets[0])

    def dev(t):
        xbuf.body().copy_(states[t].view(-1))
        x = xbuf.body().view(rows, L)
        assert x.data_ptr() % 8 == offsets[0] % 8
        return x
    D, lead = depth, st.lead
    assert lead == G.LEAD and tuple(pk["dil"]) == G.DIL
    pview = lambda s: s.planes.body().view(D, rows, 208, 128)   # noqa: E731
    record = []

    def same_planes(what):
        for k in range(D):
            assert torch.equal(pview(st)[k, :, :L].view(torch.int32), pview(fresh)[k, :, :L].view(torch.int32)), f"{what}: plane {k + 1} differs from a full forward's"
            assert bool((st.planes.bits().view(D, rows, 208, 128)[k, :, L:] == SENT32).all()), f"{what}: rows >= L of plane {k + 1} were written"

    tok = dev(0)
    got = st.run(tok, True)
    assert torch.equal(got, one_launch(tok, pk)), f"L = {L}: the full forward differs from the one-launch kernel"
    for t in range(1, len(states)):
        what = f"{entry} L = {L}, depth {depth}, items <= {max_item}, offsets {offsets}, forward {t}"
        items, ntight = _expected(entry, states[t - 1].numpy(), states[t].numpy(), L, pk["dil"], lead, D, max_item)
        # rows >= L of every plane hold NaN (the sentinel is one): the contract says they are never read as values
        st.planes.bits().view(D, rows, 208, 128)[:, :, L:] = SENT32
        assert bool(torch.isnan(pview(st)[:, :, L:]).all())
        before = None if sweep else st.planes.bits().clone()
        saved_tok = (st.x_prev.bits().clone(), st.x_prev2.bits().clone(), st.parity)
        tok = dev(t)
        got = st.run(tok, False)
        assert torch.equal(st.lists()[0], items), f"{what}: work list"
        st.items.assert_written(f"{what}: work list")
        check_order(st, what)
        cur = st.tok[st.parity] if entry == "svdd_backbone_incr4_f32" else st.x_prev
        assert torch.equal(cur.body().view(rows, L), tok), f"{what}: the carried tokens are not the forward's"
        ref = one_launch(tok, pk)
        assert torch.equal(fresh.run(tok, True), ref), f"{what}: a full forward differs from the one-launch kernel"
        same_planes(what)
        assert torch.equal(got, ref), f"{what}: logits differ at row {int((got != ref).flatten(1).any(1).nonzero()[0]) if not torch.equal(got, ref) else -1}"
        if sweep:
            record.append((got, st.lists()[0], None))
            continue
        after = st.planes.bits().clone()
        may = G.item_rows(items, ntight, rows)[..., None].expand(D, rows, 208, 128).to(DEV).reshape(-1)
        assert not bool(((after != before) & ~may).any()), f"{what}: a plane changed outside the items' tiles"
        # the same forward again from the restored state: the same lists, the same bits
        st.planes.bits().copy_(before)
        st.x_prev.bits().copy_(saved_tok[0])
        st.x_prev2.bits().copy_(saved_tok[1])
        st.parity = saved_tok[2]
        for b in (st.items, st.order, st.count):
            b.bits().fill_(SENT32)
        again = st.run(tok, False)
        assert torch.equal(again, got) and torch.equal(st.planes.bits(), after) and torch.equal(st.lists()[0], items), f"{what}: two calls differ"
        record.append((got, st.lists()[0], pview(st)[:, :, :L].clone()))
    if sweep:                                                       # the whole chain once more on the same buffers: the same bits
        st.parity = 0
        st.run(dev(0), True)
        for t in range(1, len(states)):
            st.planes.bits().view(D, rows, 208, 128)[:, :, L:] = SENT32
            assert torch.equal(st.run(dev(t), False), record[t - 1][0]), f"L = {L}: two runs of the chain differ"
        same_planes(f"{entry} L = {L}, the chain again")
    return record


STEM_CONFIGS = (("svdd_backbone_incr4_f32", 10, 2), ("svdd_backbone_incr4_f32", 12, 2), ("svdd_backbone_incr3_f32", 12, 2),
                ("svdd_backbone_incr3_f32", 12, 1))


@pytest.mark.parametrize("L", G.LENS)
def test_stem_chain(cnn_pack, L):
    for entry, depth, max_item in STEM_CONFIGS:
        _chain(cnn_pack, entry, L, depth, max_item)
        _exact(f"stem {entry[14:19]} depth={depth} items<={max_item} L={L} == one launch, fresh planes")


@pytest.mark.parametrize("offsets", [(1, 3, 5), (1, 0, 0), (0, 1, 0), (0, 0, 1)])
@pytest.mark.parametrize("L", [200, 112])
def test_stem_chain_on_odd_pointers(cnn_pack, L, offsets):
    """L % 8 == 0: backbone_list_kernel compares 8 tokens per read unless one of its three token pointers is not 8-byte aligned."""
    assert L % 8 == 0
    for depth in (10, 12):
        base = _chain(cnn_pack, "svdd_backbone_incr4_f32", L, depth, 2)
        odd = _chain(cnn_pack, "svdd_backbone_incr4_f32", L, depth, 2, offsets)
        for t, (a, b) in enumerate(zip(base, odd), 1):
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2].view(torch.int32), b[2].view(torch.int32)), \
                f"L = {L}, depth {depth}, forward {t}: offsets {offsets} give other logits, items or planes than aligned pointers"
    _exact(f"stem incr4 L={L} token pointers at offsets {offsets} == aligned")


@pytest.mark.parametrize("kind", ["single", "pairs"])
@pytest.mark.parametrize("L", G.SWEEP_LENS)
def test_stem_position_sweep(cnn_pack, L, kind):
    changes = G.sweep_single(L) if kind == "single" else G.sweep_pairs(L)
    n = len(changes[0])
    assert n == (L if kind == "single" else L - 1)
    _chain(cnn_pack, "svdd_backbone_incr4_f32", L, 12, 2, changes=changes, rows=n, sweep=True)
    _exact(f"stem sweep {kind} L={L} rows={n} == one launch, fresh planes")


# ------------------------------------------------------------------------------------------------------------------ tower
@pytest.mark.parametrize("L", G.LENS)
def test_whole_tower(L):
    n = NSEQ
    tok, (stem_w, b, ws), r64, r32 = _tower(5, L, n, 31)
    tiles, bias, ohd = _dev(fused.pack_tower(stem_w, ws)), _dev(b), _dev(N.onehot4(tok))
    lib = _lib.lib()
    outs = []
    try:
        for v in (3, 1, 2):
            lib.svdd_set_tower_version(v)
            outs.append(_twice(f"svdd_conv_tower_f32 v{v}", _tower_launch(tiles, bias, ohd, n, L, 5, 31), [n * L * 64])[0])
    finally:
        lib.svdd_set_tower_version(0)
    for o in outs[1:]:
        assert torch.equal(o.bits(), outs[0].bits()), f"L = {L}: tower versions differ"
    _rep(f"tower L={L}", outs[0].cpu(n, L, 64), r64, r32)


class _TowerCase:
    """The candidates of one length on the device, the tower's weights and the numpy rules of the windows and the parts."""

    def __init__(self, L, changes=None, B=3):
        self.L, self.B = L, B
        self.cand, self.x = G.tower_case(L, changes, B)
        self.M = self.cand.shape[1]
        self.n = n = B * self.M
        stem_w, b, ws = N.tower_inputs(5, 0)
        self.weights = (stem_w, b, ws)
        self.tiles, self.bias = _dev(fused.pack_tower(stem_w, ws)), _dev(b)
        self.ohd, self.pod = _dev(N.onehot4(self.cand.view(n, L))), _dev(N.onehot4(self.x))
        self.cd, self.xd = _dev(self.cand), _dev(self.x)
        lo, hi = _first_last(self.cand.numpy(), self.x.numpy())
        self.ref_a, self.ref_t = _aligned(lo, hi, L), _tight(lo, hi, L)
        self.lib = _lib.lib()

    def integers(self, gaps):
        """The window and part integers from the kernels, checked against the rules. -> (aligned, tight windows, {gap: parts})."""
        c, lib, n, L = self, self.lib, self.n, self.L
        wa, fa = _twice("svdd_candidate_windows", lambda w, f: lib.svdd_candidate_windows(c.cd.data_ptr(), c.xd.data_ptr(), c.B, L, c.M, G.MARGIN, w, f, _st()),
                        [(2 * n, torch.int32), (n, torch.int32)])
        wt, ft = _twice("svdd_candidate_windows_tight", lambda w, f: lib.svdd_candidate_windows_tight(c.cd.data_ptr(), c.xd.data_ptr(), c.B, L, c.M, G.MARGIN, w, f, _st()),
                        [(2 * n, torch.int32), (n, torch.int32)])
        want_a, want_fa = N.windows(c.cand, c.x, G.MARGIN)
        assert np.array_equal(want_a.numpy(), c.ref_a)
        assert np.array_equal(wa.cpu(n, 2).numpy(), c.ref_a) and torch.equal(fa.cpu(), want_fa), f"L = {L}: aligned windows"
        assert np.array_equal(wt.cpu(n, 2).numpy(), c.ref_t), f"L = {L}: tight windows {wt.cpu(n, 2).tolist()} != {c.ref_t.tolist()}"
        assert np.array_equal(ft.cpu().numpy(), (c.ref_t[:, 1] - c.ref_t[:, 0]) // 16)
        parts = {}
        for gap in gaps:
            p, npt, fl, key = _twice("svdd_candidate_parts",
                                     lambda p, q, f, k: lib.svdd_candidate_parts(c.cd.data_ptr(), c.xd.data_ptr(), c.B, L, c.M, fused.TOWER_REACH, gap, p, q, f, k, _st()),
                                     [(6 * n, torch.int32), (n, torch.int32), (n, torch.int32), (n, torch.int32)])
            ref_p, ref_n = part_rule(c.cand.numpy(), c.x.numpy(), gap)
            ref_tl = tile_layers(ref_p, L)
            assert np.array_equal(p.cpu(n, 3, 2).numpy(), ref_p) and np.array_equal(npt.cpu().numpy(), ref_n), f"L = {L}, gap {gap}: parts"
            assert np.array_equal(fl.cpu().numpy(), ref_tl) and np.array_equal(key.cpu().numpy(), (ref_tl + 5) // 6)
            parts[gap] = (p, ref_p)
        return wa, wt, parts

    def whole(self, what=""):
        lib, L = self.lib, self.L
        (parent,) = _twice(f"svdd_conv_tower_f32 parents{what}", _tower_launch(self.tiles, self.bias, self.pod, self.B, L, 5, 31), [self.B * L * 64])
        (full,) = _twice(f"svdd_conv_tower_f32 candidates{what}", _tower_launch(self.tiles, self.bias, self.ohd, self.n, L, 5, 31), [self.n * L * 64])
        return parent, full

    def windows(self, what, win, parent, nn=None, li=None, cnt=None, written=None):
        c, L = self, self.L
        pb, wb = parent.body(), win.body()
        return _twice(f"svdd_conv_tower_windows_f32 {what}",
                      lambda o: c.lib.svdd_conv_tower_windows_f32(c.ohd.data_ptr(), c.tiles.data_ptr(), c.bias.data_ptr(), wb.data_ptr(), pb.data_ptr(), o,
                                                                  c.n if nn is None else nn, L, c.M, 5, 31, _p(li), _p(cnt), _st()),
                      [c.n * L * 64], written=written)[0]

    def parts(self, what, parts, parent, nn=None, li=None, cnt=None, written=None):
        c, L = self, self.L
        pb, qb = parent.body(), parts.body()
        return _twice(f"svdd_conv_tower_parts_f32 {what}",
                      lambda o: c.lib.svdd_conv_tower_parts_f32(c.ohd.data_ptr(), c.tiles.data_ptr(), c.bias.data_ptr(), qb.data_ptr(), pb.data_ptr(), o,
                                                                c.n if nn is None else nn, L, c.M, 5, 31, fused.TOWER_REACH, _p(li), _p(cnt), _st()),
                      [c.n * L * 64], written=written)[0]

    def check(self, what, out, full, parent, inside):
        """out == the whole tower everywhere; outside `inside` (bool [n][L]) it is the parent's bits."""
        n, L = self.n, self.L
        got, want = out.bits().view(n, L, 64), full.bits().view(n, L, 64)
        bad = (got != want).flatten(1).any(1).nonzero().flatten().tolist()
        assert not bad, f"L = {L}, {what}: differs from the whole tower at candidates {bad} (changes {[G.tower_changes(L)[m % self.M][:3] for m in bad] if self.M == 15 else ''})"
        par = parent.bits().view(self.B, L, 64).repeat_interleave(self.M, dim=0)
        outside = ~torch.from_numpy(inside).to(DEV)
        assert torch.equal(got[outside], par[outside]), f"L = {L}, {what}: a row outside its window is not the parent's"


def _part_rows(ref_p, L):
    """bool [n][L]: rows within the tower's reach of a part."""
    r = np.arange(L)[None, :]
    m = np.zeros((ref_p.shape[0], L), dtype=bool)
    for k in range(3):
        a, b = ref_p[:, k, :1], ref_p[:, k, 1:]
        m |= (a >= 0) & (r >= a - fused.TOWER_REACH) & (r <= b + fused.TOWER_REACH)
    return m


@pytest.mark.parametrize("L", G.LENS)
def test_windowed_tower(L):
    c = _TowerCase(L)
    n, lib = c.n, c.lib
    wa, wt, parts = c.integers((G.GAP, L + 1))
    in_a, in_t = G.window_rows(c.ref_a, L), G.window_rows(c.ref_t, L)
    live = torch.tensor([n - 1, 3, 0, 14, 29, 7, 12, 13], dtype=torch.int32)       # candidates: every position, single, none, ..
    ld, k = _dev(live), 6
    parent0, full0 = c.whole()
    try:
        for v in (3, 1, 2):
            lib.svdd_set_tower_version(v)
            parent, full = c.whole(f" v{v}")
            assert torch.equal(parent.bits(), parent0.bits()) and torch.equal(full.bits(), full0.bits()), f"L = {L}: tower versions differ"
            c.check(f"aligned windows v{v}", c.windows(f"aligned v{v}", wa, parent), full, parent, in_a)
            c.check(f"tight windows v{v}", c.windows(f"tight v{v}", wt, parent), full, parent, in_t)
            comp = c.windows(f"tight v{v} live_idx", wt, parent, len(live), ld, _count(k), written=[_rows_mask(n, L * 64, torch.arange(k))])
            assert torch.equal(comp.bits().view(n, L, 64)[:k], full.bits().view(n, L, 64)[live[:k].long()]), f"L = {L}, v{v}: the compacted list"
    finally:
        lib.svdd_set_tower_version(0)
    for gap, (p, ref_p) in parts.items():
        c.check(f"parts gap {gap}", c.parts(f"gap {gap}", p, parent0), full0, parent0, _part_rows(ref_p, L))
        comp = c.parts(f"gap {gap} live_idx", p, parent0, len(live), ld, _count(k), written=[_rows_mask(n, L * 64, torch.arange(k))])
        assert torch.equal(comp.bits().view(n, L, 64)[:k], full0.bits().view(n, L, 64)[live[:k].long()]), f"L = {L}, gap {gap}: the compacted list"
    _exact(f"tower windows aligned / tight v1 v2 v3, parts gap 70 / {L + 1} L={L} == whole tower")


@pytest.mark.parametrize("mode", ("f16x3", "bf16"))
@pytest.mark.parametrize("L", G.LENS)
def test_windowed_tower_lp(L, mode):
    dtype, planes = fused.LP_DTYPES[mode]
    cand, x = G.tower_case(L)
    B, M = x.shape[0], cand.shape[1]
    n, row = B * M, L * planes * 64
    stem_w, b, ws = N.tower_inputs(5, 0)
    tiles, inv = (_dev(t) for t in fused.pack_tower_lp(stem_w, ws, mode))
    win, _ = N.windows(cand, x, G.MARGIN)
    lib, bias, cd, xd, wd, prec = _lib.lib(), _dev(b), _dev(cand), _dev(x), _dev(win), _lib.PRECISIONS[mode]
    (parent,) = _twice("svdd_conv_tower_lp parents", _tower_lp_launch(tiles, bias, inv, xd, B, L, 5, 31, prec), [(B * row, dtype)])
    (full,) = _twice("svdd_conv_tower_lp candidates", _tower_lp_launch(tiles, bias, inv, cd, n, L, 5, 31, prec), [(n * row, dtype)])
    pb = parent.body()
    (out,) = _twice("svdd_conv_tower_windows_lp",
                    lambda o: lib.svdd_conv_tower_windows_lp(cd.data_ptr(), tiles.data_ptr(), bias.data_ptr(), inv.data_ptr(), wd.data_ptr(), pb.data_ptr(), o,
                                                             n, L, M, 5, 31, None, None, prec, _st()), [(n * row, dtype)])
    got, want = out.bits().view(n, L, planes * 64), full.bits().view(n, L, planes * 64)
    bad = (got != want).flatten(1).any(1).nonzero().flatten().tolist()
    assert not bad, f"L = {L}, {mode}: windows differ from the whole lp tower at candidates {bad}"
    outside = ~torch.from_numpy(G.window_rows(win.numpy(), L)).to(DEV)
    par = parent.bits().view(B, L, planes * 64).repeat_interleave(M, dim=0)
    assert torch.equal(got[outside], par[outside]), f"L = {L}, {mode}: a row outside its window is not the parent's"
    _exact(f"tower_windows_lp {mode} L={L} == svdd_conv_tower_lp")


@pytest.mark.parametrize("kind", ["single", "pairs"])
@pytest.mark.parametrize("L", G.SWEEP_LENS)
def test_tower_position_sweep(L, kind):
    changes = G.tower_sweep_single(L) if kind == "single" else G.tower_sweep_pairs(L)
    c = _TowerCase(L, changes, B=1)
    assert c.M == (L if kind == "single" else L - 1)
    _, wt, parts = c.integers((G.GAP,))
    parent, full = c.whole()
    c.check("tight windows", c.windows("tight", wt, parent), full, parent, G.window_rows(c.ref_t, L))
    p, ref_p = parts[G.GAP]
    c.check("parts", c.parts("gap 70", p, parent), full, parent, _part_rows(ref_p, L))
    _exact(f"tower sweep {kind} L={L} candidates={c.M}: tight windows, parts == whole tower")
