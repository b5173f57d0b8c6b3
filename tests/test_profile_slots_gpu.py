"""-m gpu: which profiling slot every timed entry of the library records under (enum SvddProfileSlot, csrc/svdd_host.h), and that one
call is ONE span — in particular the entries that time one span over several launches (svdd_gru_bidir_train2_f32, _bwd2_f32,
svdd_backbone_incr_f32, the tail round of svdd_backbone_cnn_f32, svdd_tds_resample). bench.py, tools/ and tests/test_configs_gpu.py
read the slots by number. The entry -> slot table is the one of the call sites before the slots had names.

Values are not checked here (the per-kernel files do that): every call is the smallest the kernel accepts — 2 - 3 sequences, M = 2,
L = 50, or L = 200 where the entry needs 104 < L <= 208 — on the operands of the per-kernel tests."""
import ctypes

import pytest
import torch

from svdd_amd import _lib, fused, ops
from svdd_amd.fused import pack_conv, pack_gru, pack_gru_bwd
from tests import grad_ref as R
from tests import net_ref as N
from tests import test_net_kernels_gpu as NK
from tests.kernel_harness import DEV, _dev, _st
from tests.test_kernels_gpu import _mt_device_state

pytestmark = pytest.mark.gpu
SLOTS = 13
PROPOSE, SELECT, CONV1D, GRU, EPILOGUE_LN, CONV_TOWER, BACKBONE, VALUE_TAIL, TDS_RESAMPLE, MT19937, BACKBONE_GRAD, GRU_TRAIN, GRU_BPTT = range(SLOTS)
MODE = "f16x3"


def _f32(*shape):
    return torch.zeros(*shape, dtype=torch.float32, device=DEV)


def _backbone_calls():
    cnn, pk, _ = NK._cnn()
    n = 2
    tok50, tok200 = _dev(N.tokens(3, 50, 0)), _dev(N.tokens(n, 200, 0))
    out50 = _f32(3 * 50 * 5)
    yield "svdd_backbone_cnn_f32", BACKBONE, lambda: _lib.check(NK._bb_launch(pk, tok50, 3, 50)(out50.data_ptr()), "backbone")
    yield "svdd_backbone_cnn_lp", BACKBONE, lambda: _lib.check(NK._bb_lp_launch(NK._bb_lp(MODE)[0], tok50, 3, 50)(out50.data_ptr()), "backbone lp")
    # a batch of CUs + 2 sequences with the split workspace set (fused.backbone_cnn sets it): whole rounds on backbone_kernel and the
    # two left over on backbone_split_kernel, two launches under one span
    ncu = _lib.device_info()[1]
    tail = _dev(N.tokens(2, 200, 1))[torch.arange(ncu + 2, device=DEV) % 2].contiguous()
    yield "svdd_backbone_cnn_f32 (tail round)", BACKBONE, lambda: fused.backbone_cnn(tail, pk)
    saved = []
    yield "svdd_backbone_cnn_save_f32", BACKBONE, lambda: saved.append(fused.backbone_cnn_save(tok200, pk)[1])
    pkg = fused.pack_backbone_grad(cnn)
    yield "svdd_backbone_cnn_grad_f32", BACKBONE_GRAD, lambda: fused.backbone_cnn_grad(_f32(n, 200, 5), pk, pkg, saved[0])
    st = fused.IncrementalStem(n, 200, fused.leading_dilation1(pk["dil"]), DEV)
    assert st.lead >= 2
    yield "svdd_backbone_incr_f32 first=1", BACKBONE, lambda: fused.backbone_cnn_incremental(tok200, pk, st)
    moved = tok200.clone()
    moved[1, 77] = (moved[1, 77] + 1) % 4
    yield "svdd_backbone_incr_f32 first=0", BACKBONE, lambda: fused.backbone_cnn_incremental(moved, pk, st)


def _value_net_calls():
    lib, n, L, prec = _lib.lib(), 3, 50, _lib.PRECISIONS[MODE]
    parts = fused.LP_DTYPES[MODE][1]
    stem_w, b, ws = N.tower_inputs(5, 0)
    tiles, bias = _dev(fused.pack_tower(stem_w, ws)), _dev(b)
    tiles_lp, inv = (_dev(t) for t in fused.pack_tower_lp(stem_w, ws, MODE))
    tok = N.tokens(n, L, 1)
    tokd, ohd = _dev(tok), _dev(N.onehot4(tok))
    out = _f32(n * L * 64)
    out_lp = torch.zeros(n * L * parts * 64, dtype=fused.LP_DTYPES[MODE][0], device=DEV)
    yield "svdd_conv_tower_f32", CONV_TOWER, lambda: _lib.check(NK._tower_launch(tiles, bias, ohd, n, L, 5, 31)(out.data_ptr()), "tower")
    yield "svdd_conv_tower_lp", CONV_TOWER, lambda: _lib.check(
        NK._tower_lp_launch(tiles_lp, bias, inv, tokd, n, L, 5, 31, prec)(out_lp.data_ptr()), "tower lp")
    # windows: one parent of L = 200 and its M = 2 candidates, one of them changed at one position
    x = N.tokens(2, 200, 2)[1:2].contiguous()
    cand = x[:, None, :].repeat(1, 2, 1)
    cand[0, 1, 90] = (cand[0, 1, 90] + 1) % 4
    xd, cd = _dev(x), _dev(cand)
    win = fused.candidate_windows(cd, xd)
    parent = fused.conv_tower(_dev(N.onehot4(x)), tiles, bias, 31)
    parent_lp = fused.conv_tower_lp(xd, tiles_lp, bias, inv, 31, prec)
    cand_oh = _dev(N.onehot4(cand.view(2, 200)))
    yield "svdd_conv_tower_windows_f32", CONV_TOWER, lambda: fused.conv_tower_windows(cand_oh, win, parent, 2, tiles, bias, 31)
    yield "svdd_conv_tower_windows_lp", CONV_TOWER, lambda: fused.conv_tower_windows_lp(cd, win, parent_lp, tiles_lp, bias, inv, 31, prec)

    mod, xg, gout = R.gru_inputs(n, L)
    wpack, bpack = (_dev(t) for t in pack_gru(mod))
    wp_lp, bp_lp, inv_g = (_dev(t) for t in fused.pack_gru_lp(mod, MODE))
    xgd, god, wb = _dev(xg), _dev(gout), _dev(pack_gru_bwd(mod))
    yield "svdd_gru_bidir_f32", GRU, lambda: fused.gru_bidir(xgd, wpack, bpack)
    yield "svdd_gru_bidir_lp", GRU, lambda: fused.gru_bidir_lp(xgd, wp_lp, bp_lp, inv_g, prec)
    o, s, gi, dx, g = _f32(2 * n * L * 64), _f32(2 * n * L * 256), _f32(2 * n * L * 192), _f32(2 * n * L * 64), _f32(n * L * 64)
    p = lambda t: t.data_ptr()   # noqa: E731
    yield "svdd_gru_bidir_train_f32", GRU_TRAIN, lambda: _lib.check(lib.svdd_gru_bidir_train_f32(p(xgd), p(wpack), p(bpack), p(o), p(s), n, L, _st()), "train")
    yield "svdd_gru_bidir_train2_f32", GRU_TRAIN, lambda: _lib.check(
        lib.svdd_gru_bidir_train2_f32(p(xgd), p(wpack), p(bpack), p(gi), p(o), p(s), n, L, _st()), "train2")
    yield "svdd_gru_bidir_bwd_f32", GRU_BPTT, lambda: _lib.check(lib.svdd_gru_bidir_bwd_f32(p(god), p(o), p(s), p(wb), p(dx), n, L, _st()), "bwd")
    yield "svdd_gru_bidir_bwd2_f32", GRU_BPTT, lambda: _lib.check(
        lib.svdd_gru_bidir_bwd2_f32(p(god), p(o), p(s), p(wb), p(gi), p(xgd), p(g), n, L, _st()), "bwd2")

    h, w1, b1, gam, bet, w_eff, b_eff = N.tail_inputs(n, L, 1, net_scale=True)
    hd, wd, bd = _dev(h), _dev(w_eff), _dev(b_eff)
    w1p, b1f = (_dev(t) for t in fused.pack_tail(w1, b1, gam, bet))
    w1p_lp, b1f_lp, inv_t = fused.pack_tail_lp(w1, b1, gam, bet, MODE)
    w1p_lp, b1f_lp = _dev(w1p_lp), _dev(b1f_lp)
    yield "svdd_value_tail_f32", VALUE_TAIL, lambda: fused.value_tail(hd, w1p, b1f, wd, bd)
    yield "svdd_value_tail_lp", VALUE_TAIL, lambda: fused.value_tail_lp(hd, w1p_lp, b1f_lp, wd, bd, inv_t, prec)
    th, tw1, tb1, tgam, tbet, tweff = (_dev(t) for t in R.tail_inputs(n, L))
    g0, g1 = _f32(n * L * 64), _f32(n * L * 64)
    yield "svdd_reward_tail_grad_f32", VALUE_TAIL, lambda: _lib.check(
        lib.svdd_reward_tail_grad_f32(p(th[0]), p(th[1]), p(tw1), p(tb1), p(tgam), p(tbet), p(tweff), 1e-5, n, L, p(g0), p(g1), _st()), "tail grad")

    sx, sw, sb, sg = R.stem_inputs(n, L)
    wk, sxd, sbd, sgd = _dev(sw.permute(2, 1, 0).reshape(-1, 64)), _dev(sx), _dev(sb), _dev(sg)
    sdx = _f32(n * L * 4)
    yield "svdd_reward_stem_f32", CONV_TOWER, lambda: _lib.check(lib.svdd_reward_stem_f32(p(sxd), p(wk), p(sbd), p(out), n, L, 15, _st()), "stem")
    yield "svdd_reward_stem_bwd_f32", CONV_TOWER, lambda: _lib.check(lib.svdd_reward_stem_bwd_f32(p(sgd), p(wk), p(sdx), n, L, 15, _st()), "stem bwd")

    w5 = _dev(pack_conv(ws[0]))
    yield "svdd_conv1d_cl_f32", CONV1D, lambda: fused.conv1d_cl(xgd, w5, 64, 5, 1)
    yield "svdd_conv1d_cl_gated_f32", CONV1D, lambda: _lib.check(
        lib.svdd_conv1d_cl_gated_f32(p(xgd), p(w5), p(out), n, L, 64, 64, 5, 1, None, None, _st()), "gated conv")
    ones, zeros = torch.ones(64, device=DEV), torch.zeros(64, device=DEV)
    yield "svdd_epilogue_ln_f32", EPILOGUE_LN, lambda: fused.epilogue_ln(xgd, bias=zeros, gamma=ones, beta=zeros)


def _sampler_calls():
    B, L, M = 3, 50, 2
    x = _dev(N.tokens(B, L, 3))
    logits, q = _f32(B, L, 5), torch.full((B, L, 5), 0.2, device=DEV)
    rng = ops.Rng(seed=7)
    yield "svdd_propose", PROPOSE, lambda: ops.propose(logits, x, 0.5, 0.5, M, rng)
    yield "svdd_sample_categorical", PROPOSE, lambda: ops.sample_categorical(q, x, M, rng)
    cand = x[:, None, :].repeat(1, M, 1).contiguous()
    scores = torch.arange(B * M, dtype=torch.float32, device=DEV)
    yield "svdd_select", SELECT, lambda: ops.select(scores, cand)
    slot = torch.arange(B * M, dtype=torch.int32, device=DEV)
    yield "svdd_select_compact", SELECT, lambda: ops.select_compact(scores, slot, _f32(B), cand)
    u = torch.tensor([0.1, 0.5, 0.9], dtype=torch.float64, device=DEV)
    yield "svdd_tds_resample", TDS_RESAMPLE, lambda: ops.tds_resample(torch.ones(B, device=DEV), torch.ones(B, device=DEV), 1.0, x, u)
    state, _ = _mt_device_state(0, 0)
    rand = _f32(700)
    yield "svdd_mt19937_uniform_f32", MT19937, lambda: _lib.check(
        _lib.lib().svdd_mt19937_uniform_f32(state.data_ptr(), rand.data_ptr(), 700, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "mt19937")


def test_every_timed_entry_records_one_span_in_its_own_slot():
    """After ONE call of a timed entry svdd_profile_collect reports exactly one launch with a positive time in the entry's slot and
    none in the other twelve. The operands are made with profiling off (making them launches timed kernels too)."""
    seen = []
    try:
        for calls in (_backbone_calls, _value_net_calls, _sampler_calls):
            for name, slot, call in calls():
                torch.cuda.synchronize()
                for k in range(SLOTS):
                    _lib.profile_collect(k)
                _lib.profile_enable(True)
                call()
                _lib.profile_enable(False)
                torch.cuda.synchronize()
                got = [_lib.profile_collect(k) for k in range(SLOTS)]
                print(f"SLOT {name} {slot} {got[slot][0] * 1e3:.1f} us")
                assert [n for _, n in got] == [int(k == slot) for k in range(SLOTS)], (name, slot, got)
                assert got[slot][0] > 0.0, (name, got[slot])
                seen.append(name)
    finally:
        _lib.profile_enable(False)
    assert len(seen) == len(set(seen)) == 31, seen
    fused.check_backbone_split()
