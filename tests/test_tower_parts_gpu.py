"""-m gpu: the fp32 windowed tower on the candidates' PARTS with per-layer row ranges (svdd_candidate_parts +
svdd_conv_tower_parts_f32) gives the bits of the tight windows and of the whole tower.

B = 3 parents, M = 8 candidates each, L = 105, 200 and 208, the repository's seeded value net (synthetic.build). Hand-built
candidates (_changes): no change; one change at row 0, at row L - 1, mid-sequence at several offsets; two changes 69 apart (one part)
and 70 apart (two); changes at 0, 70 and 140; four clusters; every position changed; changes whose one part clips at both sequence
ends. Checked:
  * the parts, their number, the tile-layers and the sort key of svdd_candidate_parts against the numpy rule of
    tests/test_tower_parts_cpu.py, exactly, for gap = 70 and for a gap above L (one part always); the cap of 3 parts on a longer row;
  * the tower output on parts, torch.equal to conv_tower_windows on tight windows and to conv_tower on the whole candidates, for
    both gaps; without live_idx, with a compacted list, and on a sub-slice of the list into a guarded buffer (the guard rows and
    the rows past the slice's count stay untouched);
  * rows of a computed tile past a layer's needed range may hold garbage that the next layer never reads: held by the equality with
    the whole tower on every candidate, the windows of which end at every offset of a tile here;
  * the scores: forward_candidates with tower_parts "on" / "layers" / "off" == forward(onehot);
  * one short C2-shaped SVDD-MC decode (B = 8, 16 steps) with tower_parts "off", "layers" and "on": the same tokens and the same
    traced scores, bit for bit; tower_tile_layers of skip_stats falls from "off" to "layers" to "on"."""
import numpy as np
import pytest
import torch

from svdd_amd import fused, ops, synthetic
from tests.kernel_harness import DEV
from tests.test_tower_parts_cpu import GAP, part_rule, tile_layers

pytestmark = pytest.mark.gpu
B, M, MASK = 3, 8, 4


@pytest.fixture(scope="module")
def value_net():
    _, emb, head, _ = synthetic.build("dna", DEV)
    return fused.FusedValueNet(emb, head).to(DEV).eval()


def _changes(L):
    mid = L // 2
    ch = [[], [0], [L - 1], [mid], [20, 89], [20, 90], [0, 70, 140], [3, 5, 75, 77, 147, 150, 190, 195],
          list(range(L)), list(range(20, L, 60)) + [L - 21], [mid + 5], [mid + 11], [1], [L - 2], [33, 103], [17, 86],
          [], [2, 9], [L - 28], [27], [28], [mid - 7, mid + 7], [10, 80, 150], [L - 18, L - 100]]
    assert len(ch) == B * M
    return [sorted({p for p in c if 0 <= p < L}) for c in ch]


def _case(L):
    """(cand [B, M, L] u8, x [B, L] u8) on the CPU."""
    g = torch.Generator().manual_seed(900 + L)
    x = torch.randint(0, 4, (B, L), generator=g, dtype=torch.uint8)
    x[torch.rand(B, L, generator=g) < 0.5] = MASK
    cand = x[:, None, :].repeat(1, M, 1)
    for i, pos in enumerate(_changes(L)):
        b, m = divmod(i, M)
        for p in pos:
            cand[b, m, p] = (int(x[b, p]) + 1 + b) % 4 if x[b, p] < 4 else (m + b) % 4      # a real change, base or MASK before
    return cand.contiguous(), x.contiguous()


def _parts(cand, x, gap):
    n = cand.shape[0] * cand.shape[1]
    outs = [torch.full((n,), -7, dtype=torch.int32, device=DEV) for _ in range(3)]
    parts = fused.candidate_parts(cand, x, gap=gap, nparts=outs[0], flags=outs[1], key=outs[2])
    return (parts, *outs)


@pytest.mark.parametrize("L", [105, 200, 208])
def test_tower_on_parts_gives_the_window_and_whole_tower_bits(value_net, L):
    fv = value_net
    cand_c, x_c = _case(L)
    cand, x = cand_c.to(DEV), x_c.to(DEV)
    n = B * M
    onehot = ops.transform_samples(cand.view(n, L))
    parent_out = fused.conv_tower(ops.transform_samples(x), fv.tw_tiles, fv.tw_bias, fv.tw_resmask)
    full = fused.conv_tower(onehot, fv.tw_tiles, fv.tw_bias, fv.tw_resmask)
    win_t = fused.candidate_windows(cand, x, tight=True)
    seq_t = fused.conv_tower_windows(onehot, win_t, parent_out, M, fv.tw_tiles, fv.tw_bias, fv.tw_resmask)
    assert torch.equal(seq_t, full)
    old = 6 * ((win_t[:, 1] - win_t[:, 0]) // 16).cpu().numpy()

    for gap in (GAP, L + 1):
        # ---- the integers
        parts, nparts, flags, key = _parts(cand, x, gap)
        ref_p, ref_n = part_rule(cand_c.numpy(), x_c.numpy(), gap)
        ref_t = tile_layers(ref_p, L)
        assert np.array_equal(parts.cpu().numpy(), ref_p) and np.array_equal(nparts.cpu().numpy(), ref_n)
        assert np.array_equal(flags.cpu().numpy(), ref_t) and np.array_equal(key.cpu().numpy(), (ref_t + 5) // 6)
        assert torch.equal(fused.candidate_parts(cand, x, gap=gap), parts)               # the optional outputs NULL
        assert np.array_equal(fused.part_layer_tiles(parts, L).sum(1).cpu().numpy(), ref_t)
        assert (ref_t <= old).all() and ref_t.sum() < old.sum() and ((ref_t == 0) == (old == 0)).all()
        if gap == GAP:
            assert ref_n.max() == (3 if L > 140 else 2) and (ref_n == 0).sum() == 2 and (ref_n == 2).sum() >= 2
        else:
            assert ref_n.max() == 1

        # ---- the tower output: every candidate, workgroup i = candidate i
        seq = fused.conv_tower_windows(onehot, parts, parent_out, M, fv.tw_tiles, fv.tw_bias, fv.tw_resmask)
        bad = (seq != full).flatten(1).any(1).nonzero().flatten().tolist()
        assert not bad, f"gap {gap}: the tower on parts differs from the whole tower at candidates {bad}"
        assert torch.equal(seq, seq_t)

        # ---- a compacted list, largest first
        live_idx = torch.full((n,), -1, dtype=torch.int32, device=DEV)
        slot = torch.empty(n, dtype=torch.int32, device=DEV)
        count = torch.zeros(1, dtype=torch.int32, device=DEV)
        ops.compact_by_key(key, live_idx, slot, count)
        k = int(count)
        assert k == n - 2
        idx = live_idx[:k].long()
        assert bool((key[idx][:-1] >= key[idx][1:]).all())
        seq_c = fused.conv_tower_windows(onehot, parts, parent_out, M, fv.tw_tiles, fv.tw_bias, fv.tw_resmask, live_idx=live_idx, count=count)
        assert torch.equal(seq_c[:k], full[idx])

        # ---- a sub-slice of the list into a guarded buffer: entries [5, 5 + 9) of the list, room for 12
        guard = torch.full((1 + 12 + 1, L, 64), -3.0, device=DEV)
        sub = torch.full((1,), 9, dtype=torch.int32, device=DEV)
        fused.conv_tower_windows(onehot, parts, parent_out, M, fv.tw_tiles, fv.tw_bias, fv.tw_resmask, live_idx=live_idx[5:], count=sub,
                                 out=guard[1:13])
        assert torch.equal(guard[1:10], full[idx[5:14]])
        assert bool((guard[0] == -3.0).all()) and bool((guard[10:] == -3.0).all())

    # ---- the scores through the net's own routing
    want = fv.forward(onehot)
    try:
        for mode in ("on", "layers", "off"):
            fv.tower_parts = mode
            assert fv.tower_ranges_of(cand, x).shape == ((n, 2) if mode == "off" else (n, 3, 2))
            assert torch.equal(fv.forward_candidates(onehot, cand, x), want), mode
    finally:
        fv.tower_parts = "on"


def test_parts_cap_on_a_longer_row():
    """With gap = 70 a fourth part needs L >= 211, more than the tower takes: the cap is checked on the integers alone."""
    L = 300
    x = torch.zeros((1, L), dtype=torch.uint8)
    cand = x[:, None, :].repeat(1, 4, 1)
    for m, pos in enumerate(([5, 100, 200, 299], [0, 70, 140, 210, 280], [10, 79, 148, 217], [])):
        cand[0, m, pos] = 1
    parts, nparts, flags, key = _parts(cand.to(DEV), x.to(DEV), GAP)
    ref_p, ref_n = part_rule(cand.numpy(), x.numpy(), GAP)
    assert ref_p[0].tolist() == [[5, 5], [100, 100], [200, 299]] and ref_n.tolist() == [3, 3, 1, 0]
    assert np.array_equal(parts.cpu().numpy(), ref_p) and np.array_equal(nparts.cpu().numpy(), ref_n)
    assert np.array_equal(flags.cpu().numpy(), tile_layers(ref_p, L))


def test_short_mc_decode_same_tokens_and_scores_for_every_tower_parts_mode():
    model, emb, head, _ = synthetic.build("dna", DEV)
    model.rng_mode, model.philox_seed = "philox", 5
    fn = model.value_callable(emb, head)
    outs = {}
    try:
        for mode in ("off", "layers", "on"):
            fn.tower_parts = mode
            model.trace, model.skip_stats = [], {}
            x0 = model.controlled_sample(emb, head, num_steps=16, eval_sp_size=8, sample_M=10)
            torch.cuda.synchronize()
            outs[mode] = (x0, [sc for _, sc in model.trace if sc is not None], dict(model.skip_stats))
            model.trace, model.skip_stats = None, None
    finally:
        fn.tower_parts = "on"
    ref = outs["off"]
    assert len(ref[1]) == 16
    for mode in ("layers", "on"):
        o = outs[mode]
        assert torch.equal(o[0], ref[0]), mode
        assert len(o[1]) == 16 and all(torch.equal(a, b) for a, b in zip(o[1], ref[1])), mode
        assert o[2]["live_candidates"] == ref[2]["live_candidates"]
    t = {m: outs[m][2]["tower_tile_layers"] for m in outs}
    r = {m: outs[m][2]["tower_window_rows"] for m in outs}
    print(f"tower_tile_layers {t}, tower_window_rows {r}")
    assert t["on"] <= t["layers"] < t["off"] and r["on"] <= r["layers"] < r["off"]
