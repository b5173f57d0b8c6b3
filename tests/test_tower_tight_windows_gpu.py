"""-m gpu: the fp32 windowed tower on TIGHT candidate windows (svdd_candidate_windows_tight: w0 = max(0, lo - 27), only the length a
multiple of 16) gives the bits of the 16-aligned windows and of the whole tower.

B = 3 parents, M = 8 candidates each, L = 200 and 120, the repository's seeded value net (synthetic.build). The candidates of every
parent: one change at lo with (lo - 27) % 16 = 0, 9, 10 and 15 (the aligned window of a single change takes 5 tiles from offset 10
on, the tight one always 4); a change at lo < 27 (w0 = 0: the sequence end is exact); one at hi > L - 28 (w1 >= L, and past L rounded
up to 16); two changes 150 apart (L = 120 has no such pair: the two are L - 40 apart there, the window is the whole sequence either
way); an exact copy. Checked, all with torch.equal:
  * the window integers and the flags (= tile counts) of both entries against the numpy formulas below;
  * the tower output on tight windows == on aligned windows == svdd_conv_tower_f32 on the candidates, for every kernel generation
    (svdd_set_tower_version 1, 2, 3: conv_tower_win_kernel, conv_tower2_kernel with two / one column tile per wave);
  * the scores: forward_candidates with tight windows == with aligned windows == forward(onehot); and the compacted path
    (svdd_compact_by_key on the tight tile counts, forward_candidates_from on the list) == the same rows of forward(onehot)."""
import numpy as np
import pytest
import torch

from svdd_amd import _lib, fused, ops, synthetic
from tests.kernel_harness import DEV

pytestmark = pytest.mark.gpu
B, M, MARGIN, MASK = 3, 8, 27, 4


def _first_last(cand, x):
    d = (cand != x[:, None, :]).reshape(-1, cand.shape[2])
    any_ = d.any(1)
    return np.where(any_, d.argmax(1), 0), np.where(any_, d.shape[1] - 1 - d[:, ::-1].argmax(1), -1)


def _aligned(lo, hi, L):
    w0, w1 = np.maximum(0, lo - MARGIN) & ~15, np.minimum((L + 15) & ~15, (hi + MARGIN + 1 + 15) & ~15)
    return np.stack([np.where(hi >= 0, w0, 0), np.where(hi >= 0, w1, 0)], 1).astype(np.int32)


def _tight(lo, hi, L):
    w0 = np.maximum(0, lo - MARGIN)
    w1 = w0 + 16 * -(-(np.minimum(L, hi + MARGIN + 1) - w0) // 16)
    return np.stack([np.where(hi >= 0, w0, 0), np.where(hi >= 0, w1, 0)], 1).astype(np.int32)


@pytest.fixture(scope="module")
def value_net():
    _, emb, head, _ = synthetic.build("dna", DEV)
    return fused.FusedValueNet(emb, head).to(DEV).eval()


def _case(L):
    """(cand [B, M, L] u8, x [B, L] u8) on the CPU."""
    g = torch.Generator().manual_seed(700 + L)
    x = torch.randint(0, 4, (B, L), generator=g, dtype=torch.uint8)
    x[torch.rand(B, L, generator=g) < 0.5] = MASK
    cand = x[:, None, :].repeat(1, M, 1)
    far = 150 if L > 190 else L - 40
    for b in range(B):
        base = MARGIN + 16 * (b + 1)                                 # parent b: windows that start 16 rows further
        changes = [[base + 0], [base + 9], [base + 10], [base + 15], [3 + 7 * b], [L - 5 - 9 * b], [20 + b, 20 + b + far], []]
        assert len(changes) == M
        for m, pos in enumerate(changes):
            for p in pos:
                cand[b, m, p] = (int(x[b, p]) + 1 + b) % 4 if x[b, p] < 4 else (m + b) % 4      # a real change, base or MASK before
    return cand.contiguous(), x.contiguous()


@pytest.mark.parametrize("L", [200, 120])
def test_tight_windows_give_the_aligned_windows_bits(value_net, L):
    fv = value_net
    cand_c, x_c = _case(L)
    lo, hi = _first_last(cand_c.numpy(), x_c.numpy())
    assert sorted(set(((lo[hi >= 0] - MARGIN) % 16).tolist()) & {0, 9, 10, 15}) == [0, 9, 10, 15]
    assert (lo[hi >= 0] < MARGIN).any() and (hi > L - 28).any() and (hi < 0).sum() == B and ((hi - lo) >= min(150, L - 40)).sum() == B
    cand, x = cand_c.to(DEV), x_c.to(DEV)
    onehot = ops.transform_samples(cand.view(B * M, L))

    # ---- the window integers
    fa = torch.full((B * M,), -7, dtype=torch.int32, device=DEV)
    ft = torch.full((B * M,), -7, dtype=torch.int32, device=DEV)
    win_a = fused.candidate_windows(cand, x, flags=fa)
    win_t = fused.candidate_windows(cand, x, flags=ft, tight=True)
    win_t2 = fused.candidate_windows(cand, x, tight=True)            # flags = NULL
    ref_a, ref_t = _aligned(lo, hi, L), _tight(lo, hi, L)
    assert np.array_equal(win_a.cpu().numpy(), ref_a) and np.array_equal(win_t.cpu().numpy(), ref_t) and torch.equal(win_t, win_t2)
    assert np.array_equal(fa.cpu().numpy(), (ref_a[:, 1] - ref_a[:, 0]) // 16) and np.array_equal(ft.cpu().numpy(), (ref_t[:, 1] - ref_t[:, 0]) // 16)
    assert (ref_t[:, 0] % 16 != 0).any() and (ref_t[:, 1] > ((L + 15) & ~15)).any()      # unaligned starts; an end past L rounded up
    assert int(ft.sum()) < int(fa.sum()) and bool((ft <= fa).all())
    assert fv.tight_windows and torch.equal(fv.windows_of(cand, x), win_t)

    # ---- the tower output, every kernel generation
    parent_out = fused.conv_tower(ops.transform_samples(x), fv.tw_tiles, fv.tw_bias, fv.tw_resmask)
    full = fused.conv_tower(onehot, fv.tw_tiles, fv.tw_bias, fv.tw_resmask)
    try:
        for ver in (1, 2, 3):
            _lib.call("svdd_set_tower_version", ver)
            seq_a = fused.conv_tower_windows(onehot, win_a, parent_out, M, fv.tw_tiles, fv.tw_bias, fv.tw_resmask)
            seq_t = fused.conv_tower_windows(onehot, win_t, parent_out, M, fv.tw_tiles, fv.tw_bias, fv.tw_resmask)
            assert torch.equal(seq_a, full), f"tower version {ver}: aligned windows differ from the whole tower"
            bad = (seq_t != full).flatten(1).any(1).nonzero().flatten().tolist()
            assert not bad, f"tower version {ver}: tight windows differ from the whole tower at candidates {bad}"
    finally:
        _lib.call("svdd_set_tower_version", 0)

    # ---- the scores
    want = fv.forward(onehot)
    got_t = fv.forward_candidates(onehot, cand, x)
    fv.tight_windows = False
    try:
        got_a = fv.forward_candidates(onehot, cand, x)
    finally:
        fv.tight_windows = True
    assert torch.equal(got_t, want) and torch.equal(got_a, want)
    live_idx = torch.full((B * M,), -1, dtype=torch.int32, device=DEV)
    slot = torch.empty(B * M, dtype=torch.int32, device=DEV)
    count = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.compact_by_key(ft, live_idx, slot, count)                    # the sort key is the tight tile count
    n = int(count)
    assert n == B * (M - 1)
    idx = live_idx[:n].long()
    assert bool((ft[idx][:-1] >= ft[idx][1:]).all())                 # largest windows first
    sc = fv.forward_candidates_from(onehot, cand, win_t, parent_out, live_idx=live_idx, count=count)
    assert torch.equal(sc[:n], want[idx])
