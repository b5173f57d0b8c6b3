"""-m gpu: the incremental stem of the backbone (svdd_backbone_incr_f32; Diffusion.incremental_backbone) gives the bits of the
one-launch kernel svdd_backbone_cnn_f32, step after step, on a chained trajectory of token changes.

The backbone is an H = 128 CNNModel with 20 DISTINCT layers (net_ref.distinct_layers), so that a tile computed with a neighbouring
layer's weights, or a halo read from the wrong plane, cannot hide behind equal layers.

A trajectory is one full forward that fills the carried planes and 13 incremental steps over 16 rows whose scripts hold, each at
least once: no change at all; a change at position 0 and one at L - 1; changes on both sides of a tile boundary (15 / 16, one at a
time and together); two changes 8, 40 and 80 positions apart; twelve changes in one row; every position changed at once; a token
changed to another token (not only MASK to base); a change undone one step later; the remaining rows change at 0 .. 3 random
positions per step as a decode does. After EVERY step
  * the logits are torch.equal to svdd_backbone_cnn_f32 on the same tokens;
  * the work list equals the one derived here by brute force (tile T of plane k is inside the reach iff some changed position p has
    a position of T within 4 + 4 k of it), cut into runs of at most max_item tiles; every slot of every row is rewritten;
  * planes, token copy and work list sit in sentinel-filled buffers with guards (tests/kernel_harness.py): rows >= L of a plane are
    never written, and every tile of planes 1 .. P - 1 that the list does not name and that no item of the next layer reads is
    overwritten with the sentinel before the step and must still hold it afterwards (only the tiles the mask names are written);
  * the planes equal, bit for bit, the planes a fresh full forward of the same tokens fills (no stale tile survives the chain);
  * the step run again from the saved state gives the same bits in logits, planes and list.

Teeth (patched copies of the library loaded through SVDD_HIP_LIB, this file run against each): with the reach shortened by one
tile (4 + 4 k - 16 in backbone_worklist_kernel) and with the halo tiles of a segment read from plane k where plane k - 1 is due
(backbone_seg_kernel), the file fails — the results are in the docstring of test_incremental_chain."""
import ctypes

import pytest
import torch

from svdd_amd import _lib
from tests.incr_harness import Stem, distinct_pack, one_launch as _one_launch
from tests.kernel_harness import DEV, SENT32, _st

pytestmark = pytest.mark.gpu
MASK, SLOTS, STEPS, ROWS = 4, 7, 13, 16


@pytest.fixture(scope="module")
def cnn_pack():
    return distinct_pack()


def _script(L, seed):
    """tokens [STEPS + 1][ROWS][L] u8 (CPU): step 0 is the state of the full forward, step t the state after t sets of changes."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 4, (ROWS, L), generator=g, dtype=torch.int64)
    x[torch.rand(ROWS, L, generator=g) < 0.6] = MASK
    x[6] = torch.randint(0, 4, (L,), generator=g)                  # row 6: base tokens only (token -> another token)
    x[7, 100], x[7, 37] = 1, MASK
    states = [x.clone()]

    def bump(r, pos, k=1):                                          # a real change: never the token that is there
        for p in pos:
            x[r, p] = (x[r, p] + k) % 5

    def other_base(r, pos):                                         # base token -> a different base token
        for p in pos:
            assert x[r, p] < 4
            x[r, p] = (x[r, p] + 1 + int(torch.randint(0, 3, (1,), generator=g))) % 4

    for t in range(1, STEPS + 1):
        # row 0: never changes
        if t == 1: bump(1, [0])
        if t == 2: bump(1, [L - 1])
        if t == 5: bump(1, [0, L - 1])
        if t == 1: bump(2, [15])
        if t == 2: bump(2, [16])
        if t == 3: bump(2, [15, 16])
        if t == 4: bump(2, [31, 32, 111, 112])
        if t == 1: bump(3, [60, 68])
        if t == 2: bump(3, [20, 60])
        if t == 3: bump(3, [24, 104])
        if t == 6: bump(3, [L - 9, L - 1])
        if t == 7: bump(3, [3, 43])
        if t in (1, 6): bump(4, [(11 * i + 5 * t) % L for i in range(12)] if L > 132 else list(range(t, 12 * 9 + t, 9)))
        if t in (2, 7): bump(5, range(L), k=t)
        other_base(6, [int(p) for p in torch.randperm(L, generator=g)[:1 + t % 3]])
        if t == 1: x[7, 100] = 2                                    # ... and back one step later
        if t == 2: x[7, 100] = 1
        if t == 3: x[7, 37] = 0
        if t == 4: x[7, 37] = MASK
        if t == 8: bump(7, [64])
        if t == 9: bump(7, [64], k=4)
        for r in range(8, ROWS):
            bump(r, [int(p) for p in torch.randperm(L, generator=g)[:int(torch.randint(0, 4, (1,), generator=g))]])
        if t >= 8:                                                  # the scripted rows go on like a decode, too
            for r in (1, 2, 3, 4, 5):
                bump(r, [int(p) for p in torch.randperm(L, generator=g)[:t % 3]])
        states.append(x.clone())
    assert all(torch.equal(s[0], states[0][0]) for s in states)
    twelve = (states[1][4] != states[0][4]).sum()
    assert int(twelve) == 12 and bool((states[2][5] != states[1][5]).all()) and torch.equal(states[2][7], states[0][7])
    return [s.to(torch.uint8) for s in states]


def _expected_items(prev, new, L, P, max_item):
    """[P][ROWS][SLOTS] int32 by brute force, and the bool tile masks [P][ROWS][13]."""
    items = torch.zeros(P, ROWS, SLOTS, dtype=torch.int32)
    masks = torch.zeros(P, ROWS, 13, dtype=torch.bool)
    for r in range(ROWS):
        changed = (prev[r] != new[r]).nonzero().flatten().tolist()
        for k in range(1, P + 1):
            reach = 4 + 4 * k
            for T in range(13):
                masks[k - 1, r, T] = any(abs(p - q) <= reach for p in changed for q in range(16 * T, min(16 * T + 16, L)))
            t, c = 0, 0
            while t < 13:
                if not masks[k - 1, r, t]:
                    t += 1
                    continue
                n = 1
                while n < max_item and t + n < 13 and masks[k - 1, r, t + n]:
                    n += 1
                items[k - 1, r, c] = t | n << 8
                c, t = c + 1, t + n
            assert c <= SLOTS
    return items, masks


def _tile_elems(masks, P):
    """bool [P][ROWS][208][128] from bool tile masks [P][ROWS][13]."""
    return masks.repeat_interleave(16, dim=2)[..., None].expand(P, ROWS, 208, 128)


@pytest.mark.parametrize("max_item", [2, 4])
@pytest.mark.parametrize("L", [200, 137])
def test_incremental_chain(cnn_pack, L, max_item):
    """Teeth, measured on one MI355X with this file as it stands (L = 200, max_item = 2): the library as committed passes; with the
    reach of backbone_worklist_kernel shortened by one tile (4 + 4 k - 16) the first incremental step fails on the work list; with
    the halo tiles of backbone_seg_kernel read from plane k instead of plane k - 1 it fails at step 1 with "plane 2 differs from a
    full forward's" (layer 1 has no plane to confuse: it builds f_0 from the tokens)."""
    pk = cnn_pack
    states = [s.to(DEV) for s in _script(L, 5 + L)]
    st = Stem("svdd_backbone_incr_f32", pk, ROWS, L, None, max_item, stat=1)
    P = st.D
    assert P == 8 and pk["dil"][P] != 1
    in_seq = torch.zeros(P, ROWS, 208, 128, dtype=torch.bool, device=DEV)
    in_seq[:, :, :L] = True

    got = st.run(states[0], True)
    assert torch.equal(got, _one_launch(states[0], pk))
    st.planes.assert_written_where("planes after the full forward", in_seq)
    st.x_prev.assert_written("x_prev")
    st.items.assert_untouched("work list after the full forward")
    assert torch.equal(st.x_prev.body().view(ROWS, L), states[0])
    marked = 0
    for t in range(1, STEPS + 1):
        tok = states[t]
        items, masks = _expected_items(states[t - 1].cpu(), tok.cpu(), L, P, max_item)
        marked += int(masks.sum())
        # tiles of planes 1 .. P - 1 that this step neither writes (mask of the plane) nor reads (the next layer's tiles + halo)
        read = masks.clone()
        read[:, :, 1:] |= masks[:, :, :-1]
        read[:, :, :-1] |= masks[:, :, 1:]
        idle = ~masks
        idle[:-1] &= ~read[1:]
        idle[-1] = False                                            # the tail reads every row of the last plane
        poison = (_tile_elems(idle, P).to(DEV) & in_seq).reshape(-1)
        saved = (st.planes.bits().clone(), st.x_prev.bits().clone())
        st.planes.bits()[poison] = SENT32
        poisoned = st.planes.bits().clone()
        got = st.run(tok, False)
        assert torch.equal(st.items.body().view(P, ROWS, SLOTS).cpu(), items), f"step {t}: work list"
        st.items.assert_written(f"step {t}: work list")
        left = st.planes.untouched()
        assert bool(left[poison].all()), f"step {t}: a tile outside the mask was written"
        assert bool(left[~in_seq.reshape(-1)].all()), f"step {t}: rows >= L of a plane were written"
        after = st.planes.bits().clone()
        after[poison] = saved[0][poison]
        st.planes.bits().copy_(after)
        ref = _one_launch(tok, pk)
        assert torch.equal(st.x_prev.body().view(ROWS, L), tok)
        # the planes of a fresh full forward on the same tokens
        fresh = Stem("svdd_backbone_incr_f32", pk, ROWS, L, None, max_item, stat=1)
        assert torch.equal(fresh.run(tok, True), ref)
        keep = in_seq.reshape(-1)
        bad = (after != fresh.planes.bits()) & keep
        assert not bool(bad.any()), f"step {t}: plane {int(bad.nonzero()[0]) // (ROWS * 208 * 128) + 1} differs from a full forward's"
        assert torch.equal(got, ref), f"step {t}: logits differ at row {int((got != ref).flatten(1).any(1).nonzero()[0])}"
        # the same step again from the saved state: the same bits
        st.planes.bits().copy_(poisoned)
        st.x_prev.bits().copy_(saved[1])
        st.items.bits().fill_(SENT32)
        again = st.run(tok, False)
        assert torch.equal(again, got) and torch.equal(st.items.body().view(P, ROWS, SLOTS).cpu(), items)
        again_planes = st.planes.bits().clone()
        again_planes[poison] = saved[0][poison]
        assert torch.equal(again_planes, after), f"step {t}: two launches differ"
        st.planes.bits().copy_(after)
    assert int(st.stat) == 2 * marked                              # every step ran twice


def test_incremental_entry_rejects_what_it_cannot_run(cnn_pack):
    pk = cnn_pack
    tok = torch.zeros((ROWS, 200), dtype=torch.uint8, device=DEV)
    st = Stem("svdd_backbone_incr_f32", pk, ROWS, 200, stat=1)
    dil = (ctypes.c_int * len(pk["dil"]))(*pk["dil"])
    args = lambda L, lead, mi: ("svdd_backbone_incr_f32", tok, pk["table0"], pk["tiles"], pk["vec"], pk["w2"], st.out.ptr, ROWS, L,
                                len(pk["dil"]), dil, lead, st.planes.ptr, st.x_prev.ptr, st.items.ptr, None, 1, mi, _st())
    for bad in ((104, 8, 2), (209, 8, 2), (200, 1, 2), (200, 9, 2), (200, 8, 3)):     # L, a run that holds a dilated layer, item size
        with pytest.raises(_lib.SvddError):
            _lib.call(*args(*bad))
    for b in (st.planes, st.items, st.x_prev, st.out):
        b.assert_untouched("a rejected call")


def test_mc_decode_incremental_is_bit_identical():
    """SVDD-MC at B = 256, L = 200, M = 10: incremental_backbone "on" and "off" give the same tokens and the same logits and scores at
    every step; the executed share of the stem is on record in skip_stats (the CPU simulation of the unmasking process gave 0.34 for
    a 128-step decode; fewer steps change more positions per step)."""
    from svdd_amd import synthetic
    model, emb, head, reward = synthetic.build("dna", DEV)
    model.rng_mode, model.philox_seed = "philox", 3
    B, M, S = 256, 10, 32
    runs = {}
    for mode in ("off", "on", "auto"):
        model.incremental_backbone, model.trace, model.skip_stats = mode, [], {}
        torch.manual_seed(0)
        x0 = model.controlled_sample(emb, head, num_steps=S, eval_sp_size=B, sample_M=M)
        torch.cuda.synchronize()
        runs[mode] = (x0, model.trace, dict(model.skip_stats))
    model.incremental_backbone, model.trace, model.skip_stats = "auto", None, None
    for mode in ("on", "auto"):
        assert torch.equal(runs[mode][0], runs["off"][0])
        assert len(runs[mode][1]) == len(runs["off"][1]) >= S
        for (la, sa), (lb, sb) in zip(runs[mode][1], runs["off"][1]):
            assert torch.equal(la, lb) and (sa is None) == (sb is None) and (sa is None or torch.equal(sa, sb))
        st = runs[mode][2]
        assert 0 < st["backbone_stem_tile_layers"] < st["backbone_stem_tile_layers_dense"] == (len(runs[mode][1]) - 1) * B * 13 * 8
        print(f"STEM executed tile-layers {st['backbone_stem_tile_layers']} of {st['backbone_stem_tile_layers_dense']}")
    assert "backbone_stem_tile_layers" not in runs["off"][2]
