"""-m gpu: svdd_backbone_incr3_f32 — the incremental backbone with the carried planes extended through the dilation-4 layers —
gives the bits of svdd_backbone_cnn_f32, step after step.

Chains of 12 steps on 16 rows (H = 128 CNNModel, 20 DISTINCT layers: net_ref.distinct_layers) behind one full forward. The rows:
  0  never changes          1  changes at position 0            2  changes at position L - 1       3  changes at the middle
  4  two changes L - 3 >= 102 rows apart (1 and L - 2): more than the deepest reach, 100
  5  two changes one tile apart (40 and 56)                     6  every position changes at once (steps 2 and 7)
  7  changes on odd steps only: every change is followed by a step without one
  8 .. 15  zero to three random changes per step, as a decode makes them; from step 8 on rows 1 .. 6 go on like that too
Lengths: 200 (tile 12 drops the taps + 8, + 12, + 16 of a dilation-4 layer, tile 0 tap - 16), 208 (tile 12 is full), 193 (tile 12
holds one row), 105 (7 tiles, the smallest length the entry takes); items of at most 2 tiles at every length, 1 and 4 at L = 200;
12 carried layers at every length, 9 and 10 at L = 200.
After every step: the logits equal svdd_backbone_cnn_f32's on the same tokens; every plane, rows < L, equals the planes of a fresh
first = 1 forward; the work list equals the numpy restatement (tests/incr3_ref.py); order[k] is a permutation of the non-empty
items with tile counts never increasing; the guards around every buffer are intact and rows >= L of the planes are unwritten; the
tiles outside a layer's mask that the next layer does not read were poisoned before the step and are still poisoned after it; the
two counters of `stat` hold the marked tile-layers of the dilation-1 and of the deeper layers; the step made again from the saved
state gives the same bits.
One short SVDD-MC decode (B = 256, L = 200, M = 10, 32 steps, Philox) with 12 carried layers, with 8 and with the incremental
backbone off: the same tokens, the same logits and scores at every step.

Teeth, from runs of this file on one MI355X against deliberately broken builds of the library (L = 200, items <= 2, depth 12):
  * the deep reach shortened by one tile (r[k - 1] - 16 for the dilation-4 layers in backbone_worklist_kernel): step 1 fails on
    "work list";
  * the halo tiles of backbone_seg_kernel read from plane k where plane k - 1 is due: step 1 fails on "plane 2 differs from a full
    forward's";
  * the dilation-4 liveness rule dropped (tapmask all ones: every (tile, tap) pair issues its MFMAs): test_deep_chain still passes —
    a product with an all-zero image row changes an accumulator only where it holds -0.0 — and all four cases of
    test_dropped_taps_issue_no_mfma fail on "tile .. of plane 9 differs where taps .. are dropped" (infinite weights in exactly
    the dropped taps turn a superfluous product into a NaN).
The library as committed passes every case."""
import pytest
import torch

from tests import incr3_ref as R
from tests.incr_harness import Stem, check_order as _check_order, distinct_pack, one_launch as _one_launch
from tests.kernel_harness import DEV, SENT32

pytestmark = pytest.mark.gpu
MASK, ROWS, STEPS = 4, 16, 12


@pytest.fixture(scope="module")
def cnn_pack():
    return distinct_pack()


_SCRIPTS = {}


def _script(L):
    """tokens [STEPS + 1][ROWS][L] u8 (CPU), built once per length: state 0 belongs to the full forward, state t follows the t-th set
    of changes."""
    if L in _SCRIPTS:
        return _SCRIPTS[L]
    g = torch.Generator().manual_seed(31 + L)
    x = torch.randint(0, 4, (ROWS, L), generator=g, dtype=torch.int64)
    x[torch.rand(ROWS, L, generator=g) < 0.5] = MASK
    states = [x.clone()]

    def bump(r, pos, k=1):                                          # a real change: never the token that is there
        for p in pos:
            x[r, p] = (x[r, p] + k) % 5

    def some(n):
        return [int(p) for p in torch.randperm(L, generator=g)[:n]]

    for t in range(1, STEPS + 1):
        if t in (1, 5): bump(1, [0])
        if t in (1, 4): bump(2, [L - 1])
        if t in (1, 3): bump(3, [L // 2])
        if t in (1, 6): bump(4, [1, L - 2])
        if t in (1, 2): bump(5, [40, 56])
        if t in (2, 7): bump(6, range(L), k=t)
        if t % 2: bump(7, some(1 + t % 3))
        for r in range(8, ROWS):
            bump(r, some(int(torch.randint(0, 4, (1,), generator=g))))
        if t >= 8:
            for r in range(1, 7):
                bump(r, some(t % 3))
        states.append(x.clone())
    d = [a != b for a, b in zip(states, states[1:])]
    assert not any(bool(s[0].any()) for s in d)
    assert d[0][1].nonzero().flatten().tolist() == [0] and d[0][2].nonzero().flatten().tolist() == [L - 1]
    assert d[0][3].nonzero().flatten().tolist() == [L // 2] and d[0][4].nonzero().flatten().tolist() == [1, L - 2] and L - 3 > 100
    assert d[0][5].nonzero().flatten().tolist() == [40, 56] and bool(d[1][6].all()) and bool(d[6][6].all())
    assert all(bool(d[t - 1][7].any()) == bool(t % 2) for t in range(1, STEPS + 1))
    _SCRIPTS[L] = [s.to(torch.uint8) for s in states]
    return _SCRIPTS[L]


def _stem(pk, L, depth, max_item):
    return Stem("svdd_backbone_incr3_f32", pk, ROWS, L, depth, max_item)


CASES = [(200, 2, 12), (200, 1, 12), (200, 4, 12), (200, 2, 9), (200, 2, 10), (208, 2, 12), (193, 2, 12), (105, 2, 12)]


@pytest.mark.parametrize("L,max_item,depth", CASES)
def test_deep_chain(cnn_pack, L, max_item, depth):
    pk = cnn_pack
    states = _script(L)
    dev = [s.to(DEV) for s in states]
    st, fresh = _stem(pk, L, depth, max_item), _stem(pk, L, depth, max_item)
    D, lead = depth, st.lead
    assert lead == 8 and list(pk["dil"][8:12]) == [4] * 4
    in_seq = torch.zeros(D, ROWS, 208, 128, dtype=torch.bool, device=DEV)
    in_seq[:, :, :L] = True
    keep = in_seq.reshape(-1)

    got = st.run(dev[0], True)
    assert torch.equal(got, _one_launch(dev[0], pk))
    st.planes.assert_written_where("planes after the full forward", in_seq)
    st.x_prev.assert_written("x_prev")
    for b in (st.items, st.order, st.count):
        b.assert_untouched("the lists after the full forward")
    marked = [0, 0]
    for t in range(1, STEPS + 1):
        what = f"L = {L}, items <= {max_item}, depth {depth}, step {t}"
        tok = dev[t]
        items, masks = R.expected_items(states[t - 1].numpy(), states[t].numpy(), L, pk["dil"], D, max_item)
        items, masks = torch.from_numpy(items), torch.from_numpy(masks)
        marked[0] += int(masks[:lead].sum())
        marked[1] += int(masks[lead:].sum())
        # tiles of planes 1 .. D - 1 that this step neither writes (mask of the plane) nor reads (the next layer's tiles + halo)
        read = masks.clone()
        read[:, :, 1:] |= masks[:, :, :-1]
        read[:, :, :-1] |= masks[:, :, 1:]
        idle = ~masks
        idle[:-1] &= ~read[1:]
        idle[-1] = False                                            # the tail reads every row of the last plane
        poison = (idle.repeat_interleave(16, dim=2)[..., None].expand(D, ROWS, 208, 128).to(DEV) & in_seq).reshape(-1)
        saved = (st.planes.bits().clone(), st.x_prev.bits().clone())
        st.planes.bits()[poison] = SENT32
        poisoned = st.planes.bits().clone()
        got = st.run(tok, False)
        assert torch.equal(st.lists()[0], items), f"{what}: work list"
        st.items.assert_written(f"{what}: work list")
        st.count.assert_written(f"{what}: order_count")
        ents = _check_order(st, what)
        left = st.planes.untouched()
        assert bool(left[poison].all()), f"{what}: a tile outside the mask was written"
        assert bool(left[~keep].all()), f"{what}: rows >= L of a plane were written"
        after = st.planes.bits().clone()
        after[poison] = saved[0][poison]
        st.planes.bits().copy_(after)
        ref = _one_launch(tok, pk)
        assert torch.equal(st.x_prev.body().view(ROWS, L), tok)
        assert torch.equal(fresh.run(tok, True), ref)
        bad = (after != fresh.planes.bits()) & keep
        assert not bool(bad.any()), f"{what}: plane {int(bad.nonzero()[0]) // (ROWS * 208 * 128) + 1} differs from a full forward's"
        assert torch.equal(got, ref), f"{what}: logits differ at row {int((got != ref).flatten(1).any(1).nonzero()[0])}"
        # the same step again from the saved state: the same bits
        st.planes.bits().copy_(poisoned)
        st.x_prev.bits().copy_(saved[1])
        for b in (st.items, st.order, st.count):
            b.bits().fill_(SENT32)
        again = st.run(tok, False)
        assert torch.equal(again, got) and torch.equal(st.lists()[0], items), f"{what}: two calls differ"
        assert all(torch.equal(a, b) for a, b in zip(_check_order(st, what + " (again)"), ents))
        again_planes = st.planes.bits().clone()
        again_planes[poison] = saved[0][poison]
        assert torch.equal(again_planes, after), f"{what}: two calls differ in the planes"
        st.planes.bits().copy_(after)
    assert st.stat.tolist() == [2 * marked[0], 2 * marked[1]]      # every step ran twice
    assert fresh.stat.tolist() == [0, 0]                           # a first = 1 forward marks nothing


@pytest.mark.parametrize("L,taps,tile", [(200, (6, 7, 8), 12), (200, (0,), 0), (208, (8,), 12), (193, (5, 6, 7, 8), 12)])
def test_dropped_taps_issue_no_mfma(cnn_pack, L, taps, tile):
    """A (row tile, tap) pair that backbone_kernel's schedule drops at dilation 4 must issue no MFMA in the segment kernel either.
    With finite weights a superfluous product of zero rows changes no bit, so the weights of exactly the dropped taps of layer 9
    are set to + inf here: 0 x inf is a NaN. The tile that drops them stays finite in the one-launch forward and must come out of
    the segment launch with the same bits; its neighbours, for which the taps are live, are not finite."""
    assert sorted(set(range(9)) - set(R.live_taps(L, tile, 4))) == list(taps)
    pk = dict(cnn_pack)
    nl = len(pk["dil"])
    pk["tiles"] = pk["tiles"].clone()
    w = pk["tiles"][:nl * 4 * 9 * 128 * 32].view(nl, 4, 9, 128, 32)
    for t in taps:
        w[8, :, t] = float("inf")
    states = _script(L)
    dev = [s.to(DEV) for s in states]
    st, fresh = _stem(pk, L, 9, 2), _stem(pk, L, 9, 2)
    st.run(dev[0], True)
    st.run(dev[1], False)                                           # rows 1 and 2 changed at 0 and at L - 1: both end tiles are marked
    fresh.run(dev[1], True)
    rows = slice(16 * tile, min(16 * tile + 16, L))
    plane = lambda s: s.planes.bits().view(9, ROWS, 208, 128)[8]
    items = st.lists()[0][8]
    for r in (1, 2):
        marked = [(int(e) & 255, int(e) >> 8) for e in items[r] if int(e)]
        assert any(t0 <= tile < t0 + n for t0, n in marked) == (r == (1 if tile == 0 else 2))
    r = 1 if tile == 0 else 2
    want = plane(fresh)[r, rows]
    # relu(conv) = plane 9 - plane 8: finite and not all zero in the tile that drops the taps; where the taps are live every sum holds
    # an inf (-> inf) or infs of both signs (-> NaN, which the ReLU's fmaxf turns into 0) — so in the neighbouring tile it is 0 or inf
    p8 = lambda sl: fresh.planes.body().view(9, ROWS, 208, 128)[7, r, sl]
    conv = want.view(torch.float32) - p8(rows)
    assert bool(torch.isfinite(conv).all()) and bool((conv != 0).any())
    other = slice(16, 32) if tile == 0 else slice(16 * tile - 16, 16 * tile)
    conv_other = plane(fresh)[r, other].view(torch.float32) - p8(other)
    assert bool(((conv_other == 0) | torch.isinf(conv_other)).all())
    assert torch.equal(plane(st)[r, rows], want), f"L = {L}: tile {tile} of plane 9 differs where taps {taps} are dropped"


def test_mc_decode_deep_planes_is_bit_identical():
    """SVDD-MC at B = 256, L = 200, M = 10, 32 steps: 12 carried layers, 8 carried layers and the one-launch kernel give the same
    tokens and the same logits and scores at every step; the executed share of the dilation-4 layers is on record in skip_stats."""
    from svdd_amd import synthetic
    model, emb, head, reward = synthetic.build("dna", DEV)
    model.rng_mode, model.philox_seed = "philox", 3
    B, M, S = 256, 10, 32
    runs = {}
    for name, mode, depth in (("off", "off", "auto"), ("8", "on", 8), ("12", "on", 12)):
        model.incremental_backbone, model.incremental_depth, model.trace, model.skip_stats = mode, depth, [], {}
        torch.manual_seed(0)
        x0 = model.controlled_sample(emb, head, num_steps=S, eval_sp_size=B, sample_M=M)
        torch.cuda.synchronize()
        runs[name] = (x0, model.trace, dict(model.skip_stats))
    model.incremental_backbone, model.incremental_depth, model.trace, model.skip_stats = "auto", "auto", None, None
    for name in ("8", "12"):
        assert torch.equal(runs[name][0], runs["off"][0])
        assert len(runs[name][1]) == len(runs["off"][1]) >= S
        for (la, sa), (lb, sb) in zip(runs[name][1], runs["off"][1]):
            assert torch.equal(la, lb) and (sa is None) == (sb is None) and (sa is None or torch.equal(sa, sb))
    s8, s12 = runs["8"][2], runs["12"][2]
    forwards = len(runs["12"][1]) - 1
    assert 0 < s12["backbone_deep_tile_layers"] < s12["backbone_deep_tile_layers_dense"] == forwards * B * 13 * 4
    assert s8["backbone_deep_tile_layers"] == 0 == s8["backbone_deep_tile_layers_dense"]
    for key in ("backbone_stem_tile_layers", "backbone_stem_tile_layers_dense"):
        assert s12[key] == s8[key]
    assert s12["backbone_stem_tile_layers_dense"] == forwards * B * 13 * 8
    print(f"DEEP executed tile-layers {s12['backbone_deep_tile_layers']} of {s12['backbone_deep_tile_layers_dense']}; "
          f"stem {s12['backbone_stem_tile_layers']} of {s12['backbone_stem_tile_layers_dense']}")
    assert "backbone_deep_tile_layers" not in runs["off"][2]
    with pytest.raises(ValueError):
        model.incremental_depth = 13
        model.controlled_sample(emb, head, num_steps=2, eval_sp_size=B, sample_M=M)
    model.incremental_depth = "auto"
