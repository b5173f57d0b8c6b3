"""-m gpu: svdd_backbone_incr4_f32 — the incremental backbone with tight items in the dilation-1 layers (backbone_seg_tight_kernel,
the halo packed into one register slot), the work list and its size order built in one launch (backbone_list_kernel) and the carried
tokens in a ping-pong pair. Five rows, L = 105 (byte reads of the tokens), 200 and 208 (8 tokens per read), 8, 10 and 12 carried
layers, three incremental forwards whose change sets hit every path of the list: a row without a change, positions 0 and L - 1, two
positions 17 apart (their runs join) and 33 apart (they do not), four clusters that need 8 items and take the aligned fallback,
every position changed, a row that changes only in the third forward. After each forward: logits and every carried plane equal,
bit for bit, those of a fresh first = 1 forward of the same tokens; `items` equals the numpy restatement (tests/incr4_ref.py);
order / order_count keep svdd_backbone_incr2_f32's contract; nothing outside the items' tiles changed in any plane, no row >= L and
no guard was written; the tokens moved to the other buffer of the pair; a repeated call from the restored state writes the same
lists and the same bits. A short SVDD-MC decode gives the same tokens with tight items, aligned items and the stem off."""
import pytest
import torch

from svdd_amd import fused
from tests import incr4_ref as R
from tests.incr_harness import Stem, check_order as _check_order, distinct_pack, one_launch as _one_launch
from tests.kernel_harness import DEV, SENT32

pytestmark = pytest.mark.gpu
MASK, ROWS, S = 4, 5, R.SEG_SLOTS


@pytest.fixture(scope="module")
def cnn_pack():
    return distinct_pack()


def _changes(L):
    """Per incremental forward, per row: the positions that change."""
    clusters = R.fallback_clusters(L) if L >= 200 else [8, 24, 59, 75]
    return [[[], [0, L - 1], [40, 57], clusters, []],
            [list(range(L)), [L // 2], [40, 73], [], []],
            [[3, 90, 91], [], [0], [L - 17, L - 1], [100]]]


def _states(L):
    """tokens [4][ROWS][L] u8 (CPU): state 0 belongs to the full forward, state t follows the t-th change set."""
    g = torch.Generator().manual_seed(41 + L)
    x = torch.randint(0, 4, (ROWS, L), generator=g, dtype=torch.int64)
    x[torch.rand(ROWS, L, generator=g) < 0.5] = MASK
    states = [x.clone()]
    for t, sets in enumerate(_changes(L)):
        for r, pos in enumerate(sets):
            x[r, pos] = (x[r, pos] + 1 + t) % 5                     # a real change: never the token that is there
        states.append(x.clone())
    return [s.to(torch.uint8) for s in states]


def _item_rows(items, lead, D):
    """bool [D][ROWS][208]: the rows of plane k that the items of layer k may write."""
    m = torch.zeros(D, ROWS, 208 + 16 * 2, dtype=torch.bool)
    for k in range(D):
        for r in range(ROWS):
            for e in items[k, r].tolist():
                if e:
                    o = (e & 255) if k < lead else 16 * (e & 255)
                    m[k, r, o:o + 16 * (e >> 8)] = True
    return m[:, :, :208]


@pytest.mark.parametrize("depth", [8, 10, 12])
@pytest.mark.parametrize("L", [105, 200, 208])
def test_tight_chain(cnn_pack, L, depth):
    pk = cnn_pack
    states = _states(L)
    dev = [s.to(DEV) for s in states]
    st, fresh = (Stem("svdd_backbone_incr4_f32", pk, ROWS, L, depth) for _ in range(2))
    D, lead = depth, st.lead
    assert lead == 8 and list(pk["dil"][8:12]) == [4] * 4
    in_seq = torch.zeros(D, ROWS, 208, 128, dtype=torch.bool, device=DEV)
    in_seq[:, :, :L] = True
    keep = in_seq.reshape(-1)

    got = st.run(dev[0], True)
    assert torch.equal(got, _one_launch(dev[0], pk))
    st.planes.assert_written_where("planes after the full forward", in_seq)
    st.tok[0].assert_written("the current token buffer")
    for b in (st.items, st.order, st.count, st.tok[1]):
        b.assert_untouched("the lists and the other token buffer after the full forward")
    cut = [0, 0]
    fell_back = False
    for t in (1, 2, 3):
        what = f"L = {L}, depth {depth}, forward {t}"
        tok = dev[t]
        items, tiles, fb = R.expected_items(states[t - 1].numpy(), states[t].numpy(), L, pk["dil"], lead, D)
        fell_back |= bool(fb.any())
        items = torch.from_numpy(items)
        cut[0] += int(tiles[:lead].sum())
        cut[1] += int(tiles[lead:].sum())
        before = st.planes.bits().clone()
        saved_tok, parity = (st.tok[0].bits().clone(), st.tok[1].bits().clone()), st.parity
        assert torch.equal(st.tok[parity].body().view(ROWS, L), dev[t - 1])
        got = st.run(tok, False)
        assert st.parity == parity ^ 1
        assert torch.equal(st.lists()[0], items), f"{what}: work list"
        st.items.assert_written(f"{what}: work list")
        st.count.assert_written(f"{what}: order_count")
        _check_order(st, what)
        assert torch.equal(st.tok[st.parity].body().view(ROWS, L), tok), f"{what}: the tokens did not move to the other buffer"
        assert torch.equal(st.tok[parity].bits(), saved_tok[parity]), f"{what}: the current token buffer was written"
        after = st.planes.bits().clone()
        assert bool(st.planes.untouched()[~keep].all()), f"{what}: rows >= L of a plane were written"
        may = _item_rows(items, lead, D)[..., None].expand(D, ROWS, 208, 128).to(DEV).reshape(-1)
        assert not bool(((after != before) & ~may).any()), f"{what}: a plane changed outside the items' tiles"
        ref = _one_launch(tok, pk)
        assert torch.equal(fresh.run(tok, True), ref)
        bad = (after != fresh.planes.bits()) & keep
        assert not bool(bad.any()), f"{what}: plane {int(bad.nonzero()[0]) // (ROWS * 208 * 128) + 1} differs from a full forward's"
        assert torch.equal(got, ref), f"{what}: logits differ at row {int((got != ref).flatten(1).any(1).nonzero()[0])}"
        # the same forward again with the planes, the token buffers and the parity put back: the same lists, the same bits
        lists = st.lists()
        st.planes.bits().copy_(before)
        for b, s in zip(st.tok, saved_tok):
            b.bits().copy_(s)
        st.parity = parity
        for b in (st.items, st.order, st.count):
            b.bits().fill_(SENT32)
        again = st.run(tok, False)
        assert torch.equal(again, got) and torch.equal(st.planes.bits(), after), f"{what}: two calls differ"
        c = lists[1].tolist()
        assert torch.equal(st.lists()[0], lists[0]) and st.lists()[1].tolist() == c
        assert all(torch.equal(st.lists()[2][k, :c[k]], lists[2][k, :c[k]]) for k in range(D)), f"{what}: two calls order differently"
    assert fell_back == (L >= 200)                                  # the slot fallback ran where a row can hold the four clusters
    assert st.stat.tolist() == [2 * cut[0], 2 * cut[1]]            # every forward ran twice
    assert fresh.stat.tolist() == [0, 0]                           # a first = 1 forward cuts nothing


def test_more_rows_than_one_workgroup_pass(cnn_pack):
    """n = 261: the list kernel takes 256 rows at a time, and packs the order from memory instead of from its registers."""
    pk, L, n, D = cnn_pack, 200, 261, 10
    g = torch.Generator().manual_seed(7)
    a = torch.randint(0, 5, (n, L), generator=g, dtype=torch.int64)
    b = a.clone()
    flip = torch.rand(n, L, generator=g) < 0.01
    flip[3], flip[258], flip[260] = False, False, False
    flip[258, [0, L - 1]] = True
    flip[260, R.fallback_clusters(L)] = True
    b[flip] = (b[flip] + 1) % 5
    st = fused.IncrementalStem(n, L, fused.leading_dilation1(pk["dil"]), DEV, D - 8, tight=True)
    a8, b8 = a.to(torch.uint8).to(DEV), b.to(torch.uint8).to(DEV)
    fused.backbone_cnn_incremental(a8, pk, st)
    got = fused.backbone_cnn_incremental(b8, pk, st)
    assert torch.equal(got, _one_launch(b8, pk))
    want, tiles, fb = R.expected_items(a.numpy(), b.numpy(), L, pk["dil"], 8, D)
    items = st.items.view(-1)[:D * n * S].view(D, n, S).cpu()
    assert torch.equal(items, torch.from_numpy(want)) and fb[0, 260]
    assert st.stat.tolist() == [int(tiles[:8].sum()), int(tiles[8:].sum())]
    order, count = st.order.view(-1)[:D * n * S].view(D, n * S).cpu(), st.order_count.cpu()
    rows = torch.arange(n, dtype=torch.int32)[:, None].expand(n, S)
    for k in range(D):
        live = items[k] != 0
        assert int(count[k]) == int(live.sum())
        ent = order[k, :int(count[k])]
        assert torch.equal(ent.sort().values, (rows[live] << 16 | items[k][live]).sort().values)
        size = (ent >> 8) & 0xFF
        assert bool((size[1:] <= size[:-1]).all())
        for c in (1, 2):                                            # inside a size class: (row, slot) order, as backbone_order_kernel
            assert torch.equal(ent[size == c], (rows[live] << 16 | items[k][live])[(items[k][live] >> 8) == c])
    assert torch.equal(st.x_prev2, b8) and st.parity == 1


def test_stem_object_flips_the_parity(cnn_pack):
    """fused.backbone_cnn_incremental on a tight IncrementalStem: same logits as the aligned stem, the tokens alternate buffers."""
    pk, L = cnn_pack, 200
    dev = [s.to(DEV) for s in _states(L)]
    lead = fused.leading_dilation1(pk["dil"])
    tight, aligned = fused.IncrementalStem(ROWS, L, lead, DEV, 2, tight=True), fused.IncrementalStem(ROWS, L, lead, DEV, 2)
    for t, tok in enumerate(dev):
        a, b = fused.backbone_cnn_incremental(tok, pk, tight), fused.backbone_cnn_incremental(tok, pk, aligned)
        assert torch.equal(a, b) and torch.equal(a, _one_launch(tok, pk))
        assert tight.parity == t % 2 and torch.equal((tight.x_prev, tight.x_prev2)[tight.parity], tok)
    assert torch.equal(tight.planes[:, :, :L], aligned.planes[:, :, :L])
    assert 0 < int(tight.stat[0]) < int(aligned.stat[0]) and int(tight.stat[1]) == int(aligned.stat[1])


def test_mc_decode_is_token_identical():
    """SVDD-MC, B = 8, 8 steps, Philox, the stem forced on: tight items, aligned items and no stem decode the same tokens."""
    from svdd_amd import synthetic
    model, emb, head, reward = synthetic.build("dna", DEV)
    model.rng_mode, model.philox_seed = "philox", 5
    assert model.incremental_items in ("tight", "aligned")
    runs = {}
    try:
        for name, mode, items in (("off", "off", "tight"), ("tight", "on", "tight"), ("aligned", "on", "aligned")):
            model.incremental_backbone, model.incremental_items, model.skip_stats = mode, items, {}
            torch.manual_seed(0)
            x0 = model.controlled_sample(emb, head, num_steps=8, eval_sp_size=8, sample_M=4)
            torch.cuda.synchronize()
            runs[name] = (x0, dict(model.skip_stats))
        model.incremental_items = "loose"
        with pytest.raises(ValueError):
            model.controlled_sample(emb, head, num_steps=2, eval_sp_size=8, sample_M=4)
    finally:
        model.incremental_backbone, model.incremental_items, model.skip_stats = "auto", "tight", None
    assert torch.equal(runs["tight"][0], runs["off"][0]) and torch.equal(runs["aligned"][0], runs["off"][0])
    t, a = runs["tight"][1], runs["aligned"][1]
    assert 0 < t["backbone_stem_tile_layers"] <= a["backbone_stem_tile_layers"] < a["backbone_stem_tile_layers_dense"]
    assert t["backbone_stem_tile_layers_dense"] == a["backbone_stem_tile_layers_dense"]
    print(f"STEM tile-layers tight {t['backbone_stem_tile_layers']}, aligned {a['backbone_stem_tile_layers']} "
          f"of {a['backbone_stem_tile_layers_dense']}")
