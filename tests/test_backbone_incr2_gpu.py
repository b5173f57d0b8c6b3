"""-m gpu: svdd_backbone_incr2_f32 — the incremental stem with its segment launches dealt from a compact, size-ordered list — gives
the bits of svdd_backbone_incr_f32 and of a fresh full forward, step after step, for work items of at most 1, 2 and 4 row tiles.

Chains of 4 steps on 8 rows at L = 105, 200 and 208 (H = 128 CNNModel, 20 DISTINCT layers: net_ref.distinct_layers). The rows:
  0  never changes                              1  changes at position 0 only          2  changes at position L - 1 only
  3  two changes 15 apart (8, 23: across the boundary 15 | 16) on odd steps, 17 apart (24, 41: across 31 | 32) on even steps
  4  every position changes (every tile in every layer; at L = 200 and 208 that is 13 one-tile items, why max_item 1 has 13 slots)
  5  changes at 40 and 104: their reaches leave tile 4 out up to layer 4 and merge from layer 5 on
  6, 7  one to three random changes per step, as a decode makes them
After every step: `out` and the planes equal the old entry's (run beside it on its own buffers; for max_item 1, which the old entry
refuses, the old entry runs with 2 — the cut changes no bit) and a fresh full forward's, bit for bit; `items` equals what the old
entry writes and the brute-force marking (tile T of plane k is marked iff a changed position lies within 4 + 4 k of one of T's
positions) cut into runs of at most max_item tiles; order_count[k] is the number of non-empty slots; order[k][:count] holds exactly
the non-empty (row, item) pairs; tile counts along the list never increase; the guards around every buffer are intact; the step
made again with x_prev put back gives the same out, planes, items, order_count and the same multiset in order.
One more case: 300 rows at L = 200, 2 steps, 5 changes per row, at residencies that leave fewer resident workgroup slots than items
(the dispatcher then hands later entries to CUs as they free up), compared with the one-launch kernel on all rows."""
import numpy as np
import pytest
import torch

from svdd_amd import _lib, fused
from tests.incr_harness import Stem, check_order as _check_lists, distinct_pack, one_launch as _one_launch, slots as _slots
from tests.kernel_harness import DEV, SENT32

pytestmark = pytest.mark.gpu
MASK, ROWS, STEPS = 4, 8, 4


@pytest.fixture(scope="module")
def cnn_pack():
    return distinct_pack()


def _script(L, seed):
    """tokens [STEPS + 1][ROWS][L] u8 (CPU): state 0 belongs to the full forward, state t follows the t-th set of changes."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 4, (ROWS, L), generator=g, dtype=torch.int64)
    x[torch.rand(ROWS, L, generator=g) < 0.5] = MASK
    states = [x.clone()]
    for t in range(1, STEPS + 1):
        def bump(r, pos, k=1):                                      # a real change: never the token that is there
            for p in pos:
                x[r, p] = (x[r, p] + k) % 5
        bump(1, [0])
        bump(2, [L - 1])
        bump(3, [8, 23] if t % 2 else [24, 41])
        bump(4, range(L), k=t)
        bump(5, [40, 104])
        for r in (6, 7):
            bump(r, [int(p) for p in torch.randperm(L, generator=g)[:1 + int(torch.randint(0, 3, (1,), generator=g))]])
        states.append(x.clone())
    for a, b in zip(states, states[1:]):
        d = a != b
        assert not d[0].any() and d[1].nonzero().flatten().tolist() == [0] and d[2].nonzero().flatten().tolist() == [L - 1]
        assert bool(d[4].all()) and d[5].nonzero().flatten().tolist() == [40, 104] and int(d[3].sum()) == 2
    return [s.to(torch.uint8) for s in states]


def _expected_items(prev, new, L, P, max_item):
    """[P][n][slots] int32 by brute force over (changed position, tile), and the tiles marked per layer."""
    n, S = prev.shape[0], _slots(max_item)
    items = np.zeros((P, n, S), dtype=np.int32)
    lo = 16 * np.arange(13)
    hi = np.minimum(lo + 15, L - 1)
    for r in range(n):
        c = (prev[r] != new[r]).nonzero().flatten().numpy()
        for k in range(1, P + 1):
            reach = 4 + 4 * k
            mask = ((c[:, None] >= lo[None] - reach) & (c[:, None] <= hi[None] + reach)).any(0) & (lo <= L - 1)
            t = cnt = 0
            while t < 13:
                if not mask[t]:
                    t += 1
                    continue
                ln = 1
                while ln < max_item and t + ln < 13 and mask[t + ln]:
                    ln += 1
                items[k - 1, r, cnt] = t | ln << 8
                cnt, t = cnt + 1, t + ln
    return torch.from_numpy(items)


def _stem(pk, n, L, max_item):
    """run() goes to the ordered entry, run_old() to svdd_backbone_incr_f32; stat is NULL."""
    return Stem("svdd_backbone_incr2_f32", pk, n, L, None, max_item, stat=0)


@pytest.fixture(autouse=True)
def _library_residency():
    yield
    fused.set_incr_residency(0)


@pytest.mark.parametrize("max_item", [1, 2, 4])
@pytest.mark.parametrize("L", [105, 200, 208])
def test_ordered_chain(cnn_pack, L, max_item):
    pk = cnn_pack
    states = _script(L, 7 + L)
    dev = [s.to(DEV) for s in states]
    new, old = _stem(pk, ROWS, L, max_item), _stem(pk, ROWS, L, max(max_item, 2))
    P = new.D
    assert P == 8
    ref = old.run_old(dev[0], True)
    assert torch.equal(new.run(dev[0], True), ref)
    assert torch.equal(new.planes.bits(), old.planes.bits())
    for b in (new.items, new.order, new.count):
        b.assert_untouched("the lists after the full forward")
    for t in range(1, STEPS + 1):
        what = f"L = {L}, items <= {max_item}, step {t}"
        prev_tokens = new.x_prev.bits().clone()
        got, ref = new.run(dev[t], False), old.run_old(dev[t], False)
        assert torch.equal(got, ref), f"{what}: out differs from the old entry's"
        assert torch.equal(new.planes.bits(), old.planes.bits()), f"{what}: planes differ from the old entry's"
        fresh = _stem(pk, ROWS, L, max_item)
        assert torch.equal(fresh.run(dev[t], True), got), f"{what}: out differs from a full forward's"
        assert torch.equal(new.planes.bits(), fresh.planes.bits()), f"{what}: planes differ from a full forward's"
        assert torch.equal(new.x_prev.body().view(ROWS, L), dev[t])
        items, count, _ = new.lists()
        new.items.assert_written(f"{what}: work list")
        new.count.assert_written(f"{what}: order_count")
        assert torch.equal(items, _expected_items(states[t - 1], states[t], L, P, max_item)), f"{what}: work list"
        if max_item != 1:
            assert torch.equal(items, old.lists()[0]), f"{what}: items differ from the old entry's"
        else:
            assert int((items[:, 4] != 0).sum()) == -(-L // 16) * P  # the row that changed everywhere: every tile a one-tile item (13 at L > 192)
        ents = _check_lists(new, what)
        # the same step again: x_prev put back, lists cleared
        planes = new.planes.bits().clone()
        new.x_prev.bits().copy_(prev_tokens)
        for b in (new.items, new.order, new.count):
            b.bits().fill_(SENT32)
        again = new.run(dev[t], False)
        assert torch.equal(again, got) and torch.equal(new.planes.bits(), planes), f"{what}: two calls differ"
        assert torch.equal(new.lists()[0], items) and torch.equal(new.lists()[1], count), f"{what}: two calls differ in the lists"
        assert all(torch.equal(a, b) for a, b in zip(_check_lists(new, what + " (again)"), ents))


@pytest.mark.parametrize("max_item,residency", [(2, 2), (1, 3), (4, 1), (2, 0)])
def test_more_items_than_resident_slots(cnn_pack, max_item, residency):
    pk, n, L = cnn_pack, 300, 200
    g = torch.Generator().manual_seed(100 + max_item)
    x = torch.randint(0, 5, (n, L), generator=g, dtype=torch.int64)
    states = [x.clone()]
    for t in range(2):
        for r in range(n):
            for p in torch.randperm(L, generator=g)[:5].tolist():
                x[r, p] = (x[r, p] + 1 + t) % 5
        states.append(x.clone())
    states = [s.to(torch.uint8) for s in states]
    dev = [s.to(DEV) for s in states]
    fused.set_incr_residency(residency)
    st = _stem(pk, n, L, max_item)
    assert torch.equal(st.run(dev[0], True), _one_launch(dev[0], pk))
    ncu = _lib.device_info()[1]
    for t in (1, 2):
        got = st.run(dev[t], False)
        ref = _one_launch(dev[t], pk)
        assert torch.equal(got, ref), f"step {t}: rows {(got != ref).flatten(1).any(1).nonzero().flatten().tolist()[:8]} differ"
        assert torch.equal(st.lists()[0], _expected_items(states[t - 1], states[t], L, st.D, max_item))
        _check_lists(st, f"n = 300, items <= {max_item}, step {t}")
        if residency:
            assert int(st.lists()[1].min()) > residency * ncu       # every layer's launch has more items than resident slots
