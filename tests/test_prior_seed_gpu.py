"""-m gpu: the seeded prior. svdd_backbone_incr_seed_f32 broadcasts ONE all-MASK row's first-forward state (carried planes, logits,
tokens) into a carried stem of n rows; the state must be, bit for bit, what the first = 1 forward of n all-MASK rows leaves: rows
< L of every plane, the logits, the current token buffer — and nothing else written (rows >= L, the other token buffer, the lists,
stat, every guard), the parity unchanged. One incremental forward after the same token change then gives the same logits and
planes from both states. Random-init backbone with distinct layers (tests/incr_harness.py); n = 129 (the smallest batch the sampler
routes through the stem by itself) and n = 5; L = 200 and 105; depth 8 (the dilation-1 run) and 10; the aligned and the tight entry.
Above the entry: the fused nets' cached rows equal a fresh evaluation of one all-MASK row and miss after a weight change, and a short
SVDD-MC decode through the stem gives the same tokens, logits and scores with the seeding on (cold and warm cache) and off."""
import pytest
import torch

from svdd_amd import _lib, fused, ops
from tests.incr_harness import Stem, distinct_pack
from tests.kernel_harness import DEV, _st

pytestmark = pytest.mark.gpu
MASK = 4
ENTRIES = {"aligned": "svdd_backbone_incr3_f32", "tight": "svdd_backbone_incr4_f32"}


@pytest.fixture(scope="module")
def cnn_pack():
    return distinct_pack()


@pytest.fixture(scope="module")
def source_rows(cnn_pack):
    """(entry kind, L, depth) -> the one-row stem after its first forward of the all-MASK row (computed once, never written again)."""
    rows = {}

    def get(kind, L, depth):
        key = (kind, L, depth)
        if key not in rows:
            st = Stem(ENTRIES[kind], cnn_pack, 1, L, depth)
            st.run(torch.full((1, L), MASK, dtype=torch.uint8, device=DEV), True)
            rows[key] = st
        return rows[key]
    return get


def _seed(st, src, parity):
    _lib.call("svdd_backbone_incr_seed_f32", src.planes.ptr, src.out.ptr, src.tok[src.parity].ptr, st.n, st.L, st.D, st.planes.ptr,
              st.out.ptr, st.x_prev.ptr, st.x_prev2.ptr, parity, _st())
    torch.cuda.synchronize()


def _same_state(a, b, what):
    for name in ("planes", "out", "x_prev", "x_prev2", "items", "order", "count"):
        ba, bb = getattr(a, name), getattr(b, name)
        ba.untouched(), bb.untouched()                                        # asserts both guards of each
        assert torch.equal(ba.bits(), bb.bits()), f"{what}: {name} differs"
    assert torch.equal(a.stat, b.stat) and a.parity == b.parity, what


@pytest.mark.parametrize("kind", ["aligned", "tight"])
@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("L", [200, 105])
@pytest.mark.parametrize("n", [129, 5])
def test_seeded_stem_equals_first_forward(cnn_pack, source_rows, n, L, depth, kind):
    assert n in (5, fused.BB_SPLIT_MAX_SEQ + 1)
    what = f"{kind}, n = {n}, L = {L}, depth {depth}"
    src = source_rows(kind, L, depth)
    ref, got = (Stem(ENTRIES[kind], cnn_pack, n, L, depth) for _ in range(2))
    if kind == "tight":
        ref.parity = got.parity = 1                                           # a stem that earlier decodes left on the second buffer
    prior = torch.full((n, L), MASK, dtype=torch.uint8, device=DEV)
    lg_ref = ref.run(prior, True)
    _seed(got, src, got.parity)
    _same_state(got, ref, what)
    in_seq = torch.zeros(depth, n, 208, 128, dtype=torch.bool, device=DEV)
    in_seq[:, :, :L] = True
    got.planes.assert_written_where(f"{what}: planes", in_seq)
    got.out.assert_written(f"{what}: logits")
    got.tok[got.parity].assert_written(f"{what}: the current token buffer")
    assert torch.equal(got.tok[got.parity].body().view(n, L), prior)
    for b in (got.items, got.order, got.count, got.tok[got.parity ^ 1]):
        b.assert_untouched(f"{what}: the lists and the other token buffer")
    assert torch.equal(got.out.body().view(n, L, 5), lg_ref) and torch.equal(lg_ref[0], lg_ref[n - 1])
    # the same change of tokens from both states: positions at both ends, a cluster, a row changed everywhere, rows left alone
    g = torch.Generator().manual_seed(7 * n + L)
    nxt = prior.cpu().clone()
    nxt[0, [0, L - 1]] = 1
    nxt[1, 40:58] = torch.randint(0, 4, (18,), generator=g, dtype=torch.uint8)
    nxt[n - 1] = torch.randint(0, 4, (L,), generator=g, dtype=torch.uint8)
    nxt = nxt.to(DEV)
    la, lb = ref.run(nxt, False), got.run(nxt, False)
    assert torch.equal(la, lb), f"{what}: logits of the incremental forward differ"
    _same_state(got, ref, f"{what}, after one incremental forward")
    src.planes.untouched(), src.out.untouched()                               # the source's guards


def test_cached_rows_equal_a_fresh_evaluation_and_miss_after_a_weight_change():
    from svdd_amd import synthetic
    model, emb, head, _ = synthetic.build("dna", DEV)
    L = 200
    tok = torch.full((1, L), MASK, dtype=torch.uint8, device=DEV)
    fn = model.value_callable(emb, head)
    tower, score = fn.prior_tower(L, MASK), fn.prior_score(L, MASK)
    assert torch.equal(tower, fused.conv_tower(ops.transform_samples(tok), fn.tw_tiles, fn.tw_bias, fn.tw_resmask))
    assert torch.equal(score, fn.forward_tokens(tok).reshape(1))
    assert fn.prior_tower(L, MASK) is tower and fn.prior_score(L, MASK) is score and fn.prior_seeds.builds == 2
    fb = model._fused_backbone()
    for tight in (False, True):
        planes, logits, x1 = fb.prior_row(L, 10, tight, MASK)
        assert torch.equal(x1, tok) and torch.equal(logits, fb.forward_rows(tok))
        st = fused.IncrementalStem(1, L, 8, DEV, 2, tight)
        assert torch.equal(fused.backbone_cnn_incremental(tok, fb.ol_pack(), st), logits)
        assert torch.equal(st.planes[:, :, :L], planes[:, :, :L])
        assert fb.prior_row(L, 10, tight, MASK)[0] is planes
    assert fb.prior_seeds.builds == 2
    # one perturbed weight in each net: the weight-validated cache rebuilds the fused nets, and the rows are computed again
    pb, pv = model.backbone.convs[3].weight, next(head.parameters())
    pb.data.view(-1)[5] += 0.125
    pv.data.view(-1)[0] += 0.125
    fb2, fn2 = model._fused_backbone(), model.value_callable(emb, head)
    assert fb2 is not fb and fn2 is not fn and len(fb2.prior_seeds) == 0 and len(fn2.prior_seeds) == 0
    assert not torch.equal(fb2.prior_row(L, 10, True, MASK)[1], logits)
    assert torch.equal(fb2.prior_row(L, 10, True, MASK)[1], fb2.forward_rows(tok))
    assert torch.equal(fn2.prior_score(L, MASK), fn2.forward_tokens(tok).reshape(1)) and not torch.equal(fn2.prior_score(L, MASK), score)


def test_mc_decode_through_the_stem_is_the_same_seeded_and_not():
    from svdd_amd import synthetic
    model, emb, head, _ = synthetic.build("dna", DEV)
    model.rng_mode, model.philox_seed, model.incremental_backbone = "philox", 5, "on"
    B, M, S = 6, 4, 8
    outs = []
    for on in (True, True, False):                                            # cold cache, warm cache, the whole first forward
        model.dedup_prior, model.trace = on, []
        x0 = model.controlled_sample(emb, head, num_steps=S, eval_sp_size=B, sample_M=M)
        torch.cuda.synchronize()
        outs.append((x0, model.trace))
        model.trace = None
    model.dedup_prior = True
    fb, fn = model._fused_backbone(), model.value_callable(emb, head)
    assert fb.prior_seeds.builds == 1 and fn.prior_seeds.builds == 2         # one row each, computed by the first decode alone
    for x0, tr in outs[:2]:
        assert torch.equal(x0, outs[2][0]) and len(tr) == len(outs[2][1]) >= S   # (the noise-removal forward is traced too)
        for (la, sa), (lb, sb) in zip(tr, outs[2][1]):
            assert torch.equal(la, lb) and (sa is None) == (sb is None) and (sa is None or torch.equal(sa, sb))
        assert all(sa is not None for _, sa in tr[:S])
