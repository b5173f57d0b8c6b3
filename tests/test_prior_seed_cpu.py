"""No GPU: what the seeded prior keeps and when it lets go of it. The all-MASK row's results (the backbone's carried planes and
logits, the value net's tower output and score) are keyed by the weights — they live ON the fused nets, which Diffusion's
weight-validated cache rebuilds when a weight changes — and by (L, depth, tight, mask) / (L, precision, mask); nothing a sampler
draws (seed, RNG mode, row offset, torch's generators) is part of a key. And svdd_backbone_incr_seed_f32 answers SVDD_E_ARG, before
any HIP call, for what it cannot take."""
import ctypes

import pytest
import torch

from svdd_amd import _lib, fused, synthetic


def test_prior_seeds_builds_once_per_key_and_stays_small():
    seeds, built = fused.PriorSeeds(), []

    def build_of(k):
        return lambda: built.append(k) or ("row", k)

    keys = [(200, 10, True, 4), (105, 10, True, 4), (200, 8, True, 4), (200, 10, False, 4)]       # L, depth, tight each tell rows apart
    for k in keys:
        assert seeds.get(k, build_of(k)) == ("row", k)
    assert built == keys and seeds.builds == 4 and len(seeds) == 4
    for k in keys:                                                                                # ... and nothing else is asked
        assert seeds.get(k, build_of(k)) == ("row", k)
    assert built == keys and seeds.builds == 4
    seeds.get((208, 12, True, 4), build_of("fifth"))                                              # the set is bounded
    assert len(seeds) <= fused.PriorSeeds.MOST and seeds.builds == 5


@pytest.fixture(scope="module")
def nets():
    return synthetic.build("dna", "cpu")


@pytest.fixture()
def stub_forward(monkeypatch):
    """The first forward of the one-row stem without a device: counts its calls, records its arguments."""
    calls = []

    def fake(tokens, pk, st, out=None, max_item=None):
        calls.append((tuple(tokens.shape), st.lead + st.deep, st.tight, int(tokens[0, 0])))
        st.valid = True
        return torch.zeros((st.n, st.L, 5))
    monkeypatch.setattr(fused, "backbone_cnn_incremental", fake)
    return calls


def test_backbone_row_is_keyed_by_weights_length_depth_and_tight_only(nets, stub_forward):
    model = nets[0]
    fb = model._fused_backbone()
    planes, logits, tok = fb.prior_row(200, 10, True, mask=model.mask_index)
    assert tuple(planes.shape) == (10, 1, 208, 128) and tuple(logits.shape) == (1, 200, 5) and tuple(tok.shape) == (1, 200)
    assert bool((tok == model.mask_index).all()) and stub_forward == [((1, 200), 10, True, 4)]
    # nothing of the RNG: other seeds, the other mode, another row offset, torch's generator — the same fused net, the same row
    model.philox_seed, model.rng_mode, model.row_offset = 99, "philox", 7
    torch.manual_seed(123)
    assert model._fused_backbone() is fb and fb.prior_row(200, 10, True, mask=4)[0] is planes and len(stub_forward) == 1
    model.philox_seed, model.rng_mode, model.row_offset = 0, "replay", 0
    # every part of the key tells
    fb.prior_row(105, 10, True)
    fb.prior_row(200, 8, True)
    fb.prior_row(200, 10, False)
    assert stub_forward[1:] == [((1, 105), 10, True, 4), ((1, 200), 8, True, 4), ((1, 200), 10, False, 4)] and fb.prior_seeds.builds == 4
    # a weight written through .data (no version bump): the cache rebuilds the fused net, and the row with it
    p = next(model.backbone.parameters())
    p.data.view(-1)[0] += 0.5
    try:
        fb2 = model._fused_backbone()
        assert fb2 is not fb and len(fb2.prior_seeds) == 0
        assert fb2.prior_row(200, 10, True)[0] is not planes and len(stub_forward) == 5
    finally:
        p.data.view(-1)[0] -= 0.5
        model.clear_fused()


def test_value_row_is_keyed_by_weights_length_and_precision(nets, monkeypatch):
    model, emb, head, _ = nets
    calls = []

    def make():
        vn = fused.FusedValueNet(emb, head).eval()
        monkeypatch.setattr(vn, "forward_tokens", lambda tok: calls.append(("score", tuple(tok.shape), int(tok[0, 0]))) or torch.zeros(1, 1, 1),
                            raising=False)
        monkeypatch.setattr(vn, "parent_tower", lambda tok: calls.append(("tower", tuple(tok.shape), int(tok[0, 0]))) or torch.zeros(1, tok.shape[1], 64),
                            raising=False)
        return vn
    cache = model._fused.__class__()
    vn = cache.get("value", (emb, head), make, None)
    s, t = vn.prior_score(200), vn.prior_tower(200)
    assert tuple(s.shape) == (1,) and tuple(t.shape) == (1, 200, 64) and calls == [("score", (1, 200), 4), ("tower", (1, 200), 4)]
    torch.manual_seed(5)
    assert cache.get("value", (emb, head), make, None) is vn and vn.prior_score(200) is s and vn.prior_tower(200) is t and len(calls) == 2
    vn.prior_score(105)
    vn.precision = "bf16x3"
    vn.prior_score(200)
    vn.precision = "f32"
    assert len(calls) == 4 and vn.prior_score(200) is s
    p = next(head.parameters())
    p.data.view(-1)[0] += 0.25
    try:
        vn2 = cache.get("value", (emb, head), make, None)
        assert vn2 is not vn and len(vn2.prior_seeds) == 0
    finally:
        p.data.view(-1)[0] -= 0.25


def test_seed_entry_signature_and_refusals():
    sig = _lib.SIGNATURES["svdd_backbone_incr_seed_f32"]
    assert len(sig) == 12 and sig[-1] is _lib.vp and _lib.STREAM not in sig            # the stream is the caller's (`on_stream`)
    L_ = _lib.lib()
    buf = (ctypes.c_char * 64)()
    a = ctypes.addressof(buf)
    a += -a % 16
    ok = dict(row_planes=a, row_logits=a, row_x=a, n=2, L=200, depth=10, planes=a, out=a, x_prev=a, x_prev2=a + 16, parity=0)

    def rc(**kw):
        return L_.svdd_backbone_incr_seed_f32(*{**ok, **kw}.values(), None)
    for name in ("row_planes", "row_logits", "row_x", "planes", "out", "x_prev"):
        assert rc(**{name: None}) == _lib.E_ARG, name
    for kw in (dict(n=0), dict(L=104), dict(L=209), dict(depth=0), dict(depth=33), dict(parity=2), dict(parity=-1),
               dict(parity=1, x_prev2=None), dict(x_prev2=a), dict(planes=a + 4), dict(row_planes=a + 8), dict(n=1 << 30, depth=4)):
        assert rc(**kw) == _lib.E_ARG, kw
