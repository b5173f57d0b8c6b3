"""-m gpu: layer 1 of the incremental stem (backbone_seg_kernel builds f_0 from the step's tokens: nine table reads per element, now
issued together through the LDS image instead of one dependent, branch-guarded read after the other) keeps the bits.

n = 6 rows, L = 200 and 120, the repository's seeded backbone (synthetic.build). One full forward fills the carried planes, then
three consecutive incremental forwards. Per step the rows change as follows: row 0 never; row 1 at position 0, then L - 1, then
both (tokens outside the sequence are skipped taps, not added zeros); row 2 at 15, then 16, then both (the two sides of a tile edge);
row 3 at two positions 5 apart (their reaches of +-4 overlap); row 4 at one position, then at EVERY position, then at three; row 5
at a few random positions as a decode does. After every forward, for each of the entries and item sizes that run layer 1
(svdd_backbone_incr2_f32 with items of <= 2 and of 1 tile, svdd_backbone_incr_f32 with items of <= 2 and <= 4 tiles):
  * the logits are torch.equal to the one-launch kernel svdd_backbone_cnn_f32 on the same tokens (computed once per step);
  * the logits and ALL carried planes (rows < L) are torch.equal to those of a fresh first forward of the same tokens — plane 1 is
    layer 1's output, so a wrong f_0 shows there before anything else.
Plane 0 is not carried (layer 1 keeps the lookup): there is no f_0 buffer to compare."""
import ctypes

import pytest
import torch

from svdd_amd import _lib, fused, synthetic
from tests.kernel_harness import DEV

pytestmark = pytest.mark.gpu
N, MASK = 6, 4
VARIANTS = [("ordered", 2), ("ordered", 1), ("slot", 2), ("slot", 4)]


@pytest.fixture(scope="module")
def pack():
    model = synthetic.build("dna", DEV)[0]
    pk = model._fused_backbone().ol_pack()
    assert fused.leading_dilation1(pk["dil"]) >= 1
    return pk


def _states(L):
    g = torch.Generator().manual_seed(31 + L)
    x = torch.randint(0, 4, (N, L), generator=g, dtype=torch.int64)
    x[torch.rand(N, L, generator=g) < 0.6] = MASK
    states = [x.clone()]

    def bump(r, pos, k=1):                                            # a real change: never the token that is there
        for p in pos:
            x[r, p] = (x[r, p] + k) % 5

    for t in (1, 2, 3):
        bump(1, {1: [0], 2: [L - 1], 3: [0, L - 1]}[t])
        bump(2, {1: [15], 2: [16], 3: [15, 16]}[t])
        bump(3, {1: [60, 65], 2: [40, 45], 3: [L - 6, L - 1]}[t])
        bump(4, {1: [77], 2: range(L), 3: [2, 50, 99]}[t], k=t)
        bump(5, [int(p) for p in torch.randperm(L, generator=g)[:t]])
        states.append(x.clone())
    assert all(torch.equal(s[0], states[0][0]) for s in states) and bool((states[2][4] != states[1][4]).all())
    return [s.to(torch.uint8).to(DEV).contiguous() for s in states]


def _one_launch(tok, pk):
    out = torch.empty((tok.shape[0], tok.shape[1], 5), dtype=torch.float32, device=DEV)
    dil = (ctypes.c_int * len(pk["dil"]))(*pk["dil"])
    _lib.call("svdd_backbone_cnn_f32", tok, pk["table0"], pk["tiles"], pk["vec"], pk["w2"], out, tok.shape[0], tok.shape[1],
              len(pk["dil"]), dil, None, None, 0)
    return out


@pytest.mark.parametrize("L", [200, 120])
def test_layer1_lookup_keeps_the_bits(pack, L, monkeypatch):
    pk = pack
    lead = fused.leading_dilation1(pk["dil"])
    states = _states(L)
    refs = [_one_launch(s, pk) for s in states]                       # once per step, shared by every variant
    fresh = []                                                        # planes of a fresh first forward of every step's tokens
    for s, ref in zip(states, refs):
        st = fused.IncrementalStem(N, L, lead, DEV)
        monkeypatch.setattr(fused, "INCR_ORDERED", True)
        assert torch.equal(fused.backbone_cnn_incremental(s, pk, st, max_item=2), ref)
        fresh.append(st.planes[:, :, :L].clone())
    for kind, max_item in VARIANTS:
        monkeypatch.setattr(fused, "INCR_ORDERED", kind == "ordered")
        st = fused.IncrementalStem(N, L, lead, DEV)
        for t, (s, ref) in enumerate(zip(states, refs)):
            got = fused.backbone_cnn_incremental(s, pk, st, max_item=max_item)
            assert st.forwards == t
            bad = (got != ref).flatten(1).any(1).nonzero().flatten().tolist()
            assert not bad, f"{kind} list, items <= {max_item}, forward {t}: logits differ from the one-launch kernel in rows {bad}"
            diff = (st.planes[:, :, :L] != fresh[t]).flatten(2).any(2).nonzero().tolist()
            assert not diff, f"{kind} list, items <= {max_item}, forward {t}: (plane - 1, row) {diff[:4]} differ from a fresh forward's"
