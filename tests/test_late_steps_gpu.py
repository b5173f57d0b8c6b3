"""-m gpu: the device-sized two-part late step (svdd_value_late_step_f32, FusedValueNet._late_step):
    tower(B) -> [GRU(B) || tower(A)] in one launch -> GRU(A) -> tail(all live rows),
with one GRU round shrunk to 32 rows (FusedValueNet.GRU_ROUND_ROWS) so that 48 candidates outgrow it (and GRU_SECOND_PART widened to
1/2 so that _gru_split, whose 5/16 rule would refuse 32 + 16, lets the case through — the rule itself is not what is tested). Live
counts 20 (B empty), 32 (A exactly full, B empty), 37 (B one ragged tile of 5) and 48, at L = 105 and 200: the score of every live
candidate equals, bit for bit, the one-part path's (split_gru_rounds = False); the device counts are (k, min(k, 32), max(k - 32, 0));
no row past the count is written in the scores, the tower output or the GRU output. A 12-step SVDD-MC decode at B = 4, M = 12
returns the same tokens and the same traced scores both ways."""
import pytest
import torch

from svdd_amd import ops, synthetic
from svdd_amd.diffusion import Diffusion
from svdd_amd.fused import FusedValueNet
from tests.kernel_harness import DEV

pytestmark = pytest.mark.gpu
MASK, B, M = 4, 4, 12
SENT = -1234.5


@pytest.fixture(scope="module")
def nets():
    return synthetic.build("dna", DEV)


@pytest.fixture()
def small_round(monkeypatch):
    monkeypatch.setattr(FusedValueNet, "GRU_ROUND_ROWS", 32)
    monkeypatch.setattr(FusedValueNet, "GRU_SECOND_PART", (1, 2))


def _candidates(L, k):
    """x [B, L], cand [B, M, L] u8 with exactly k live candidates: changes at both ends, far apart (two tower parts), single ones."""
    g = torch.Generator().manual_seed(100 * L + k)
    x = torch.randint(0, 4, (B, L), generator=g, dtype=torch.uint8)
    x[torch.rand(B, L, generator=g) < 0.6] = MASK
    x[:, [0, L - 1, 3, L - 4]] = MASK
    cand = x[:, None, :].repeat(1, M, 1)
    live = torch.randperm(B * M, generator=g)[:k].tolist()
    for i, c in enumerate(live):
        row = cand[c // M, c % M]
        if i % 5 == 0:
            pos = [0, L - 1]                                                    # both ends: two parts at L = 200, one at 105
        elif i % 5 == 1:
            pos = [3, L - 4, L // 2]
        else:
            masked = (x[c // M] == MASK).nonzero().flatten()
            pos = masked[torch.randperm(len(masked), generator=g)[:1 + i % 3]].tolist()
        row[pos] = torch.randint(0, 4, (len(pos),), generator=g, dtype=torch.uint8)
    return x.to(DEV), cand.to(DEV).contiguous(), sorted(live)


def _scores(fn, onehot, cand, x, late):
    ws = Diffusion._SkipWorkspace(B, M, DEV)
    ws.late = ws.late_on_device = late
    sc = fn.candidate_scores_compact(onehot, cand, x, ws).reshape(-1)
    torch.cuda.synchronize()
    return sc, ws


@pytest.mark.parametrize("k", [20, 32, 37, 48])
@pytest.mark.parametrize("L", [105, 200])
def test_two_part_scores_equal_the_one_part_path(nets, small_round, L, k):
    model, emb, head, _ = nets
    fn = model.value_callable(emb, head)
    assert fn.tower_parts == "on" and fn._gru_split(B * M) == 32
    x, cand, live = _candidates(L, k)
    onehot = ops.transform_samples(cand.view(B * M, L))
    fn.split_gru_rounds = False
    try:
        ref, ws_ref = _scores(fn, onehot, cand, x, late=True)
    finally:
        fn.split_gru_rounds = True
    assert ws_ref.count3.tolist()[0] == k and sorted(ws_ref.live_idx[:k].tolist()) == live
    dense_ref = torch.full((B * M,), float("nan"), device=DEV)
    dense_ref[ws_ref.live_idx[:k].long()] = ref[:k]
    _scores(fn, onehot, cand, x, late=True)                                     # allocates the path's buffers
    sb = fn._split_bufs[("late", B * M, L, DEV)]
    for t in sb.values():
        t.fill_(SENT)
    got, ws = _scores(fn, onehot, cand, x, late=True)
    assert ws.split_bufs is sb and got.data_ptr() == sb["sc"].data_ptr() and ws.seq is sb["seq"]
    assert ws.count3.tolist() == [k, min(k, 32), max(k - 32, 0)]
    assert sorted(ws.live_idx[:k].tolist()) == live
    dense = torch.full((B * M,), float("nan"), device=DEV)
    dense[ws.live_idx[:k].long()] = got[:k]
    assert torch.equal(dense[live], dense_ref[live]) and not bool(torch.isnan(dense[live]).any())
    # nothing past the count: scores, tower output, both directions of the GRU output
    assert bool((sb["sc"][k:] == SENT).all()) and bool((sb["seq"][k:] == SENT).all()) and bool((sb["h"][:, k:] == SENT).all())
    assert not bool((sb["seq"][:k] == SENT).any()) and not bool((sb["h"][:, :k] == SENT).any())
    # the tower output the select advances the parents from: the one-part path's rows, candidate by candidate
    order_ref = torch.argsort(ws_ref.live_idx[:k])
    order = torch.argsort(ws.live_idx[:k])
    assert torch.equal(sb["seq"][:k][order], ws_ref.seq[:k][order_ref])


def test_decode_same_tokens_with_the_two_part_steps_and_without(nets, small_round):
    model, emb, head, _ = nets
    model.rng_mode, model.philox_seed = "philox", 11
    fn = model.value_callable(emb, head)
    outs = []
    for on in (True, False):
        fn.split_gru_rounds, model.late_steps_from = on, "auto"
        fn.__dict__.pop("_split_bufs", None)
        model.trace = []
        x0 = model.controlled_sample(emb, head, num_steps=12, eval_sp_size=B, sample_M=M)
        torch.cuda.synchronize()
        outs.append((x0, [sc for _, sc in model.trace if sc is not None], "_split_bufs" in fn.__dict__))
        model.trace = None
    fn.split_gru_rounds = True
    assert outs[0][2] and not outs[1][2]                                        # the first decode did take the two-part steps
    assert torch.equal(outs[0][0], outs[1][0]) and len(outs[0][1]) == len(outs[1][1]) == 12
    for a, b in zip(outs[0][1], outs[1][1]):
        assert torch.equal(a, b)
