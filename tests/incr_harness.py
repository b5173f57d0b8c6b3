"""What the GPU files of the incremental backbone (tests/test_backbone_incremental_gpu.py, tests/test_backbone_incr{2,3,4}_gpu.py) share:
the backbone with distinct layers, the one-launch reference, one carried stem in sentinel-guarded buffers for any of the four
entries, and the contract of the size-ordered list."""
import ctypes

import torch

from svdd_amd import _lib, fused
from tests import net_ref as N
from tests.kernel_harness import DEV, _Buf, _st


def distinct_pack():
    """fused.pack_backbone of an H = 128 CNNModel with 20 DISTINCT layers (net_ref.distinct_layers)."""
    from svdd_amd import backbone, config
    torch.manual_seed(11)
    cnn = N.distinct_layers(backbone.CNNModel(config.dna_config().model, alphabet_size=5).eval(), 3).to(DEV)
    return fused.pack_backbone(cnn)


def slots(max_item):
    return 13 if max_item == 1 else 7


def one_launch(tok, pk):
    out = torch.empty((tok.shape[0], tok.shape[1], 5), dtype=torch.float32, device=DEV)
    dil = (ctypes.c_int * len(pk["dil"]))(*pk["dil"])
    _lib.call("svdd_backbone_cnn_f32", tok, pk["table0"], pk["tiles"], pk["vec"], pk["w2"], out, tok.shape[0], tok.shape[1],
              len(pk["dil"]), dil, None, None, 0)
    return out


class Stem:
    """Sentinel-guarded buffers of one carried stem of n rows and `depth` planes (None: the leading dilation-1 layers), and the calls
    of `entry` on them: every call synchronises and asserts both guards of every buffer, the ones the entry does not take included.
    stat: how many counters the entry is given (0: NULL). tok = (x_prev, x_prev2) is svdd_backbone_incr4_f32's token pair; `parity`
    names the one that holds the tokens and flips with every incremental forward of that entry."""

    def __init__(self, entry, pk, n, L, depth=None, max_item=2, stat=2):
        self.entry, self.pk, self.n, self.L, self.mi, self.S = entry, pk, n, L, max_item, slots(max_item)
        self.lead = fused.leading_dilation1(pk["dil"])
        self.D = D = self.lead if depth is None else depth
        self.planes, self.items = _Buf(D * n * 208 * 128), _Buf(D * n * self.S, torch.int32)
        self.order, self.count = _Buf(D * n * self.S, torch.int32), _Buf(D, torch.int32)
        self.x_prev, self.x_prev2, self.out = _Buf(n * L, torch.uint8), _Buf(n * L, torch.uint8), _Buf(n * L * 5)
        self.tok, self.parity = (self.x_prev, self.x_prev2), 0
        self.stat = torch.zeros(stat, dtype=torch.int64, device=DEV) if stat else None
        self.dil = (ctypes.c_int * len(pk["dil"]))(*pk["dil"])

    def _call(self, entry, tok, first):
        pk = self.pk
        lists = (self.order.ptr, self.count.ptr)
        extra = {"svdd_backbone_incr_f32": (), "svdd_backbone_incr2_f32": lists, "svdd_backbone_incr3_f32": lists + (self.D,),
                 "svdd_backbone_incr4_f32": lists + (self.D, self.x_prev2.ptr, self.parity)}[entry]
        _lib.call(entry, tok, pk["table0"], pk["tiles"], pk["vec"], pk["w2"], self.out.ptr, self.n, self.L, len(pk["dil"]), self.dil,
                  self.lead, self.planes.ptr, self.x_prev.ptr, self.items.ptr, self.stat, int(first), self.mi, *extra, _st())
        torch.cuda.synchronize()
        if entry == "svdd_backbone_incr4_f32":
            self.parity ^= 0 if first else 1
        for b in (self.planes, self.items, self.order, self.count, self.x_prev, self.x_prev2, self.out):
            b.untouched()                                           # asserts both guards of the buffer
        return self.out.body().view(self.n, self.L, 5).clone()

    def run(self, tok, first):
        return self._call(self.entry, tok, first)

    def run_old(self, tok, first):
        """The same arguments to the slot-ordered svdd_backbone_incr_f32."""
        return self._call("svdd_backbone_incr_f32", tok, first)

    def lists(self):
        """items [D][n][S], order_count [D], order [D][n * S] on the CPU."""
        return (self.items.body().view(self.D, self.n, self.S).cpu(), self.count.body().cpu(),
                self.order.body().view(self.D, self.n * self.S).cpu())


def check_order(st, what):
    """order_count, the multiset and the size order of `order` against `items`. -> the sorted entries per layer."""
    items, count, order = st.lists()
    rows = torch.arange(st.n, dtype=torch.int32)[None, :, None].expand_as(items)
    ents = []
    for k in range(st.D):
        live = items[k] != 0
        c = int(count[k])
        assert c == int(live.sum()), f"{what}: order_count[{k}] = {c}, {int(live.sum())} non-empty slots"
        want = (rows[k][live] << 16 | items[k][live]).sort().values
        got = order[k, :c]
        assert torch.equal(got.sort().values, want), f"{what}: order[{k}] is not the set of non-empty (row, item) pairs"
        tiles = (got >> 8) & 0xFF
        assert bool((tiles[1:] <= tiles[:-1]).all()), f"{what}: tile counts increase along order[{k}]"
        ents.append(want)
    return ents
