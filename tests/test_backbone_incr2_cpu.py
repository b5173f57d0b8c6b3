"""No GPU: svdd_backbone_incr2_f32 answers SVDD_E_ARG — before its profile span and before any HIP call — for a NULL `order` or
`order_count`, an item size outside {1, 2, 4}, and everything svdd_backbone_incr_f32 already refuses; the residency setter takes
0 .. 8 only."""
import ctypes

from svdd_amd import _lib


def test_incr2_rejects_bad_arguments_without_a_gpu():
    L_ = _lib.lib()
    one = ctypes.c_void_p(64)                                # a non-NULL pointer that is never dereferenced
    dil8 = (1,) * 8 + (4,) * 4

    def call(n=16, L=200, nl=12, dil=dil8, lead=8, first=0, max_item=2, ptrs=(one,) * 11, entry="svdd_backbone_incr2_f32"):
        d = None if dil is None else (ctypes.c_int * max(1, len(dil)))(*dil)
        x, table0, tiles, vec, w2, out, planes, x_prev, items, order, count = ptrs
        args = [x, table0, tiles, vec, w2, out, n, L, nl, d, lead, planes, x_prev, items, None, first, max_item]
        if entry == "svdd_backbone_incr2_f32":
            args += [order, count]
        return getattr(L_, entry)(*args, None)

    for k in range(11):                                      # each pointer NULL in turn: order is 9, order_count 10
        assert call(ptrs=tuple(None if i == k else one for i in range(11))) == _lib.E_ARG, k
    for mi in (0, 3, 5, 8, -1, -2):
        assert call(max_item=mi) == _lib.E_ARG, mi
    shared = (dict(L=104), dict(L=209), dict(L=0), dict(n=0), dict(n=-3), dict(nl=0), dict(nl=33, dil=(1,) * 33), dict(lead=1), dict(lead=0),
              dict(lead=13), dict(lead=9), dict(dil=(1,) * 7 + (2,) + (4,) * 4), dict(dil=None), dict(dil=(1,) * 8 + (0,) * 4))
    for kw in shared:                                        # what the old entry refuses, the new one refuses
        assert call(entry="svdd_backbone_incr_f32", **kw) == _lib.E_ARG, kw
        assert call(**kw) == _lib.E_ARG, kw
        assert call(first=1, **kw) == _lib.E_ARG, kw
    assert call(n=65537) == _lib.E_ARG                       # a row index must fit the upper half of a list entry
    assert call(entry="svdd_backbone_incr_f32", max_item=1) == _lib.E_ARG     # the old entry keeps refusing 1-tile items


def test_incr_residency_setter_range():
    L_ = _lib.lib()
    for bad in (-1, 9, 100):
        assert L_.svdd_backbone_incr_set_residency(bad) == _lib.E_ARG
    for ok in (1, 2, 3, 4, 8, 0):
        assert L_.svdd_backbone_incr_set_residency(ok) == _lib.OK
