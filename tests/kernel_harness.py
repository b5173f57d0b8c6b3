"""What the per-kernel float64 files (tests/test_grad_kernels_gpu.py, tests/test_net_kernels_gpu.py) share: sentinel-filled output
buffers with guard space on both sides, the launch-twice check and the `ERR <name> <err> bar <bar>` report."""
import ctypes

import torch

from svdd_amd import _lib
from tests import grad_ref as R

DEV = "cuda:0"
GUARD = 1024                                  # elements of guard space before and after every output
SENT32, SENT8 = 0x7FA5A5A5, 0xA5              # a NaN bit pattern / a byte no kernel writes
SENT16 = 0x7FA5                               # a NaN in fp16 and in bf16


class _Buf:
    """numel elements (fp32 / int32, fp16 / bf16, or bytes) between two guards, all sentinel-filled; .ptr is element 0.
    int64 / fp64: numel counts the int32 WORDS, two per value — body() and cpu() view them as the 64-bit type, the written / untouched
    masks stay per word. offset (bytes only): .ptr sits that many bytes into the aligned body — a misaligned view, whose front guard
    is `offset` bytes longer."""

    def __init__(self, numel, dtype=torch.float32, offset=0):
        self.numel, self.dtype = numel, dtype
        assert offset == 0 or dtype == torch.uint8, "a misaligned view is a view of bytes"
        self.lo = GUARD + offset                                              # raw index of element 0
        if dtype == torch.uint8:
            self.raw, self.sent = torch.full((numel + offset + 2 * GUARD,), SENT8, dtype=torch.uint8, device=DEV), SENT8
        elif dtype in (torch.float16, torch.bfloat16):
            self.raw, self.sent = torch.full((numel + 2 * GUARD,), SENT16, dtype=torch.int16, device=DEV), SENT16
        else:
            self.raw, self.sent = torch.full((numel + 2 * GUARD,), SENT32, dtype=torch.int32, device=DEV), SENT32
        assert self.raw.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return self.raw[self.lo:].data_ptr()

    def bits(self):
        return self.raw[self.lo:self.lo + self.numel]

    def body(self):
        return self.bits().view(self.dtype)

    def cpu(self, *shape):
        v = self.body().cpu()
        return v.view(*shape) if shape else v

    def untouched(self):
        """Bool mask of elements still holding the sentinel; asserts that both guards are intact."""
        assert bool((self.raw[:self.lo] == self.sent).all()) and bool((self.raw[self.lo + self.numel:] == self.sent).all()), "guard overwritten"
        return self.bits() == self.sent

    def assert_written(self, what):
        left = int(self.untouched().sum())
        assert left == 0, f"{what}: {left} of {self.numel} elements were never written"

    def assert_written_where(self, what, mask):
        """mask (bool, numel elements or a shape that flattens to it): exactly these elements were written."""
        left, mask = self.untouched(), mask.reshape(-1).to(self.raw.device)
        assert mask.numel() == self.numel
        never, extra = int((left & mask).sum()), int((~left & ~mask).sum())
        assert never == 0, f"{what}: {never} of {int(mask.sum())} elements the contract names were never written"
        assert extra == 0, f"{what}: {extra} elements were written that the contract says are not (first at {int((~left & ~mask).nonzero()[0])})"

    def assert_untouched(self, what):
        assert bool(self.untouched().all()), f"{what}: written although the contract says it is not"


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(t):
    return None if t is None else t.to(DEV).contiguous()


def _p(t):
    return None if t is None else t.data_ptr()


def _twice(name, launch, sizes, written=None):
    """launch(*ptrs) on fresh sentinel buffers of `sizes` (numel, or (numel, dtype)), twice: guards intact, outputs fully written
    (written[i] False: untouched instead; a bool tensor: exactly its True elements written), the two launches bit-identical.
    -> the first launch's buffers."""
    runs = []
    for _ in range(2):
        bufs = [_Buf(*s) if isinstance(s, tuple) else _Buf(s) for s in sizes]
        _lib.check(launch(*[b.ptr for b in bufs]), name)
        torch.cuda.synchronize()
        for i, b in enumerate(bufs):
            w = True if written is None else written[i]
            if isinstance(w, torch.Tensor):
                b.assert_written_where(f"{name} output {i}", w)
            elif w:
                b.assert_written(f"{name} output {i}")
            else:
                b.assert_untouched(f"{name} output {i}")
        runs.append(bufs)
    for a, b in zip(*runs):
        assert torch.equal(a.bits(), b.bits()), f"{name}: two launches differ"
    return runs[0]


def _report(name, got, r64, r32, margin, keep=None, cap=None, pool=None):
    """max |got - ref64| (over `keep`) against grad_ref.bar(margin, ref32, ref64). cap: a flat tolerance the bar may not exceed;
    pool = (ref64, ref32) of a larger sample of the same inputs to take the bar from (an operation with a handful of outputs)."""
    err = (got.double() - r64).abs()
    err = float((err if keep is None else err[keep]).max()) if err.numel() else 0.0
    b = R.bar(margin, r32, r64, keep) if pool is None else R.bar(margin, pool[1], pool[0])
    if cap is not None:
        b = min(b, cap)
    print(f"ERR {name} {err:.3e} bar {b:.1e}")
    assert err <= b, (name, err, b)
