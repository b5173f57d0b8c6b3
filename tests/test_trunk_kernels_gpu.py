"""-m gpu: every entry point of the Enformer-shaped value trunk (csrc/svdd_trunk.hip) on its own, against a float64 restatement
of the operation, through the C ABI with explicit guard and tail rows.

The element-wise kernels (act_split, layernorm_split, attn_pool, attn_small, stem_unfold) compute in fp32 and differ by plane
format only in the store: the fp32-plane instantiation (SVDD_OPT_TRUNK_PLANES_F32) is compared with float64, and the bf16
instantiations must then store exactly hi = bf16(v), lo = bf16(v - hi) of that fp32 result v (one-pass bf16: hi only). Every
kernel that takes a live count must leave the rows beyond it untouched (sentinel-filled buffers), and its live rows must be
the bits of the same call without a count. Bars: 2 - 4x the worst case measured on the MI355X, quoted beside each.

The three entries behind "first levels shared between a candidate and its parent" (svdd_trunk_windows, _stem_unfold_win,
_attn_pool_win) are held to the integer restatement tests/trunk_ref.py windows_ref (proved against the dependency cone and the
float64 tower in tests/test_trunk_ref_cpu.py) and, bit for bit, to the whole-sequence kernels above, on one case table
(trunk_ref.WINDOW_CASES). What a wrong index does to them: profiles/trunk_windows_teeth.txt."""
import contextlib

import numpy as np
import pytest
import torch

from svdd_amd import _lib
from svdd_amd.enformer_value import _positional_features
from svdd_amd.fused_trunk import GUARD, TAIL, pack_gemm_weight, pack_gemm_weight_f32
from tests import trunk_ref as R
from tests.trunk_ref import act as act_ref, attn_small_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = ("f32", "bf16x3", "bf16")
SENT16, SENT32 = 0x7FA5, 0x7FA5A5A5          # NaN bit patterns no kernel writes


@contextlib.contextmanager
def _planes(mode):
    """Plane format for the span of a block; restored even if an assertion inside fails (svdd_set_option is process-wide)."""
    prev = _lib.set_option(_lib.OPT_TRUNK_PLANES_F32, 1 if mode == "f32" else 0)
    try:
        yield
    finally:
        _lib.set_option(_lib.OPT_TRUNK_PLANES_F32, prev)


@contextlib.contextmanager
def _gemm_option(v):
    prev = _lib.set_option(_lib.OPT_TRUNK_GEMM_VERSION, v)
    try:
        yield
    finally:
        _lib.set_option(_lib.OPT_TRUNK_GEMM_VERSION, prev)


class _Buf:
    """rows x C elements behind GUARD and in front of TAIL rows of C, all sentinel-filled; .ptr is row 0."""

    def __init__(self, rows, C, dtype):
        self.rows, self.C, self.dtype = rows, C, dtype
        n = (GUARD + rows + TAIL) * C
        if dtype == torch.bfloat16:
            self.raw = torch.full((n,), SENT16, dtype=torch.int16, device=DEV)
        else:
            self.raw = torch.full((n,), SENT32, dtype=torch.int32, device=DEV)
        self.t = self.raw.view(dtype)

    @property
    def ptr(self):
        return self.t[GUARD * self.C:].data_ptr()

    def body(self):
        return self.t[GUARD * self.C:(GUARD + self.rows) * self.C].view(self.rows, self.C)

    def bits(self):
        return self.raw[GUARD * self.C:(GUARD + self.rows) * self.C].view(self.rows, self.C)

    def untouched(self):
        """Bool mask [rows, C] of elements still holding the sentinel; asserts the guard and tail rows are intact."""
        s = SENT16 if self.dtype == torch.bfloat16 else SENT32
        assert bool((self.raw[:GUARD * self.C] == s).all()) and bool((self.raw[(GUARD + self.rows) * self.C:] == s).all())
        return self.bits() == s


def _planes_out(mode, rows, C):
    """Output planes of one mode: (hi, lo); lo is allocated in one-pass mode too, but not handed to the kernel."""
    if mode == "f32":
        return _Buf(rows, C, torch.float32), None
    return _Buf(rows, C, torch.bfloat16), _Buf(rows, C, torch.bfloat16)


def _run_modes(launch, rows, C, count=None):
    """launch(hi_ptr, lo_ptr, count_ptr) in the three plane modes -> {mode: (hi _Buf, lo _Buf or None)}."""
    res = {}
    ct = None if count is None else torch.tensor([count], dtype=torch.int32, device=DEV)     # (kept alive across the launches)
    cp = None if ct is None else ct.data_ptr()
    for mode in MODES:
        hi, lo = _planes_out(mode, rows, C)
        with _planes(mode):
            _lib.check(launch(hi.ptr, lo.ptr if mode == "bf16x3" else None, cp), "launch")
            torch.cuda.synchronize()
        res[mode] = (hi, lo)
    return res


def _check_split(res, live_rows=None):
    """The bf16 instantiations store the exact split of the fp32 instantiation's values (pad rows included); one-pass bf16
    leaves its lo plane untouched. live_rows: rows beyond it must be untouched in every mode."""
    v = res["f32"][0].body()
    rows = v.shape[0]
    live = rows if live_rows is None else live_rows
    hi_want = v.to(torch.bfloat16)
    lo_want = (v - hi_want.float()).to(torch.bfloat16)
    hi3, lo3 = res["bf16x3"]
    hi1, lo1 = res["bf16"]
    assert torch.equal(hi3.bits()[:live], hi_want[:live].view(torch.int16))
    assert torch.equal(lo3.bits()[:live], lo_want[:live].view(torch.int16))
    assert torch.equal(hi1.bits()[:live], hi_want[:live].view(torch.int16))
    assert bool(lo1.untouched().all())
    for buf in (res["f32"][0], hi3, lo3, hi1):
        u = buf.untouched()
        assert bool(u[live:].all())
        assert not bool(u[:live].any())


def _report(name, err, bar):
    print(f"ERR {name} {err:.3e} bar {bar:.1e}")
    assert err <= bar, (name, err, bar)


def _count_check(launch, full, rows_per_count, n, C, live=None):
    """With count = live < n: the first live * rows_per_count rows are the bits of the call without a count (`full`, f32 mode),
    the rest untouched."""
    live = live if live is not None else max(1, n // 3)
    res = _run_modes(launch, n * rows_per_count, C, count=live)
    lr = live * rows_per_count
    assert torch.equal(res["f32"][0].bits()[:lr], full.bits()[:lr])
    _check_split(res, lr)


# ------------------------------------------------------------------------------------------------------------ stem unfold
@pytest.mark.parametrize("L", [1, 7, 8, 14, 15, 16, 200, 256])
def test_stem_unfold_exact(L):
    """Row (b, l) = channel 4 t + tok[l + t - 7] for t < 15 (MASK = 4: nothing), taps off either end empty, channels 60 - 63 and
    the two pad rows zero: exact in every plane format, and the live count honoured."""
    n = 5
    g = torch.Generator(device="cpu").manual_seed(L)
    tok = torch.randint(0, 5, (n, L), generator=g, dtype=torch.uint8)
    tok[1] = 4
    tok[2, ::3] = 4
    ref = np.zeros((n, L + 2, 64), dtype=np.float32)
    tk = tok.numpy()
    for b in range(n):
        for l in range(L):
            for t in range(15):
                p = l + t - 7
                if 0 <= p < L and tk[b, p] < 4:
                    ref[b, l, 4 * t + tk[b, p]] = 1.0
    ref = torch.from_numpy(ref.reshape(n * (L + 2), 64)).to(DEV)
    tg = tok.to(DEV)
    lib = _lib.lib()
    rows = n * (L + 2)

    def launch(hi, lo, cp):
        return lib.svdd_trunk_stem_unfold(tg.data_ptr(), n, L, hi, cp, None)
    for live in (None, 2):
        for mode in ("f32", "bf16"):
            out = _Buf(rows, 64, torch.float32 if mode == "f32" else torch.bfloat16)
            ct = None if live is None else torch.tensor([live], dtype=torch.int32, device=DEV)
            with _planes(mode):
                _lib.check(launch(out.ptr, None, None if ct is None else ct.data_ptr()), "svdd_trunk_stem_unfold")
                torch.cuda.synchronize()
            lr = rows if live is None else live * (L + 2)
            u = out.untouched()
            assert bool(u[lr:].all()) and not bool(u[:lr].any())
            got = out.body()[:lr].float()
            assert torch.equal(got, ref[:lr])
            v = got.view(-1, L + 2, 64)
            assert bool((v[:, L:] == 0).all()) and bool((v[:, :, 60:] == 0).all())
    assert float(ref.sum()) > 0


# ------------------------------------------------------------------------------------------------------------ act_split
@pytest.mark.parametrize("rps,pad", [(7, 2), (5, 0), (4, 2), (1, 0), (6, 3)])
@pytest.mark.parametrize("bn", [False, True])
@pytest.mark.parametrize("act", [0, 1, 2])
def test_act_split_against_fp64(act, bn, rps, pad):
    """act(scale x + shift) -> planes, last `pad` rows of every sequence zero; GELU = x sigmoid(1.702 x)."""
    n, C = 9, 136
    rows = n * rps
    g = torch.Generator(device="cpu").manual_seed(100 * act + 10 * rps + pad + bn)
    x = (torch.randn(rows, C, generator=g) * 3).to(DEV)
    sc = (1.0 + 0.5 * torch.randn(C, generator=g)).to(DEV) if bn else None
    sh = (0.5 * torch.randn(C, generator=g)).to(DEV) if bn else None
    lib = _lib.lib()

    def launch(hi, lo, cp):
        return lib.svdd_trunk_act_split(x.data_ptr(), None if sc is None else sc.data_ptr(), None if sh is None else sh.data_ptr(),
                                        act, rows, C, rps, pad, hi, lo, cp, None)
    res = _run_modes(launch, rows, C)
    _check_split(res)
    t = x.double() * sc.double() + sh.double() if bn else x.double()
    ref = act_ref(t, act)
    padr = (torch.arange(rows, device=DEV) % rps) >= rps - pad
    ref[padr] = 0.0
    v = res["f32"][0].body()
    assert bool((v[padr] == 0).all())
    err = float((v.double() - ref).abs().max()) / float(ref.abs().max())
    _report(f"act_split[{act},{bn},{rps},{pad}]", err, 2.5e-7)        # measured: 8.2e-8
    _count_check(launch, res["f32"][0], rps, n, C)


# ------------------------------------------------------------------------------------------------------------ layernorm
@pytest.mark.parametrize("C", [8, 24, 504, 512, 520, 1536, 4096])
def test_layernorm_split_against_fp64(C):
    """LayerNorm over partial and full lane groups; rows with mean ~1e3 and spread ~1e-2 (a one-pass variance would cancel
    to nothing there), constant rows (variance 0: only eps is left), the module's eps."""
    n, rps = 6, 3
    rows = n * rps
    eps = torch.nn.LayerNorm(8).eps
    g = torch.Generator(device="cpu").manual_seed(C)
    x = torch.randn(rows, C, generator=g) * 2 + 0.3
    big = [1, 4, 9, 13]
    for r in big:
        x[r] = 1000.0 + 0.01 * torch.randn(C, generator=g)
    x[5], x[10] = 0.375, -3.0
    x = x.to(DEV)
    gamma = (1.0 + 0.3 * torch.randn(C, generator=g)).to(DEV)
    beta = (0.2 * torch.randn(C, generator=g)).to(DEV)
    lib = _lib.lib()

    def launch(hi, lo, cp):
        return lib.svdd_trunk_layernorm_split(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), eps, rows, C, hi, lo, cp, rps, None)
    res = _run_modes(launch, rows, C)
    _check_split(res)
    xd = x.double()
    mu = xd.mean(dim=1, keepdim=True)
    var = ((xd - mu) ** 2).mean(dim=1, keepdim=True)
    ref = (xd - mu) / torch.sqrt(var + eps) * gamma.double() + beta.double()
    v = res["f32"][0].body().double()
    assert torch.equal(v[5], beta.double()) and torch.equal(v[10], beta.double())     # variance 0: exactly beta
    small = [r for r in range(rows) if r not in big]
    err = float((v[small] - ref[small]).abs().max()) / float(ref[small].abs().max())
    _report(f"layernorm[{C}]", err, 5e-7)                            # measured: 1.7e-7
    errb = float((v[big] - ref[big]).abs().max()) / float(ref[big].abs().max())
    _report(f"layernorm_bigmean[{C}]", errb, 1e-2)                  # measured: 3.9e-3 (the fp32 mean of 1e3 + 1e-2 noise)
    _count_check(launch, res["f32"][0], rps, n, C)


# ------------------------------------------------------------------------------------------------------------ attn_pool
POOL_OUTS = [(True, False, 0), (False, False, 0), (True, True, 2), (False, True, 1), (False, False, 2), (True, None, 0)]


@pytest.mark.parametrize("C", [4, 64, 768])
@pytest.mark.parametrize("L", [1, 2, 3, 37, 200, 201])
def test_attn_pool_against_fp64(L, C):
    """Pair softmax pooling; odd L pools its last row alone. Sequences with equal logits, logit gaps of +-80 and +-1e4, and
    random ones; the input pad rows hold NaN (never read). fp32 rows (pad rows untouched) and / or planes with post
    scale / shift and post_act 0 / 1 / 2 (pad rows zero)."""
    n = 5
    Lp, Lo = L + 2, (L + 1) // 2
    g = torch.Generator(device="cpu").manual_seed(L * 1000 + C)
    x = torch.randn(n, Lp, C, generator=g) * 2
    lg = torch.randn(n, Lp, C, generator=g) * 3
    lg[0] = 0.7                                                        # equal logits: the mean of the pair
    sgn = torch.where(torch.rand(L, C, generator=g) < 0.5, -1.0, 1.0)
    lg[1, :L] = 0.5 * 80.0 * sgn * torch.where(torch.arange(L)[:, None] % 2 == 0, 1.0, -1.0)
    lg[2, :L] = 0.5 * 1e4 * sgn * torch.where(torch.arange(L)[:, None] % 2 == 0, 1.0, -1.0)
    x[:, L:], lg[:, L:] = float("nan"), float("nan")
    x, lg = x.to(DEV), lg.to(DEV)
    ps, pb = (1.0 + 0.3 * torch.randn(C, generator=g)).to(DEV), (0.2 * torch.randn(C, generator=g)).to(DEV)
    # fp64 reference
    xd, ld = x.double()[:, :L], lg.double()[:, :L]
    ref = torch.zeros(n, Lo + 2, C, dtype=torch.float64, device=DEV)
    ev = min(L // 2, Lo)
    if ev:
        w = torch.softmax(ld[:, :2 * ev].reshape(n, ev, 2, C), dim=2)
        ref[:, :ev] = (xd[:, :2 * ev].reshape(n, ev, 2, C) * w).sum(dim=2)
    if L % 2:
        ref[:, Lo - 1] = xd[:, L - 1]
    lib = _lib.lib()
    orows = n * (Lo + 2)
    prow = (torch.arange(orows, device=DEV) % (Lo + 2)) >= Lo
    full_f32 = None
    for want_out, post, pact in POOL_OUTS:
        outs = {}

        def launch(hi, lo, cp, out_ptr=None, post=post, pact=pact):
            planes = post is not None
            return lib.svdd_trunk_attn_pool(x.data_ptr(), lg.data_ptr(), n, L, C, out_ptr, cp, hi if planes else None,
                                            lo if planes else None, ps.data_ptr() if post else None, pb.data_ptr() if post else None,
                                            pact, None)
        res = {}
        for mode in MODES:
            hi, lo = _planes_out(mode, orows, C)
            out = _Buf(orows, C, torch.float32) if want_out else None
            with _planes(mode):
                _lib.check(launch(hi.ptr, lo.ptr if mode == "bf16x3" else None, None, out.ptr if out else None), "svdd_trunk_attn_pool")
                torch.cuda.synchronize()
            res[mode] = (hi, lo)
            outs[mode] = out
        if want_out:
            o = outs["f32"].body().double().view(n, Lo + 2, C)
            u = outs["f32"].untouched().view(n, Lo + 2, C)
            assert bool(u[:, Lo:].all()) and not bool(u[:, :Lo].any())       # fp32 pad rows untouched
            for m in MODES[1:]:
                assert torch.equal(outs[m].bits(), outs["f32"].bits())
            err = float((o[:, :Lo] - ref[:, :Lo]).abs().max()) / float(ref.abs().max())
            _report(f"attn_pool_out[{L},{C}]", err, 3e-7)                   # measured: 1.1e-7
            assert torch.isfinite(o[:, :Lo]).all()
        if post is not None:
            _check_split(res)
            t = ref * ps.double() + pb.double() if post else ref
            pref = act_ref(t, pact).reshape(orows, C)
            pref[prow] = 0.0
            v = res["f32"][0].body().double()
            assert bool((v[prow] == 0).all())
            err = float((v - pref).abs().max()) / float(pref.abs().max())
            _report(f"attn_pool_planes[{L},{C},{post},{pact}]", err, 5e-7)    # measured: 1.6e-7
            if full_f32 is None:
                full_f32 = (launch, res["f32"][0])
    launch, full = full_f32
    _count_check(launch, full, Lo + 2, n, C, live=2)


# ------------------------------------------------------------------------------------------------------------ attn_small
ATTN_SHAPES = [(1, 1, 1), (3, 16, 64), (8, 64, 192), (3, 65, 200), (1, 130, 64), (8, 16, 1)]


@pytest.mark.parametrize("heads,dk,dv", ATTN_SHAPES)
@pytest.mark.parametrize("T", [1, 2, 3, 4])
def test_attn_small_against_fp64(T, heads, dk, dv):
    """Relative-position attention on T <= 4 tokens: every template instantiation, dk / dv below, at and above a wave's 64
    lanes, n * heads not a multiple of 4, one sequence with large logits; the rel_k of the module's own positional features."""
    n, nfeat = 7, 12
    g = torch.Generator(device="cpu").manual_seed(T * 100 + heads * 10 + dk + dv)
    qkv = torch.randn(n * T, heads * (2 * dk + dv), generator=g)
    qkv[T:2 * T, :2 * heads * dk] *= 12.0                                 # sequence 1: logits of tens to hundreds
    rel_w = torch.randn(heads * dk, nfeat, generator=g, dtype=torch.float64) * nfeat ** -0.5
    rel_k = (_positional_features(T, nfeat, "cpu", torch.float64) @ rel_w.t()).view(2 * T - 1, heads, dk).transpose(0, 1)
    rel_k = rel_k.float().contiguous()
    cb, pb = torch.randn(heads, dk, generator=g), torch.randn(heads, dk, generator=g)
    qkv, rel_k, cb, pb = qkv.to(DEV), rel_k.to(DEV), cb.to(DEV), pb.to(DEV)
    ref = attn_small_ref(qkv.double(), rel_k.double(), cb.double(), pb.double(), n, T, heads, dk, dv)
    lib = _lib.lib()
    C = heads * dv

    def launch(hi, lo, cp):
        return lib.svdd_trunk_attn_small(qkv.data_ptr(), rel_k.data_ptr(), cb.data_ptr(), pb.data_ptr(), n, T, heads, dk, dv, hi, lo, cp, None)
    res = _run_modes(launch, n * T, C)
    _check_split(res)
    v = res["f32"][0].body().double()
    err = float((v - ref).abs().max()) / float(ref.abs().max())
    _report(f"attn_small[{T},{heads},{dk},{dv}]", err, 1e-5)      # measured: 3.3e-6 (T = 4), 0 at T = 1
    _count_check(launch, res["f32"][0], T, n, C)


# ------------------------------------------------------------------------------------------------------------ GEMM
# M, N, Cin, taps, rows_per_seq, live, act, bias, resid, lda, ldo, post scale / shift, post_act, pad
GEMM_CASES = [
    (1000, 768, 96, 1, 8, None, 2, True, True, 96, 768, True, 2, 2),
    (2100, 896, 64, 5, 14, None, 0, True, False, 72, 900, True, 1, 2),
    (777, 256, 160, 5, 7, 40, 1, False, True, 168, 260, False, 2, 0),
    (5000, 1152, 64, 1, 10, 333, 2, False, False, 64, 1152, True, 0, 3),
    (100, 128, 32, 1, 5, None, 0, True, True, 40, 132, False, 0, 0),
    (513, 384, 32, 3, 9, 0, 1, True, True, 32, 384, True, 2, 2),
    # the transformer tower's shapes: one sequence = T tokens, T in {1, 3, 5}
    (37, 384, 256, 1, 1, 20, 2, True, False, 256, 388, True, 2, 0),
    (111, 512, 128, 1, 3, 17, 1, True, True, 136, 512, False, 1, 0),
    (200, 256, 96, 1, 5, None, 0, False, True, 96, 256, True, 2, 1),
]


@pytest.mark.parametrize("case", GEMM_CASES, ids=[f"M{c[0]}N{c[1]}K{c[2]}T{c[3]}" for c in GEMM_CASES])
def test_gemm_against_fp64(case):
    """svdd_trunk_gemm: fp32 planes (both LDS-DMA tile heights, same bits) against fp64, and the fused second output
    post_act(post_scale y + post_shift) with its pad rows against fp64 in all three plane modes. Strides wider than the
    minimum (the extra A columns hold NaN: never read; the extra out columns stay untouched), act 0 / 1 / 2, bias and / or
    residual absent, the live count."""
    M, N, Cin, T, rps, live, act, has_b, has_r, lda, ldo, has_post, pact, pad = case
    g = torch.Generator(device="cpu").manual_seed(M + N + T)
    a = torch.randn(M, Cin, generator=g)
    w = torch.randn(N, Cin, T, generator=g) * (Cin * T) ** -0.5
    bias = torch.randn(N, generator=g).to(DEV) if has_b else None
    resid = torch.randn(M, ldo, generator=g).to(DEV) if has_r else None
    ps = (1.0 + 0.2 * torch.randn(N, generator=g)).to(DEV) if has_post else None
    pb = (0.1 * torch.randn(N, generator=g)).to(DEV) if has_post else None
    cnt = None if live is None else torch.tensor([live], dtype=torch.int32, device=DEV)
    m_live = M if live is None else min(M, live * rps)
    lib = _lib.lib()
    hw = w.to(torch.bfloat16)
    parts_w = {"f32": w, "bf16x3": (hw, (w - hw.float()).to(torch.bfloat16)), "bf16": (hw,)}
    ha = a.to(torch.bfloat16)
    parts_a = {"f32": (a,), "bf16x3": (ha, (a - ha.float()).to(torch.bfloat16)), "bf16": (ha,)}

    def a_planes(mode):
        out = []
        for p in parts_a[mode]:
            buf = torch.zeros(GUARD + M + TAIL, lda, dtype=p.dtype, device=DEV)
            buf[:, Cin:] = float("nan")
            buf[GUARD:GUARD + M, :Cin] = p.to(DEV)
            out.append(buf)
        return out

    def reference(mode):
        ae = sum(p.double() for p in parts_a[mode])
        we = w.double() if mode == "f32" else sum(p.double() for p in parts_w[mode])
        ap = torch.zeros(M + T, Cin, dtype=torch.float64)
        ap[T // 2:T // 2 + M] = ae
        y = sum(ap[t:t + M] @ we[:, :, t].t() for t in range(T)).to(DEV)
        if has_b:
            y = y + bias.double()
        y = act_ref(y, act)
        if has_r:
            y = y + resid[:, :N].double()
        z = act_ref(y * ps.double() + pb.double() if has_post else y, pact)
        z[(torch.arange(M, device=DEV) % rps) >= rps - pad] = 0.0
        return y, z

    def run(mode, count, height=None):
        wp = (pack_gemm_weight_f32(w) if mode == "f32" else pack_gemm_weight(w, len(parts_w[mode]))).to(DEV)
        pl = a_planes(mode)
        out = _Buf(M, ldo, torch.float32)
        pdt = torch.float32 if mode == "f32" else torch.bfloat16
        o_hi = _Buf(M, N, pdt)
        o_lo = _Buf(M, N, pdt) if mode == "bf16x3" else None
        with _planes(mode), _gemm_option(height or 40):
            rc = lib.svdd_trunk_gemm(pl[0][GUARD:].data_ptr(), pl[1][GUARD:].data_ptr() if len(pl) > 1 else None, wp.data_ptr(),
                                     None if bias is None else bias.data_ptr(), None if resid is None else resid.data_ptr(), out.ptr,
                                     M, N, Cin, T, lda, ldo, act, None if count is None else count.data_ptr(), rps,
                                     o_hi.ptr, None if o_lo is None else o_lo.ptr, None if ps is None else ps.data_ptr(),
                                     None if pb is None else pb.data_ptr(), pact, pad, None)
            _lib.check(rc, "svdd_trunk_gemm")
            torch.cuda.synchronize()
        return out, o_hi, o_lo

    for mode in MODES:
        y, z = reference(mode)
        full = run(mode, None, 41 if mode == "f32" else None)
        if mode == "f32":
            short = run(mode, None, 42)                                     # 192-row tiles: the same bits
            for b1, b2 in zip(full[:2], short[:2]):
                assert torch.equal(b1.bits(), b2.bits())
        out, o_hi, o_lo = full
        u = out.untouched()
        assert bool(u[:, N:].all()) and not bool(u[:, :N].any())           # ldo > N: the extra columns are never written
        assert not bool(o_hi.untouched().any())
        ov = out.body()[:, :N].double()
        scale = max(1.0, float(y.abs().max()))
        err = float((ov - y).abs().max()) / scale
        zv = o_hi.body().double() + (o_lo.body().double() if o_lo is not None else 0.0)
        padr = (torch.arange(M, device=DEV) % rps) >= rps - pad
        assert bool((o_hi.body()[padr] == 0).all())
        errz = float((zv - z).abs().max()) / max(1.0, float(z.abs().max()))
        # (out, planes); measured: f32 7.9e-7 / 8.4e-7, bf16x3 4.0e-6 / 6.6e-6, bf16 3.2e-7 / 3.4e-3 (the planes' bf16 rounding)
        bars = {"f32": (2.5e-6, 2.5e-6), "bf16x3": (1.2e-5, 2e-5), "bf16": (1e-6, 1e-2)}[mode]
        _report(f"gemm_out[{mode},{M},{N},{Cin},{T}]", err, bars[0])
        _report(f"gemm_planes[{mode},{M},{N},{Cin},{T}]", errz, bars[1])
        if cnt is not None:
            part = run(mode, cnt)
            for bf, bp in zip(full, part):
                if bf is None:
                    continue
                up = bp.untouched()
                assert bool(up[m_live:].all())
                assert torch.equal(bp.bits()[:m_live], bf.bits()[:m_live])


# ------------------------------------------------------------------------------------------------------------ shared-level windows
def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32).reshape(-1)).to(DEV)


def _count(count):
    ct = None if count is None else torch.tensor([count], dtype=torch.int32, device=DEV)
    return ct, None if ct is None else ct.data_ptr()


@pytest.mark.parametrize("case", R.WINDOW_CASES, ids=R.window_case_id)
def test_trunk_windows_exact(case):
    """svdd_trunk_windows: w0, wlen, seg equal trunk_ref.windows_ref in all depth x n x slots entries (unused slots and candidates
    beyond the live count: zeros), every entry written, nothing around the tables written, a second launch the same bits.
    Teeth (profiles/trunk_windows_teeth.txt): the next level's window end one pair short -> 37 cases red, a level-0 window one row
    short of an odd position's reach -> 48; both also moved the end-to-end scores of tests/test_trunk_gpu.py. Deeper windows joined
    within 2 rows instead of 4 -> 17 red here and nothing red there (the result stays exact: only this test holds the rule)."""
    L, depth, slots, halo, count, perm = case
    cand, parent, pidx, div, edits = R.window_case_tokens(case)
    n = len(cand)
    cg, pg, ig = torch.from_numpy(cand).to(DEV), torch.from_numpy(parent).to(DEV), torch.from_numpy(pidx).to(DEV)
    ct, cp = _count(count)
    want = R.windows_ref(cand, parent, pidx, div, L, halo, depth, slots, count)
    lib = _lib.lib()
    runs = []
    for rep in range(2):
        tabs = [_Buf(depth * n, slots, torch.float32) for _ in range(3)]                     # (int32 tables behind the fp32 sentinel)
        _lib.check(lib.svdd_trunk_windows(cg.data_ptr(), pg.data_ptr(), ig.data_ptr(), div, n, L, halo, depth, slots, cp,
                                          tabs[0].ptr, tabs[1].ptr, tabs[2].ptr, None), "svdd_trunk_windows")
        torch.cuda.synchronize()
        for buf in tabs:
            assert not bool(buf.untouched().any())                                           # (asserts guard and tail rows too)
        runs.append([buf.bits().cpu().numpy().reshape(depth, n, slots) for buf in tabs])
    for name, got, again, ref in zip(("w0", "wlen", "seg"), runs[0], runs[1], want):
        assert np.array_equal(got, ref), (name, np.argwhere(got != ref)[:4].tolist())
        assert np.array_equal(got, again), name
        if count is not None:
            assert not got[:, count:].any()
    assert want[1].any() == (count != 0)


STEM_WIN_CASES = sorted({(L, 1, slots, halo, count, perm) for L, _, slots, halo, count, perm in R.WINDOW_CASES},
                        key=lambda c: (c[0], c[2], c[3], -1 if c[4] is None else c[4], c[5]))


@pytest.mark.parametrize("case", STEM_WIN_CASES, ids=R.window_case_id)
def test_stem_unfold_win_exact(case):
    """svdd_trunk_stem_unfold_win on the tables of windows_ref (off = exclusive prefix sum of the level-0 seg): compact row
    off[c slots] + r is, bit for bit, the row svdd_trunk_stem_unfold writes for the r-th window row of candidate c, and the
    brute-force one-hot unfold of test_stem_unfold_exact; the buffer holds the window rows and the tail, not n L rows; with a
    live count (the tables still those of all candidates) the rows of the candidates beyond it stay untouched.
    Teeth: the slot walk without `r -= wl` -> 16 of the 29 cases red (so is the end-to-end test)."""
    L, _, slots, halo, count, perm = case
    cand, parent, pidx, div, edits = R.window_case_tokens(case)
    n = len(cand)
    w0, wlen, seg = (t[0] for t in R.windows_ref(cand, parent, pidx, div, L, halo, 1, slots))
    off, total = R.compact_offsets(seg)
    live = n if count is None else count
    live_total = total if live >= n else int(off[live * slots])
    ref = np.zeros((n, L, 64), dtype=np.float32)
    for b in range(n):
        for l in range(L):
            for t in range(15):
                p = l + t - 7
                if 0 <= p < L and cand[b, p] < 4:
                    ref[b, l, 4 * t + cand[b, p]] = 1.0
    src, dst, pos = [], [], []
    for c in range(live):
        r = 0
        for j in range(slots):
            for q in range(int(w0[c, j]), int(w0[c, j] + wlen[c, j])):
                src.append(c * (L + 2) + q)
                dst.append(int(off[c * slots]) + r)
                pos.append((c, q))
                r += 1
    assert dst == list(range(live_total)) and total <= n * L
    src_t = torch.tensor(src, dtype=torch.long, device=DEV)
    want = torch.from_numpy(np.stack([ref[c, q] for c, q in pos]) if pos else np.zeros((0, 64), dtype=np.float32)).to(DEV)
    cg = torch.from_numpy(cand).to(DEV)
    w0g, wlg, ofg = _i32(w0), _i32(wlen), _i32(off)
    ct, cp = _count(count)
    lib = _lib.lib()
    for mode in ("f32", "bf16"):
        dt = torch.float32 if mode == "f32" else torch.bfloat16
        dense, out = _Buf(n * (L + 2), 64, dt), _Buf(total, 64, dt)
        with _planes(mode):
            _lib.check(lib.svdd_trunk_stem_unfold(cg.data_ptr(), n, L, dense.ptr, None, None), "svdd_trunk_stem_unfold")
            _lib.check(lib.svdd_trunk_stem_unfold_win(cg.data_ptr(), n, L, slots, w0g.data_ptr(), wlg.data_ptr(), ofg.data_ptr(), out.ptr,
                                                      cp, None), "svdd_trunk_stem_unfold_win")
            torch.cuda.synchronize()
        u = out.untouched()
        assert bool(u[live_total:].all()) and not bool(u[:live_total].any())
        assert torch.equal(out.bits()[:live_total], dense.bits()[src_t])
        assert torch.equal(out.body()[:live_total].float(), want)
    assert count == 0 or float(want.sum()) > 0


def _pool64(x, lg, L):
    """AttentionPool(2) of x, logits [n, L, C] in float64 -> [n, ceil(L / 2), C]; an odd L pools its last row alone."""
    n, _, C = x.shape
    Lo, ev = (L + 1) // 2, L // 2
    out = torch.zeros(n, Lo, C, dtype=torch.float64, device=x.device)
    if ev:
        w = torch.softmax(lg[:, :2 * ev].reshape(n, ev, 2, C), dim=2)
        out[:, :ev] = (x[:, :2 * ev].reshape(n, ev, 2, C) * w).sum(dim=2)
    if L % 2:
        out[:, Lo - 1] = x[:, L - 1]
    return out


# the pooling cases: every length at its greatest depth with 4 slots, 1 and 2 slots at L = 200 and at the short / odd-level lengths,
# and the table's halo / count / permuted cases — each at every one of its levels
_POOL_BASE = [c for c in R.WINDOW_CASES[:-8] if (c[2] == 4 and c[1] == max(k[1] for k in R.WINDOW_CASES if k[0] == c[0]))
              or c[:3] in ((200, 4, 1), (200, 4, 2), (16, 4, 2), (30, 2, 1))]
POOL_WIN_CASES = [(c, d) for c in _POOL_BASE + R.WINDOW_CASES[-8:] for d in range(c[1])]
POOL_POSTS = [(True, 2), (True, 1), (True, 0), (False, 0)]


@pytest.mark.parametrize("C", [8, 64])
@pytest.mark.parametrize("case,d", POOL_WIN_CASES, ids=[f"{R.window_case_id(c)}-lv{d}" for c, d in POOL_WIN_CASES])
def test_attn_pool_win(case, d, C):
    """svdd_trunk_attn_pool_win at level d of a case (length L >> d; in_halo 0 at level 0, 2 below it), in the three plane modes,
    with post scale / shift and post_act 0 / 1 / 2 and without. The compact input rows are gathered from dense random rows (one
    candidate with equal logits, two with logit gaps of +-80 and +-1e4) with NaN in every context row and between the segments
    (3 free rows behind each): never read. The parents' planes come from svdd_trunk_attn_pool on the parents' dense rows (the rows
    behind the last parent hold the sentinel). Whole-sequence output: where a window covers the pair, the bits of
    svdd_trunk_attn_pool on the candidate's dense rows; elsewhere the bits of row parent_idx[c] / div of the parents' planes; the
    two pad rows zero; candidates beyond the live count untouched. Compact output (v0, vlen, off2 = the next level of the tables):
    row off2[s] + r is position v0[s] - 2 + r of that result, zeros outside [0, Lo), nothing from the total on. The bf16 planes
    are the exact split of the fp32 plane, and the fp32 plane is within 5e-7 of float64 (the bar of test_attn_pool_against_fp64;
    measured: 2.2e-7). An odd length: whole output only, and v0 is refused with every buffer untouched.
    Teeth: in_halo dropped from the source row -> 72 cases red (levels >= 1: level 0 has in_halo 0); the parent's row without
    / div, or the parent of the neighbouring candidate -> 96 of the 112 cases red; the live count ignored -> all 24 cases with a
    count red (the end-to-end test notices the first three, not the last)."""
    L0, depth, slots, halo, count, perm = case
    cand, parent, pidx, div, edits = R.window_case_tokens(case)
    n, B = len(cand), len(parent)
    tabs = R.windows_ref(cand, parent, pidx, div, L0, halo, depth, slots)                    # of all candidates: the count is the kernel's
    L = L0 >> d
    Lo, in_halo = (L + 1) // 2, 2 if d else 0
    w0, wlen, seg = (t[d] for t in tabs)
    off, total = R.compact_offsets(seg, gap=3)
    live = n if count is None else count
    par = pidx // div
    g = torch.Generator(device="cpu").manual_seed(1000 * L0 + 10 * d + C)
    x, lg = torch.randn(n, L, C, generator=g) * 2, torch.randn(n, L, C, generator=g) * 3
    xp, lgp = torch.randn(B, L, C, generator=g) * 2, torch.randn(B, L, C, generator=g) * 3
    sgn = torch.where(torch.rand(L, C, generator=g) < 0.5, -1.0, 1.0) * torch.where(torch.arange(L)[:, None] % 2 == 0, 1.0, -1.0)
    lg[3], lg[10], lg[9] = 0.7, 0.5 * 80.0 * sgn, 0.5 * 1e4 * sgn                           # both ends / every position / spread
    nan = float("nan")
    xc = torch.cat([R.to_compact(x, w0, wlen, off, in_halo, total, nan), torch.full((4, C), nan)]).to(DEV)
    lc = torch.cat([R.to_compact(lg, w0, wlen, off, in_halo, total, nan), torch.full((4, C), nan)]).to(DEV)
    pad = lambda t: torch.cat([t, torch.full((t.shape[0], 2, C), nan)], dim=1).to(DEV)       # noqa: E731
    xd, ld, xpd, lpd = pad(x), pad(lg), pad(xp), pad(lgp)
    ps, pb = (1.0 + 0.3 * torch.randn(C, generator=g)).to(DEV), (0.2 * torch.randn(C, generator=g)).to(DEV)
    # which output rows are pooled from the candidate's window rows, and the compact rows of the next level
    cov = np.zeros((n, Lo + 2), dtype=bool)
    for c in range(n):
        for j in range(slots):
            for q in range(int(w0[c, j]), int(w0[c, j] + wlen[c, j]), 2):
                cov[c, q // 2] = True
    rows = n * (Lo + 2)
    is_pad = torch.from_numpy(np.tile(np.arange(Lo + 2) >= Lo, n)).to(DEV)
    cov_t = torch.from_numpy(cov.reshape(-1)).to(DEV)
    prow = torch.from_numpy((par[:, None].astype(np.int64) * (Lo + 2) + np.arange(Lo + 2)[None, :]).reshape(-1)).to(DEV)
    compact = d + 1 < depth
    if compact:
        assert L % 2 == 0
        v0, vlen, seg2 = (t[d + 1] for t in tabs)
        off2, total2 = R.compact_offsets(seg2)
        live2 = total2 if live >= n else int(off2[live * slots])
        src2 = []
        for c in range(n):
            for j in range(slots):
                if vlen[c, j] > 0:
                    assert len(src2) == off2[c * slots + j]
                    src2 += [c * (Lo + 2) + (i if 0 <= i < Lo else Lo) for i in range(int(v0[c, j]) - 2, int(v0[c, j] + vlen[c, j]) + 2)]
        assert len(src2) == total2
        src2 = torch.tensor(src2, dtype=torch.long, device=DEV)
        v0g, vlg, o2g = _i32(v0), _i32(vlen), _i32(off2)
    w0g, wlg, ofg, ig = _i32(w0), _i32(wlen), _i32(off), _i32(pidx)
    ct, cp = _count(count)
    lib = _lib.lib()
    ref_x, ref_p = _pool64(xd[:, :L].double(), ld[:, :L].double(), L), _pool64(xpd[:, :L].double(), lpd[:, :L].double(), L)
    for post, pact in POOL_POSTS:
        sp, bp = (ps.data_ptr(), pb.data_ptr()) if post else (None, None)
        whole, comp = {}, {}
        for mode in MODES:
            lo_of = lambda bufs: bufs[1].ptr if mode == "bf16x3" else None                  # noqa: E731
            dense, pp = _planes_out(mode, rows, C), _planes_out(mode, rows, C)
            whole[mode] = _planes_out(mode, rows, C)
            with _planes(mode):
                _lib.check(lib.svdd_trunk_attn_pool(xd.data_ptr(), ld.data_ptr(), n, L, C, None, None, dense[0].ptr, lo_of(dense),
                                                    sp, bp, pact, None), "svdd_trunk_attn_pool")
                _lib.check(lib.svdd_trunk_attn_pool(xpd.data_ptr(), lpd.data_ptr(), B, L, C, None, None, pp[0].ptr, lo_of(pp),
                                                    sp, bp, pact, None), "svdd_trunk_attn_pool")
                win = lambda out, nxt: lib.svdd_trunk_attn_pool_win(                        # noqa: E731
                    xc.data_ptr(), lc.data_ptr(), n, L, C, in_halo, slots, w0g.data_ptr(), wlg.data_ptr(), ofg.data_ptr(), ig.data_ptr(), div,
                    pp[0].ptr, lo_of(pp), cp, out[0].ptr, lo_of(out), sp, bp, pact, *nxt, None)
                _lib.check(win(whole[mode], (None, None, None)), "svdd_trunk_attn_pool_win")
                if compact:
                    comp[mode] = _planes_out(mode, total2, C)
                    _lib.check(win(comp[mode], (v0g.data_ptr(), vlg.data_ptr(), o2g.data_ptr())), "svdd_trunk_attn_pool_win")
                elif L % 2:                                                                 # an odd length has no compact output
                    rej = _planes_out(mode, rows, C)
                    assert win(rej, (w0g.data_ptr(), wlg.data_ptr(), ofg.data_ptr())) == _lib.E_ARG
                torch.cuda.synchronize()
            if not compact and L % 2:
                assert all(bool(b.untouched().all()) for b in rej if b is not None)
            planes = range(2 if mode == "bf16x3" else 1)
            lr = live * (Lo + 2)
            for k in planes:
                want = torch.where(cov_t[:, None], dense[k].bits(), pp[k].bits()[prow])
                want[is_pad] = 0
                assert torch.equal(whole[mode][k].bits()[:lr], want[:lr]), (mode, post, pact, k)
                if compact:
                    assert torch.equal(comp[mode][k].bits()[:live2], want[src2[:live2]]), (mode, post, pact, k)
            assert bool(pp[0].untouched()[B * (Lo + 2):].all())
        _check_split(whole, lr)
        if compact:
            _check_split(comp, live2)
        if live:
            t = [r * ps.double() + pb.double() if post else r for r in (ref_x, ref_p)]
            t = [act_ref(r, pact) for r in t]
            covl = torch.from_numpy(cov[:live, :Lo]).to(DEV)
            ref = torch.where(covl[:, :, None], t[0][:live], t[1][torch.from_numpy(par[:live].astype(np.int64)).to(DEV)])
            v = whole["f32"][0].body().view(n, Lo + 2, C)[:live, :Lo].double()
            assert torch.isfinite(v).all()
            err = float((v - ref).abs().max()) / float(ref.abs().max())
            _report(f"attn_pool_win[{R.window_case_id(case)},{d},{C},{post},{pact}]", err, 5e-7)
    assert cov[:live].any() == (live > 0)
