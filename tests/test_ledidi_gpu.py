"""-m gpu: Ledidi design.

  kernel        svdd_ledidi_step through the raw C entry in sentinel-guarded buffers against tests/ledidi_ref.py, bit for bit: what is
                written and what is left alone (a stopped design, a design outside the chunk, a frozen position's y), over two
                consecutive launches (the first one samples only, the second closes an iteration and samples the next)
  whole call    Diffusion.ledidi against the restatement's host loop around the SAME device scores and gradients
  independence  of chunk_rows, check_every, the batch a design sits in; the Philox seed
  contracts     score_best is forward_tokens' bits, frozen positions, the edit count, best_total / best_iter against the trace
  sign          the mean sample score rises over 40 iterations (tests/test_ledidi_cpu.py holds this for the float64 restatement)"""
import numpy as np
import pytest
import torch

from tests import e2e_parity
from tests import ledidi_ref as R
from tests.conftest import load_golden
from tests.kernel_harness import DEV, SENT32, SENT8, _Buf, _st
from tests.test_ledidi_cpu import SIGN_CASE, sign_case_inputs

pytestmark = pytest.mark.gpu
PATIENCE = 3


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _same(got, want, what):
    """Equal bits; a computed NaN equals any computed NaN, never the sentinel."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype != np.float32:
        bad = got != want
    else:
        gb, wb = got.view(np.uint32), want.view(np.uint32)
        bad = (gb != wb) & ~(np.isnan(got) & np.isnan(want) & (gb != SENT32) & (wb != SENT32))
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:5].tolist(), got[bad][:5], want[bad][:5])


_NP = {torch.float32: np.float32, torch.int32: np.int32, torch.uint8: np.uint8}


class _Device:
    """Every buffer of one svdd_ledidi_step call chain in guarded device memory, filled from a restatement State (and xin / the trace
    from sentinel arrays), so that after every launch the device must hold the restatement's bits everywhere."""
    DTYPES = dict(w=torch.float32, m=torch.float32, v=torch.float32, y=torch.float32, tok=torch.uint8, edits=torch.int32,
                  best_total=torch.float32, best_output=torch.float32, best_input=torch.float32, best_iter=torch.int32,
                  x_best=torch.uint8, score_best=torch.float32, wo=torch.int32, stopped=torch.int32, live=torch.int32)

    def __init__(self, st, xin, trace):
        self.bufs = {}
        for name, dt in self.DTYPES.items():
            self.put(name, getattr(st, name))
        self.put("xin", xin, torch.float32)
        for k, name in enumerate(("trace_total", "trace_out", "trace_in")):
            if trace is not None:
                self.put(name, trace[k], torch.float32)

    def put(self, name, arr, dt=None):
        dt = dt or self.DTYPES[name]
        if name not in self.bufs:
            self.bufs[name] = _Buf(arr.size, dt)
        self.bufs[name].body().copy_(torch.from_numpy(np.ascontiguousarray(arr, _NP[dt]).reshape(-1)).to(DEV))

    def ptr(self, name):
        return self.bufs[name].ptr if name in self.bufs else None

    def check(self, st, xin, trace, what):
        for name, b in self.bufs.items():
            b.untouched()                                                   # asserts both guards
            ref = xin if name == "xin" else trace[("trace_total", "trace_out", "trace_in").index(name)] if name.startswith("trace") \
                else getattr(st, name)
            _same(b.cpu().numpy().reshape(ref.shape), np.ascontiguousarray(ref, _NP[b.dtype]), f"{what}: {name}")


def _launch(D, x0d, ed_d, cfgc, rng_struct, B, L, S, d0, nd, n_pad, it, sample, grad=None, sc=None, target=None, err=None):
    import ctypes
    from svdd_amd import _lib
    p = lambda t: None if t is None else t.data_ptr()                       # noqa: E731
    rc = _lib.lib().svdd_ledidi_step(
        x0d.data_ptr(), p(ed_d), p(grad), p(sc), p(target), ctypes.byref(cfgc), None if rng_struct is None else ctypes.byref(rng_struct),
        B, L, S, d0, nd, n_pad, it, int(sample), D.ptr("w"), D.ptr("m"), D.ptr("v"), D.ptr("y"), D.ptr("tok"), D.ptr("xin"), D.ptr("edits"),
        D.ptr("best_total"), D.ptr("best_output"), D.ptr("best_input"), D.ptr("best_iter"), D.ptr("x_best"), D.ptr("score_best"),
        D.ptr("wo"), D.ptr("stopped"), D.ptr("live"), D.ptr("trace_total"), D.ptr("trace_out"), D.ptr("trace_in"), p(err), _st())
    _lib.check(rc, "svdd_ledidi_step")
    torch.cuda.synchronize()


def _sent(shape, dtype=np.float32):
    if dtype == np.uint8:
        return np.full(shape, SENT8, np.uint8)
    return np.full(shape, SENT32, np.uint32).view(np.float32)


# id: (B, L, S, tau, frozen, target, philox, d0, extra designs after the chunk, n_pad, scenario per design, optional outputs, sample last)
#   scenario: improve | keep (not improved) | tie (total == best_total: not improved) | patience (stops exactly) | stopped (at entry) | nan
CASES = {
    "L1": (1, 1, 1, 1.0, "none", False, False, 0, 0, 0, ("improve",), True, True),
    "L5_S3_frozen_some": (3, 5, 3, 1.0, "some", False, False, 0, 0, 1, ("improve", "keep", "patience"), True, True),
    "L64_S10_target": (3, 64, 10, 0.5, "none", True, False, 0, 0, 2, ("tie", "improve", "stopped"), True, True),
    "L65_philox_offset": (3, 65, 3, 1.0, "some", False, True, 2, 1, 7, ("patience", "stopped", "improve"), False, True),
    "L200_S10": (3, 200, 10, 1.0, "none", False, True, 0, 0, 2, ("improve", "nan", "keep"), True, True),
    "L256_S64_last": (1, 256, 64, 0.5, "none", True, False, 0, 0, 0, ("improve",), False, False),
    "L257_all_frozen": (3, 257, 3, 1.0, "all", False, False, 1, 0, 7, ("keep", "improve", "patience"), True, True),
    "L1024_S3_target_nan": (3, 1024, 3, 0.5, "some", True, True, 0, 2, 3, ("nan", "patience", "improve"), True, True),
    "L1024_S64": (1, 1024, 64, 1.0, "none", False, True, 0, 0, 0, ("keep",), True, True),
}


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_equals_the_fp32_restatement_bit_for_bit(name):
    from svdd_amd import _lib, ops
    B, L, S, tau, frozen, with_target, philox, d0, extra, n_pad, scen, optional, sample_last = CASES[name]
    Bt = d0 + B + extra
    rng = np.random.default_rng([B, L, S, d0, n_pad])
    x0 = rng.integers(0, 4, (Bt, L)).astype(np.uint8)
    editable = {"none": None, "some": rng.random(L) < 0.6, "all": np.zeros(L, bool)}[frozen]
    if frozen == "some":
        editable[0] = True
    cfg = R.Cfg(S, tau=tau, l=0.1, lr=1.0, patience=PATIENCE)
    dcfg = ops.LedidiConfig(S, tau=tau, l=0.1, lr=1.0, patience=PATIENCE)
    score0 = rng.standard_normal(Bt).astype(np.float32)
    tgt = rng.standard_normal(Bt).astype(np.float32) if with_target else None
    st = R.State(x0, S, score0, -score0 if tgt is None else (score0 - tgt) * (score0 - tgt))
    st.w[:] = (6.0 * rng.standard_normal(st.w.shape)).astype(np.float32)      # weights that make edits
    st.m[:] = (1e-2 * rng.standard_normal(st.m.shape)).astype(np.float32)
    st.v[:] = (1e-4 * rng.random(st.v.shape)).astype(np.float32)
    st.y, st.tok = _sent(st.y.shape), _sent(st.tok.shape, np.uint8)           # never written: must stay the sentinel
    st.edits[:] = -7
    xin = _sent((B * S + n_pad, L, 4))
    trace = [_sent(Bt) for _ in range(3)] if optional else None
    D = _Device(st, xin, trace)
    x0d = dev(x0)
    ed_d = None if editable is None else dev(editable.astype(np.uint8))
    tgt_d = None if tgt is None else dev(tgt)
    err = torch.zeros(1, dtype=torch.int32, device=DEV) if optional else None
    seed, row_offset, it0 = 0x1234_5678_9ABC_DEF0, ((1 << 32) + 5 if d0 else 0), (70000 if philox else 4)
    u = [None, None] if philox else [rng.random((Bt, S, L, 4)).astype(np.float32) for _ in range(2)]
    ud = [None if a is None else dev(a) for a in u]
    rs = lambda k: (_lib.SvddRng(_lib.RNG_PHILOX, 0, None, seed, row_offset, 0, 0) if philox             # noqa: E731
                    else _lib.SvddRng(_lib.RNG_REPLAY, 0, ud[k].data_ptr(), 0, 0, 0, 0))
    # launch 1: grad NULL, the samples of iteration it0
    _launch(D, x0d, ed_d, dcfg.at(it0), rs(0), Bt, L, S, d0, B, n_pad, it0, True, err=err)
    R.step(st, x0, editable, cfg, xin, d0, B, n_pad, it0, u=u[0], philox=(seed, row_offset))
    D.check(st, xin, trace, "launch 1")
    if frozen != "all" and L > 1:
        assert int(st.edits[d0:d0 + B].sum()) > 0
    # the designs' situations before launch 2
    sc = rng.standard_normal((Bt, S)).astype(np.float32)
    grad = (1e-2 * rng.standard_normal((B * S + n_pad, L, 4))).astype(np.float32)
    grad[B * S:] = np.nan                                                   # pad rows' gradients are never read
    for k, what in enumerate(scen):
        d = d0 + k
        if what == "nan":
            sc[d, S // 2] = np.nan
        total = R.losses(sc[d], st.edits[d], None if tgt is None else tgt[d], cfg)[2]
        st.best_total[d] = total + np.float32(1.0) if what == "improve" else total if what == "tie" else total - np.float32(1.0)
        st.wo[d] = PATIENCE - 1 if what == "patience" else 0
        if what == "stopped":
            st.stopped[d] = 1
            st.live[0] -= 1
    for f in ("best_total", "wo", "stopped", "live"):
        D.put(f, getattr(st, f))
    live_before = int(st.live[0])
    # launch 2: close iteration it0 (AdamW step it0 + 1), sample iteration it0 + 1
    _launch(D, x0d, ed_d, dcfg.at(it0, 16.0), rs(1) if sample_last else None, Bt, L, S, d0, B, n_pad, it0, sample_last, grad=dev(grad),
            sc=dev(sc), target=tgt_d, err=err)
    R.step(st, x0, editable, cfg, xin, d0, B, n_pad, it0, grad=grad, sc=sc, target=tgt, u=u[1], philox=(seed, row_offset),
           sample_next=sample_last, trace=trace, scale=16.0)
    D.check(st, xin, trace, "launch 2")
    assert int(st.live[0]) == live_before - sum(s == "patience" for s in scen)
    for k, what in enumerate(scen):
        d = d0 + k
        assert int(st.stopped[d]) == (what in ("patience", "stopped")), (k, what)
        assert (int(st.best_iter[d]) == it0) == (what == "improve"), (k, what)
    assert err is None or int(err[0]) == 0


def test_kernel_flags_an_editable_start_token_above_3():
    from svdd_amd import _lib, ops
    B, L, S = 2, 9, 2
    rng = np.random.default_rng(3)
    x0 = rng.integers(0, 4, (B, L)).astype(np.uint8)
    x0[1, 4], x0[0, 8] = 5, 4                                                # position 4 editable, position 8 frozen
    editable = np.ones(L, bool)
    editable[8] = False
    cfg, dcfg = R.Cfg(S, patience=PATIENCE), ops.LedidiConfig(S, patience=PATIENCE)
    u = rng.random((B, S, L, 4)).astype(np.float32)
    ud = dev(u)
    for d0, want in ((0, 0), (1, 1)):                                        # design 0 alone holds its bad token at a frozen position
        st = R.State(x0, S, np.zeros(B, np.float32), np.zeros(B, np.float32))
        st.y = _sent(st.y.shape)
        xin = _sent((S, L, 4))
        D = _Device(st, xin, None)
        err = torch.zeros(1, dtype=torch.int32, device=DEV)
        _launch(D, dev(x0), dev(editable.astype(np.uint8)), dcfg.at(0), _lib.SvddRng(_lib.RNG_REPLAY, 0, ud.data_ptr(), 0, 0, 0, 0),
                B, L, S, d0, 1, 0, 0, True, err=err)
        assert R.step(st, x0, editable, cfg, xin, d0, 1, 0, 0, u=u) == want == int(err[0])
        D.check(st, xin, None, f"token above 3, design {d0}")
    assert (xin[:, 4] == 0).sum() >= 3 * S                                   # a token that is no base: at most one channel set


# ------------------------------------------------------------------------------------------------ whole calls ----
@pytest.fixture(scope="module")
def nets():
    from svdd_amd import synthetic
    return {"rna": synthetic.build("rna", DEV), "tiny": e2e_parity.tiny_engine(load_golden("nets_tiny.npz"), 50, 8, DEV)}


def _device_fns(model, emb, head, L):
    """The scoring and gradient functions Diffusion.ledidi uses, as numpy functions for the restatement's host loop."""
    fused, grad_fn = model._attr_route(emb, head, None, L)
    scorer = model._design_scorer(emb, head, None)

    def score_fn(tok):
        with torch.no_grad():
            return scorer(dev(tok)).cpu().numpy()

    def grad(xin):
        if fused is not None:
            with torch.no_grad():
                return fused.mean_score_input_grad(dev(xin)).cpu().numpy(), float(xin.shape[0])
        xg = dev(xin).requires_grad_(True)
        with torch.enable_grad():
            out = grad_fn(xg)
            g = out[1] if isinstance(out, tuple) else torch.autograd.grad(out.sum(), xg)[0]
        return g.detach().cpu().numpy(), 1.0
    return fused, score_fn, grad


def _equal_to_state(res, st, n_iter, trace):
    _same(res.x_best.cpu().numpy(), st.x_best, "x_best")
    for f in ("score_best", "best_total", "best_output", "best_input", "best_iter"):
        _same(getattr(res, f).cpu().numpy(), getattr(st, f), f)
    assert res.n_iter == n_iter
    _same(res.trace.cpu().numpy(), trace.astype(np.float32), "trace")


WHOLE = {"fused_12_in_16_replay": ("rna", 3, 4, dict(l=0.002, lr=2.5), False, None, True),
         "fused_20_in_32_philox_positions": ("rna", 2, 10, dict(l=0.002, lr=2.5), False, list(range(5, 45, 2)), False),
         "fused_target": ("rna", 3, 4, dict(l=0.002, lr=2.5), True, None, False),
         "generic_tiny": ("tiny", 2, 3, dict(l=0.002, lr=2.5), False, [0, 3, 10, 11, 12, 30, 49], True)}


@pytest.mark.parametrize("name", list(WHOLE))
def test_whole_call_equals_the_host_loop_exactly(nets, name):
    """6 iterations, early_stopping_iter = 2: every result field, n_iter and the trace equal the restatement's host loop around the
    same device scores and gradients (a round trip per iteration there, none here)."""
    net, B, S, hyper, with_target, positions, replay = WHOLE[name]
    model, emb, head = nets[net][:3]
    L, max_iter = 50, 5
    fused, score_fn, grad_fn = _device_fns(model, emb, head, L)
    assert (fused is not None) == (net == "rna")
    rng = np.random.default_rng([7, B, S])
    x0 = rng.integers(0, 4, (B, L)).astype(np.uint8)
    noise = rng.random((max_iter + 1, B, S, L, 4)).astype(np.float32) if replay else None
    target = None
    if with_target:
        target = (score_fn(x0) + np.float32(0.5)).astype(np.float32)
    model.philox_seed, model.row_offset = 99, 0
    res = model.ledidi(dev(x0), emb, head, max_iter=max_iter, batch_size=S, early_stopping_iter=2, positions=positions,
                       target=None if target is None else dev(target), return_trace=True, noise=None if noise is None else dev(noise),
                       **hyper)
    torch.cuda.synchronize()
    editable = None if positions is None else np.isin(np.arange(L), positions)
    cfg = R.Cfg(S, patience=2, **hyper)
    st, n_iter, trace = R.run(x0, score_fn, grad_fn, cfg, max_iter, editable=editable, target=target, noise=noise,
                              philox=(99, 0), chunks=R.chunks_of(B, S, 1024, fused is not None))
    _equal_to_state(res, st, n_iter, trace)
    print(f"ledidi {name}: n_iter {n_iter} stopped {st.stopped.tolist()} best_iter {st.best_iter.tolist()} edits {st.edits.sum(1).tolist()}")
    assert res.trace.shape == (n_iter, B, 3)
    if name in ("fused_20_in_32_philox_positions", "fused_target"):         # early_stopping_iter = 2 stops a design, and not every one:
        assert st.stopped.any() and not st.stopped.all(), st.stopped        # per-design stopping and n_iter are compared non-trivially
    if name == "fused_12_in_16_replay":
        assert st.stopped.all() and n_iter < max_iter + 1                   # every design stops early: the loop ends before max_iter
    if positions is not None:
        frozen = ~editable
        assert (res.x_best.cpu().numpy()[:, :, frozen] == x0[:, None, frozen]).all()


@pytest.fixture(scope="module")
def base_run(nets):
    """One fused-route call shared by the independence and contract tests: B = 5, S = 4, 8 iterations, patience 3, Philox."""
    model, emb, head, _ = nets["rna"]
    x0 = np.random.default_rng(17).integers(0, 4, (5, 50)).astype(np.uint8)
    kw = dict(max_iter=7, batch_size=4, early_stopping_iter=3, l=0.002, lr=2.5, positions=list(range(2, 48)), return_trace=True)
    model.philox_seed, model.row_offset = 5, 0
    return x0, kw, model.ledidi(dev(x0), emb, head, **kw)


def _fields(res):
    return [res.x_best, res.score_best, res.best_total, res.best_output, res.best_input, res.best_iter, res.trace]


def test_result_does_not_depend_on_chunking_polling_or_the_batch(nets, base_run):
    """chunk_rows 4 (one design per pass of 4 rows, five passes), 16 (four designs per pass of 16, then one in 4) and 64 (all 20 rows in
    one pass of 32, the default's chunking), check_every 1 and 4, against the default call: the same bits in every field and the trace.
    Design 3 alone with row_offset 3 has the bits it has inside the batch. The same Philox seed twice gives the same result, another
    seed another one."""
    model, emb, head, _ = nets["rna"]
    x0, kw, want = base_run
    model.philox_seed, model.row_offset = 5, 0
    for extra in (dict(chunk_rows=4), dict(chunk_rows=16), dict(chunk_rows=64), dict(check_every=1), dict(check_every=4)):
        got = model.ledidi(dev(x0), emb, head, **kw, **extra)
        assert got.n_iter == want.n_iter, extra
        for a, b in zip(_fields(got), _fields(want)):
            _same(a.cpu().numpy(), b.cpu().numpy(), str(extra))
    try:
        model.row_offset = 3                                                # design 3 alone, keyed as design 3 of the batch
        alone = model.ledidi(dev(x0[3:4]), emb, head, **kw)
    finally:
        model.row_offset = 0
    n = alone.n_iter
    for a, b in zip(_fields(alone)[:-1], _fields(want)[:-1]):
        assert torch.equal(a[0], b[3])
    _same(alone.trace.cpu().numpy()[:, 0], want.trace.cpu().numpy()[:n, 3], "trace of design 3")
    again = model.ledidi(dev(x0), emb, head, **kw)
    for a, b in zip(_fields(again), _fields(want)):
        _same(a.cpu().numpy(), b.cpu().numpy(), "same seed")
    model.philox_seed = 6
    other = model.ledidi(dev(x0), emb, head, **kw)
    model.philox_seed = 5
    assert not torch.equal(other.trace.nan_to_num(), want.trace.nan_to_num())


def test_result_contracts(nets, base_run):
    """score_best are forward_tokens' bits of x_best; frozen positions equal x0; best_input * S is the Hamming count; best_total is the
    minimum of the trace's total-loss column and of its starting value, best_iter its first occurrence; best_iter == -1 rows are x0."""
    from svdd_amd.diffusion import design_pick
    model, emb, head, _ = nets["rna"]
    x0, kw, res = base_run
    B, S, L = res.x_best.shape
    fn = model.value_callable(emb, head)
    sc = fn.forward_tokens(res.x_best.reshape(B * S, L)).reshape(B, S)
    assert torch.equal(sc, res.score_best)
    xb = res.x_best.cpu().numpy()
    frozen = ~np.isin(np.arange(L), kw["positions"])
    assert (xb[:, :, frozen] == x0[:, None, frozen]).all()
    ham = (xb != x0[:, None, :]).sum(axis=(1, 2))
    assert np.array_equal(res.best_input.cpu().numpy() * np.float32(S), ham.astype(np.float32))
    tr = res.trace.cpu().numpy()
    start = R.output0(res.score0.cpu().numpy(), None, S)
    bi, bt = res.best_iter.cpu().numpy(), res.best_total.cpu().numpy()
    for b in range(B):
        col = tr[:, b, 0]
        col = col[~np.isnan(col)]
        lowest = min(float(col.min()), float(start[b]))
        assert float(bt[b]) == lowest
        assert int(bi[b]) == (-1 if lowest == float(start[b]) else int(np.argmax(col == lowest)))
        if bi[b] == -1:
            assert (xb[b] == x0[b][None]).all()
        else:
            assert (xb[b] != x0[b][None]).any()                             # an iteration without an edit ties with the start: no improvement
    assert (bi >= 0).any()
    tok, score, edits = design_pick(res)
    assert tok.shape == (B, L) and torch.equal(score, res.score_best.max(dim=1).values)
    assert torch.equal(edits.cpu(), (tok.cpu() != torch.from_numpy(x0)).sum(1))


@pytest.mark.parametrize("S", [10, 3])
def test_start_value_ties_with_an_iteration_that_edits_nothing(nets, S):
    """S = 10 and 3 (a division that is not exact), a target, an edit weight no score gain can pay: no design ever improves, so
    best_total / best_output still hold the start value. They are the restatement's bits (the kernel's own formula on S copies of the
    start score, one correctly rounded division), best_iter stays -1, x_best is x0: an iteration without edits ties with the start."""
    model, emb, head, _ = nets["rna"]
    B, L = 32, 50
    x0 = np.random.default_rng([23, S]).integers(0, 4, (B, L)).astype(np.uint8)
    scorer = model._design_scorer(emb, head, None)
    score0 = scorer(dev(x0)).cpu().numpy()
    target = (score0 - np.float32(0.25) + np.float32(0.5) * np.random.default_rng(S).random(B).astype(np.float32)).astype(np.float32)
    model.philox_seed, model.row_offset = 11, 0
    res = model.ledidi(dev(x0), emb, head, max_iter=3, batch_size=S, l=100.0, lr=4.0, target=dev(target), return_trace=True)
    want = R.output0(score0, target, S)
    _same(res.best_total.cpu().numpy(), want, "best_total")
    _same(res.best_output.cpu().numpy(), want, "best_output")
    assert (res.best_iter.cpu().numpy() == -1).all()
    assert (res.x_best.cpu().numpy() == x0[:, None, :]).all()
    tr = res.trace.cpu().numpy()
    assert res.n_iter == 4 and (tr[:, :, 0] >= want[None]).all()
    no_edit = tr[:, :, 2] == 0
    assert no_edit[0].any() and (tr[:, :, 0][no_edit] == np.broadcast_to(want, tr.shape[:2])[no_edit]).all()     # a tie, bit for bit
    acc = np.zeros(B, np.float32)                                           # these inputs tell a true division from a multiplication
    for _ in range(S):                                                      # by the rounded reciprocal
        acc = acc + (score0 - target) * (score0 - target)
    assert (acc * np.float32(1.0 / S) != acc / np.float32(S)).any()


def test_harness_ledidi_reports_the_picks(nets):
    from svdd_amd.harness import BaseModel
    model, emb, head, reward = nets["rna"]
    x0 = dev(np.random.default_rng(17).integers(0, 4, (3, 50)).astype(np.uint8))
    h = BaseModel(emb, head, model, reward, 2)
    model.philox_seed, model.row_offset = 5, 0
    tok, scores, edits, report = h.ledidi(x0, max_iter=3, batch_size=4, l=0.0, lr=4.0)
    assert tok.shape == (3, 50) and scores.shape == (3,) and edits.shape == (3,)
    assert set(report) == {"ledidi_score_gain_mean", "ledidi_edits_mean", "ledidi_improved_fraction", "ledidi_iters"}
    assert report["ledidi_iters"] == 4 and 0.0 <= report["ledidi_improved_fraction"] <= 1.0


def test_mean_sample_score_rises(nets):
    """The sign test: "rna" net, L = 50, B = 8, S = 10, l = 0, 40 iterations without early stopping: the mean over designs of the last
    iteration's mean sample score is above the first's (the float64 restatement does this on five seeds, tests/test_ledidi_cpu.py).
    A gradient with the wrong sign walks the other way."""
    model, emb, head, _ = nets["rna"]
    c = SIGN_CASE
    model.philox_seed, model.row_offset = 0, 0
    res = model.ledidi(dev(sign_case_inputs()), emb, head, max_iter=c["max_iter"], batch_size=c["S"], l=c["l"],
                       early_stopping_iter=c["max_iter"] + 2, return_trace=True)
    assert res.n_iter == c["max_iter"] + 1
    first, last = float(-res.trace[0, :, 1].mean()), float(-res.trace[-1, :, 1].mean())
    print(f"ledidi sign test: first {first:.6e} last {last:.6e} gain {last - first:.6e}")
    assert last > first
