"""-m gpu: gradient attributions.

  kernels    svdd_attr_path / svdd_attr_fold through the raw C entries in sentinel-guarded buffers: equal to tests/attr_ref.py bit for
             bit (what is written AND what is left alone), whatever the pass cuts
  fused      Diffusion.attributions on the fused ConvGRU value net against the float64 gradient pass of tests/grad_ref.py (the
             kernels' own ReLU decisions pinned, as tests/test_grad_kernels_gpu.py does) pushed through fold_ref in float64
  exactness  the table does not depend on chunk_rows or on the other rows of the batch; input x gradient is n x the mean's gradient
  generic    a length and a head the fused pass refuses (forward_grad + autograd), and an opaque PyTorch net, against float64
  fixtures   g38 / g39 (the reference's nets in float64, tests/golden/make_golden_attr.py) and their completeness gaps, without the
             steps whose interpolants sit on a tail ReLU kink by the float64 reference alone

Bars are computed from references, never from the kernels: grad_ref.bar(8, ref32, ref64) = 8 x max|ref32 - ref64| floored at 2 ulp
of max|ref64| (margin 8: the pass has hardware transcendentals and several reductions). For the fused cases ref32 is grad_ref's
fp32 restatement in the kernels' arithmetic pushed through fold_ref in float32; for the generic route and the fixtures it is torch
fp32 autograd on the CPU. The quadrature weights sum to 1: the fold does not widen a bar. One `ERR <name> <err> bar <bar>` line per
comparison."""
import copy

import numpy as np
import pytest
import torch

from tests import attr_ref as A
from tests import e2e_parity
from tests import grad_ref as R
from tests.conftest import load_golden
from tests.kernel_harness import DEV, SENT32, _Buf, _report, _st

pytestmark = pytest.mark.gpu
SOFT_BAR = 1e-4                    # README: "soft values within 1e-4"


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _sent(*shape):
    """A float32 array holding the guard buffers' sentinel bit pattern: what a reference array starts as."""
    return np.full(shape, SENT32, np.uint32).view(np.float32)


def _same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = got.view(np.uint32) != want.view(np.uint32)
    sent = (got.view(np.uint32) == SENT32) | (want.view(np.uint32) == SENT32)
    bad &= ~(np.isnan(got) & np.isnan(want) & ~sent)                        # a computed NaN equals any computed NaN, never the sentinel
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:5].tolist(), got[bad][:5], want[bad][:5])


# (B, L, S, rows per pass, n_pad of every pass)
CASES = [(1, 1, 1, [1], 0), (2, 3, 5, [4, 4, 2], 0), (3, 33, 7, [8, 8, 5], 3), (2, 50, 4, [8], 0), (1, 200, 3, [3], 0)]
CASE_IDS = ["1x1x1", "2x3x5", "3x33x7", "2x50x4", "1x200x3"]


def _case_inputs(B, L, S, kind):
    rng = np.random.default_rng([B, L, S])
    x = rng.integers(0, 5, (B, L)).astype(np.uint8)                         # tokens 0..4: MASK among them
    x[0, 0] = 4
    alpha = rng.random(S).astype(np.float32)
    alpha[S - 1] = 1.0
    weight = rng.standard_normal(S).astype(np.float32)
    base = {"none": None, "shared": rng.standard_normal((L, 4)).astype(np.float32),
            "per_row": rng.standard_normal((B, L, 4)).astype(np.float32)}[kind]
    return x, alpha, weight, base


# ------------------------------------------------------------------------------------------------ svdd_attr_path ----
def _path(x, base, alpha, r0, n_rows, n_pad, misalign=0, want_err=True):
    """One svdd_attr_path launch through the raw C entry into a guarded buffer (misalign: floats the output is offset by)."""
    from svdd_amd import _lib
    B, L = x.shape
    numel = (n_rows + n_pad) * L * 4
    xd, ad, bd = dev(x), dev(alpha), None if base is None else dev(base)
    out, err = _Buf(numel + misalign), torch.zeros(1, dtype=torch.int32, device=DEV)
    rc = _lib.lib().svdd_attr_path(xd.data_ptr(), None if bd is None else bd.data_ptr(), 0 if base is None else (1 if base.ndim == 2 else B),
                                   ad.data_ptr(), B, L, alpha.size, r0, n_rows, n_pad, out.ptr + 4 * misalign,
                                   err.data_ptr() if want_err else None, _st())
    _lib.check(rc, "svdd_attr_path")
    torch.cuda.synchronize()
    mask = torch.ones(numel + misalign, dtype=torch.bool)
    mask[:misalign] = False
    out.assert_written_where("out", mask)
    return out.cpu().numpy()[misalign:].reshape(n_rows + n_pad, L, 4), int(err[0])


@pytest.mark.parametrize("kind", ["none", "shared", "per_row"])
@pytest.mark.parametrize("B,L,S,cuts,n_pad", CASES, ids=CASE_IDS)
def test_attr_path_kernel_matches_the_restatement(B, L, S, cuts, n_pad, kind):
    """Every pass of every case, exact; guards intact; the output offset by 4 bytes (the scalar path) on the 33-position case; pad rows
    are copies of row 0; alpha = 1 without a baseline is the exact one-hot."""
    x, alpha, _, base = _case_inputs(B, L, S, kind)
    r0 = 0
    for n in cuts:
        want, _ = A.path_ref(x, base, alpha, r0, n, n_pad)
        got, err = _path(x, base, alpha, r0, n, n_pad, misalign=1 if L == 33 else 0)
        _same_bits(got, want, f"path r0={r0}")
        assert err == 0
        for i in range(n_pad):
            assert got[n + i].tobytes() == got[0].tobytes()
        r0 += n
    assert r0 == B * S
    if kind == "none":
        got, _ = _path(x, None, alpha, B * S - 1, 1, 0)                     # the last pair: alpha = 1
        assert np.array_equal(got[0], A.onehot_ref(x[B - 1]))


def test_attr_path_flags_a_token_above_mask_and_treats_it_as_mask():
    x, alpha, _, base = _case_inputs(2, 50, 4, "shared")
    bad, as_mask = x.copy(), x.copy()
    bad[1, 17], as_mask[1, 17] = 5, 4
    got, err = _path(bad, base, alpha, 0, 8, 0)
    want, werr = A.path_ref(bad, base, alpha, 0, 8)
    assert err == 1 and werr == 1
    _same_bits(got, want, "token 5")
    _same_bits(got, _path(as_mask, base, alpha, 0, 8, 0)[0], "token 5 acts as 4")
    assert _path(bad, base, alpha, 0, 4, 0)[1] == 0                         # row 0 alone: nothing to flag
    _path(bad, base, alpha, 0, 8, 0, want_err=False)                        # err NULL: accepted


# ------------------------------------------------------------------------------------------------ svdd_attr_fold ----
class _Fold:
    """acc / attr / rowsum in guarded buffers that live across the passes of one table, beside reference arrays that start as the
    sentinel too: after every pass the buffers must hold the references' bits, written and unwritten elements alike."""

    def __init__(self, x, weight, base, mode, scale, want_rowsum=True):
        self.x, self.weight, self.base, self.mode, self.scale = x, weight, base, mode, scale
        B, L = x.shape
        self.acc, self.attr, self.rowsum = _Buf(B * L * 4), _Buf(B * 4 * L), (_Buf(B) if want_rowsum else None)
        self.r_acc, self.r_attr, self.r_rowsum = _sent(B, L, 4), _sent(B, 4, L), (_sent(B) if want_rowsum else None)
        self.xd, self.wd, self.bd = dev(x), dev(weight), None if base is None else dev(base)

    def fold(self, grad, r0, n_rows):
        """grad [>= n_rows, L, 4] float32 numpy: the pass's gradients (rows beyond n_rows must not be read)."""
        from svdd_amd import _lib
        B, L = self.x.shape
        gd = dev(grad)
        rc = _lib.lib().svdd_attr_fold(gd.data_ptr(), self.scale, self.wd.data_ptr(), self.xd.data_ptr(),
                                       None if self.bd is None else self.bd.data_ptr(),
                                       0 if self.base is None else (1 if self.base.ndim == 2 else B), B, L, self.weight.size, r0, n_rows,
                                       self.mode, self.acc.ptr, self.attr.ptr, None if self.rowsum is None else self.rowsum.ptr, _st())
        _lib.check(rc, "svdd_attr_fold")
        torch.cuda.synchronize()
        A.fold_ref(grad, self.scale, self.weight, self.x, self.base, r0, n_rows, self.mode, self.r_acc, self.r_attr, self.r_rowsum)
        for buf, ref, what in ((self.acc, self.r_acc, "acc"), (self.attr, self.r_attr, "attr"), (self.rowsum, self.r_rowsum, "rowsum")):
            if buf is not None:
                buf.untouched()                                             # asserts both guards
                _same_bits(buf.cpu().numpy().reshape(ref.shape), ref, f"{what} after r0={r0}")

    def results(self):
        B, L = self.x.shape
        return (self.acc.cpu().numpy().reshape(B, L, 4), self.attr.cpu().numpy().reshape(B, 4, L),
                None if self.rowsum is None else self.rowsum.cpu().numpy())


def _with_nan_pads(grad, r0, n, n_pad):
    """The pass's gradient rows followed by n_pad rows of NaN: what a padded pass hands the fold (never read)."""
    return np.concatenate([grad[r0:r0 + n], np.full((n_pad,) + grad.shape[1:], np.nan, np.float32)])


@pytest.mark.parametrize("kind", ["none", "shared", "per_row"])
@pytest.mark.parametrize("mode", [A.GRADIENT, A.TIMES_INPUT], ids=["gradient", "times_input"])
@pytest.mark.parametrize("B,L,S,cuts,n_pad", CASES, ids=CASE_IDS)
def test_attr_fold_kernel_matches_the_restatement(B, L, S, cuts, n_pad, mode, kind):
    """The case's passes, exact after every pass (unfinished rows' attr and rowsum still the sentinel); one pass and pair-by-pair
    passes give the same bits; pad rows hold NaN and are never read; the row sum is close to the float64 sum."""
    x, _, weight, base = _case_inputs(B, L, S, kind)
    grad = np.random.default_rng([7, B, L, S]).standard_normal((B * S, L, 4)).astype(np.float32)
    tables = []
    for plan in (cuts, [B * S], [1] * (B * S)):
        f = _Fold(x, weight, base, mode, 16.0)
        r0 = 0
        for n in plan:
            f.fold(_with_nan_pads(grad, r0, n, n_pad), r0, n)
            r0 += n
        tables.append(f.results())
    for t in tables[1:]:
        for a, b, what in zip(t, tables[0], ("acc", "attr", "rowsum")):
            _same_bits(a, b, what)
    acc, attr, rowsum = tables[0]
    assert not np.isnan(attr).any() and not np.isnan(acc).any() and not np.isnan(rowsum).any()
    a64 = attr.astype(np.float64)
    assert (np.abs(rowsum - a64.reshape(B, -1).sum(1)) <= 4 * L * 2.0 ** -23 * np.abs(a64).reshape(B, -1).sum(1)).all()
    if mode == A.TIMES_INPUT and kind == "none":
        assert (attr.transpose(0, 2, 1)[x == 4] == 0).all()                 # a MASK position's column


def test_attr_fold_keeps_a_nan_in_its_row_and_takes_no_rowsum():
    B, L, S = 3, 33, 7
    x, _, weight, base = _case_inputs(B, L, S, "per_row")
    grad = np.random.default_rng(8).standard_normal((B * S, L, 4)).astype(np.float32)
    grad[S + 2, 5, 1] = np.nan                                              # row 1, step 2
    f = _Fold(x, weight, base, A.TIMES_INPUT, 4.0)
    f.fold(grad, 0, B * S)
    _, attr, rowsum = f.results()
    assert np.isnan(attr[1, 1, 5]) and np.isnan(rowsum[1]) and int(np.isnan(attr).sum()) == 1 and not np.isnan(rowsum[[0, 2]]).any()
    g = _Fold(x, weight, base, A.TIMES_INPUT, 4.0, want_rowsum=False)       # rowsum NULL
    g.fold(grad, 0, B * S)
    _same_bits(g.results()[1], attr, "attr without rowsum")


# ------------------------------------------------------------------------------------------------ whole calls ----
@pytest.fixture(scope="module")
def nets():
    """"rna" / "dna": the seed-44 full-size nets at L = 50 / 200 (the nets of g38 / g39); "two": a 64-channel ConvGRU value net with
    a two-task head; "tiny": the reference's 8-channel value net (PyTorch modules: the opaque route)."""
    from svdd_amd import synthetic
    from svdd_amd.value_nets import ConvGRUTrunk, ConvHead
    torch.manual_seed(91)
    emb2 = ConvGRUTrunk(stem_in_channels=4, stem_channels=64, stem_kernel_size=15, n_conv=6, channel_init=64, kernel_size=5, dropout=0.1)
    head2 = ConvHead(2, 64)
    for m in (emb2, head2):
        m.to(DEV).eval()
        for p in m.parameters():
            p.requires_grad_(False)
    return {"rna": synthetic.build("rna", DEV), "dna": synthetic.build("dna", DEV), "two": (emb2, head2),
            "tiny": e2e_parity.tiny_engine(load_golden("nets_tiny.npz"), 50, 8, DEV)}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@pytest.mark.parametrize("name", list(A.FUSED_CASES))
def test_fused_route_vs_float64_with_pinned_tower_decisions(nets, name):
    """Integrated gradients from a non-zero baseline in ONE pass (15 pairs padded to 16 rows; 8 pairs), every element against
    grad_ref.value_grad in float64 under the kernels' own tower decisions, scaled to the row's gradient and pushed through fold_ref in
    float64. A row with a pass sequence whose tail pre-activation lies within 2e-6 of zero is excluded (cap: seq_cap of the pass's
    rows; tests/test_attr_cpu.py holds it for these inputs)."""
    task, L, B, S = A.FUSED_CASES[name]
    model, emb, head, _ = nets[task]
    fn = model._classifier_fused_value(emb, head, L)
    assert fn is not None
    x, base, al, w = A.fused_inputs(name)
    n = B * S
    rows = A.pass_rows(n)
    fn.keep_grad_pass = True
    try:
        attr = model.attributions(dev(x), emb, head, method="integratedgradients", baseline=dev(base), n_steps=S, chunk_rows=rows)
        kept = fn.last_grad_pass
    finally:
        fn.keep_grad_pass, fn.last_grad_pass = False, None
    torch.cuda.synchronize()
    fs = [f.cpu() for f in kept["fs"]]
    assert fs[0].shape == (rows, L, 64) and attr.shape == (B, 4, L) and attr.dtype == torch.float32
    xp = _t(A.path_ref(x, base, al, 0, n, rows - n)[0])
    p = R.params_of(fn)
    masks = [(f > 0) for f in fs]
    r64, r32 = R.ref64(R.value_grad, xp, p, masks), R.ref32(R.value_grad, xp, p, masks)
    kink = R.tail_kink_seqs(r64["z"])
    assert int(kink.sum()) <= R.seq_cap(rows), int(kink.sum())
    keep_row = torch.tensor([not bool(kink[b * S:(b + 1) * S].any()) for b in range(B)])
    refs = []
    for g, dt in ((r32["grad"], np.float32), (r64["grad"], np.float64)):
        acc, out = np.zeros((B, L, 4), dt), np.zeros((B, 4, L), dt)
        A.fold_ref(g.numpy().astype(dt), float(rows), w.astype(dt), x, base.astype(dt), 0, n, A.TIMES_INPUT, acc, out)
        refs.append(_t(out))
    keep = keep_row[:, None, None].expand(B, 4, L)
    _report(f"attr_fused {name} L={L} B={B} S={S}", attr.cpu(), refs[1], refs[0], 8, keep=keep)


def _ig(model, emb, head, x, **kw):
    return model.attributions(dev(x), emb, head, method="integratedgradients", **kw)


def test_fused_table_does_not_depend_on_chunk_rows_or_on_the_batch(nets):
    """L = 50, 21 (row, step) pairs: chunk_rows 8 (passes of 8, 8 and 5 padded to 8), 16 (16, then 5 padded to 8) and 64 (one pass of
    32) give the same bits: every pass's 1 / n is a power of two and every gradient-pass kernel treats rows independently. Row 1 of
    the B = 3 call equals the B = 1 call on that row. A chunk_rows that is no power of two is rounded down to one."""
    model, emb, head, _ = nets["rna"]
    assert model._classifier_fused_value(emb, head, 50) is not None
    x, base, _, _ = A.fused_inputs("rna")
    tables = {c: _ig(model, emb, head, x, baseline=dev(base), n_steps=7, chunk_rows=c, return_delta=True) for c in (8, 16, 64, 13)}
    for c in (16, 64, 13):
        assert torch.equal(tables[c][0], tables[8][0]) and torch.equal(tables[c][1], tables[8][1]), c
    one = _ig(model, emb, head, x[1:2], baseline=dev(base), n_steps=7)
    assert torch.equal(one[0], tables[8][0][1])
    per_row = _ig(model, emb, head, x, baseline=dev(np.broadcast_to(base, (3, 50, 4)).copy()), n_steps=7, chunk_rows=8)
    assert torch.equal(per_row, tables[8][0])


def test_input_x_gradient_is_n_times_the_means_gradient(nets):
    """inputxgradient = onehot * (n * mean_score_input_grad(onehot)) bit for bit, n = 4 (3 rows padded with a copy of row 0): the
    row's attribution carries no 1 / B. gradient is the same table without the one-hot; a MASK column is 0 in the one, not the other."""
    from svdd_amd import ops
    model, emb, head, _ = nets["rna"]
    fn = model._classifier_fused_value(emb, head, 50)
    x, _, _, _ = A.fused_inputs("rna")
    xd = dev(x)
    oh = ops.transform_samples(torch.cat([xd, xd[:1]]))
    g = fn.mean_score_input_grad(oh)[:3] * 4.0
    assert torch.equal(model.attributions(xd, emb, head, method="gradient"), g.permute(0, 2, 1))
    ixg = model.attributions(xd, emb, head)
    assert torch.equal(ixg, (oh[:3] * g).permute(0, 2, 1))
    m = torch.from_numpy(x == 4).to(DEV)
    assert bool((ixg.permute(0, 2, 1)[m] == 0).all()) and bool((g[m] != 0).any())
    assert torch.equal(model.attributions(xd.long(), emb, head, n_steps=0), ixg)            # any integer dtype; n_steps ignored


def test_attributions_refuses_a_token_above_mask(nets):
    from svdd_amd import ops
    model, emb, head, _ = nets["rna"]
    x, _, _, _ = A.fused_inputs("rna")
    bad = x.copy()
    bad[2, 9] = 5
    with pytest.raises(ops.SvddError, match="token"):
        model.attributions(dev(bad), emb, head)
    with pytest.raises(ops.SvddError, match="GPU"):
        model.attributions(dev(x), emb, head, baseline=torch.zeros(50, 4))                  # a CPU baseline


def _cpu_refs(emb, head, x, method, base, quad, dtypes=(torch.float64, torch.float32)):
    """attributions_ref in float64 and in fp32 (torch autograd on the CPU) on copies of the modules."""
    out = []
    for dt in dtypes:
        e, h = copy.deepcopy(emb).cpu().to(dt), copy.deepcopy(head).cpu().to(dt)
        out.append(A.attributions_ref(lambda p: h(e(p)), x, method, base, quad, dtype=dt))
    return out


@pytest.mark.parametrize("method", ["gradient", "integratedgradients"])
def test_generic_route_two_task_head_at_a_length_the_fused_pass_refuses(nets, method):
    """L = 33 and a two-task head (task 0 explained): the fused pass applies to neither; the interpolants go through forward_grad
    and torch autograd of the sum of the pass's scores, in passes of 5 rows."""
    from svdd_amd.fused import FusedValueNet
    model = nets["rna"][0]
    emb, head = nets["two"]
    B, L, S = 2, 33, 4
    fused, _ = model._attr_route(emb, head, None, L)
    assert fused is None and isinstance(model.value_callable(emb, head), FusedValueNet)
    rng = np.random.default_rng(21)
    x = rng.integers(0, 5, (B, L)).astype(np.uint8)
    base = (0.25 + 0.05 * rng.standard_normal((B, L, 4))).astype(np.float32)
    quad = A.quadrature_ref(S)
    got = model.attributions(dev(x), emb, head, method=method, baseline=dev(base), n_steps=S, chunk_rows=5)
    r64, r32 = _cpu_refs(emb, head, x, method, base, quad)
    _report(f"attr_generic two-task L={L} {method}", got.cpu(), _t(r64["attr"]), _t(r32["attr"]), 8)


def test_generic_route_opaque_modules_and_the_reward_layout(nets):
    """The tiny 8-channel value net (PyTorch modules, autograd inside _gru_backward_ready) at L = 50, and the same net wrapped as a
    reward model fed [n, 4, L]."""
    model, emb, head = nets["tiny"]
    B, L, S = 2, 50, 3
    assert model._attr_route(emb, head, None, L)[0] is None
    rng = np.random.default_rng(22)
    x = rng.integers(0, 5, (B, L)).astype(np.uint8)
    quad = A.quadrature_ref(S)
    got, delta = model.attributions(dev(x), emb, head, method="integratedgradients", n_steps=S, return_delta=True)
    r64, r32 = _cpu_refs(emb, head, x, "integratedgradients", None, quad)
    _report(f"attr_generic opaque L={L}", got.cpu(), _t(r64["attr"]), _t(r32["attr"]), 8)
    assert delta.shape == (B,) and bool(torch.isfinite(delta).all())

    class Reward(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.emb, self.head = emb, head

        def forward(self, t):                                               # [n, 4, L]
            return self.head(self.emb(t.transpose(1, 2)))
    rw = model.attributions(dev(x), None, None, reward_model=Reward(), method="integratedgradients", n_steps=S)
    _report(f"attr_generic opaque reward layout L={L}", rw.cpu(), _t(r64["attr"]), _t(r32["attr"]), 8)


# ------------------------------------------------------------------------------------------------ the fixtures ----
@pytest.mark.parametrize("name,task", [("g38_attr_tiny.npz", "rna"), ("g39_attr_full.npz", "dna")])
def test_recorded_reference_attributions_on_the_fused_route(nets, name, task):
    """g38 / g39: the reference's nets in float64 on the CPU against the engine's tables on the fused route, under
    bar(8, ref32, ref64), ref32 = torch fp32 autograd on the CPU on this project's modules. Against a recording the net's ReLU
    decisions are free, so the integrated-gradients tables are compared WITHOUT the steps that hold a tail-kink interpolant (a tail
    pre-activation within 2e-6 of zero, where an fp32 evaluation may take either side and the gradient jumps: grad_ref.tail_kink_seqs),
    found by the float64 reference alone: at most seq_cap of the pass's rows (a condition here, held for the recorded inputs by
    tests/test_attr_cpu.py; the fixture's seed was chosen by that count, tests/golden/make_golden_attr.py). IG is linear in its
    steps: the engine's table of the excluded steps alone (the same call with the quadrature restricted to them) is taken off the
    engine's full 50-step table, and the same table in float64 on this project's modules (equal to the reference's nets to 1e-9,
    tests/test_attr_cpu.py) off the recording. return_delta is compared the same way, under a bar that also holds one fp32 ulp of
    every term of the difference (the gap is a difference of two scores and the row's sum). The largest deviation of the FULL tables
    from the recording, excluded steps included, is reported against the project's soft-value figure of 1e-4 and held to it."""
    g = load_golden(name)
    model, emb, head, _ = nets[task]
    x, S = g["x"], int(g["alphas"].size)
    B, L = x.shape
    assert model._attr_route(emb, head, None, L)[0] is not None
    rows = A.pass_rows(B * S)
    tag = name.split("_")[0]
    worst = 0.0
    for key, method in (("gradient", "gradient"), ("inputxgradient", "inputxgradient")):
        attr = model.attributions(dev(x), emb, head, method=method)
        (r32,) = _cpu_refs(emb, head, x, method, None, None, dtypes=(torch.float32,))
        worst = max(worst, float((attr.cpu().double() - _t(g[key])).abs().max()))
        _report(f"attr_{tag} {key}", attr.cpu(), _t(g[key]), _t(r32["attr"]), 8)
    for key, base in (("zero", None), ("base", g["baseline"])):
        based = None if base is None else dev(base)
        count, steps = A.FIXTURE_KINK_STEPS[(name, key)]                   # = A.kink_steps(x, base, alphas, the net): test_attr_cpu.py
        assert count <= R.seq_cap(rows), (count, R.seq_cap(rows))
        keep = np.setdiff1d(np.arange(S), steps)
        attr, delta = model.attributions(dev(x), emb, head, method="integratedgradients", baseline=based, n_steps=S, return_delta=True)
        worst = max(worst, float((attr.cpu().double() - _t(g["ig_" + key])).abs().max()))
        got, want = attr.cpu().double(), _t(g["ig_" + key])
        got_sum, want_gap = delta.cpu().double(), _t(g["delta_" + key])
        if steps:                                                           # take the excluded steps' share off both sides
            sub = (g["alphas"][steps], g["weights"][steps])
            off = model.attributions(dev(x), emb, head, method="integratedgradients", baseline=based,
                                     quadrature=(_t(sub[0]), _t(sub[1]))).cpu().double()
            (off64,) = _cpu_refs(emb, head, x, "integratedgradients", base, sub, dtypes=(torch.float64,))
            got, want = got - off, want - _t(off64["attr"])
            got_sum, want_gap = got_sum - off.reshape(B, -1).sum(1), want_gap - _t(off64["attr"]).reshape(B, -1).sum(1)
        (r32,) = _cpu_refs(emb, head, x, "integratedgradients", base, (g["alphas"][keep], g["weights"][keep]), dtypes=(torch.float32,))
        _report(f"attr_{tag} ig_{key} without {len(steps)} of {S} steps ({count} kink interpolants)", got, want, _t(r32["attr"]), 8)
        terms = np.abs(g["score_x"]) + np.abs(g["score_" + key]) + np.abs(g["ig_" + key]).reshape(B, -1).sum(1)
        bar = max(8.0 * float((_t(r32["delta"]).double() - want_gap).abs().max()), 2.0 * R.FP32_EPS * float(terms.max()))
        err = float((got_sum - want_gap).abs().max())
        print(f"ERR attr_{tag} delta_{key} {err:.3e} bar {bar:.1e} (recorded gap {np.abs(g['delta_' + key]).max():.3e})")
        assert err <= bar, (key, err, bar)
    print(f"ERR attr_{tag} largest deviation of the full tables {worst:.3e} bar {SOFT_BAR:.0e}")
    assert worst <= SOFT_BAR


def test_harness_get_attributions_is_the_diffusion_call(nets):
    from svdd_amd.harness import BaseModel
    model, emb, head, reward = nets["rna"]
    x, base, _, _ = A.fused_inputs("rna")
    h = BaseModel(emb, head, model, reward, 2)
    want = model.attributions(dev(x), emb, head, reward_model=reward)
    assert torch.equal(h.get_attributions(dev(x)), want)
    assert not torch.equal(want, model.attributions(dev(x), emb, head))                     # the value net is another net
    a, d = h.get_attributions(dev(x), method="integratedgradients", baseline=dev(base), n_steps=5, return_delta=True)
    b, e = model.attributions(dev(x), emb, head, reward_model=reward, method="integratedgradients", baseline=dev(base), n_steps=5,
                              return_delta=True)
    assert torch.equal(a, b) and torch.equal(d, e)
