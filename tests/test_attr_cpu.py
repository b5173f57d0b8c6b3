"""No GPU: gradient attributions.

  restatement  tests/attr_ref.py on a quadratic score whose attributions are known in closed form (Gauss-Legendre is exact there);
               fold_ref's independence of the pass cuts; the power-of-two argument of the fused route in float32 itself
  entries      svdd_attr_path / svdd_attr_fold refuse bad arguments before they touch a device; ABI 17; explicit streams
  python       Diffusion.attributions refuses bad arguments before any device work; BaseModel.get_attributions exists
  fixtures     g38 / g39 (the reference's nets in float64, tests/golden/make_golden_attr.py) against attributions_ref on the project's
               own modules in float64
  inputs       the fused-route cases of tests/test_attr_gpu.py keep the float64 reference's tail-kink sequences within the cap
"""
import copy
import ctypes

import numpy as np
import pytest
import torch

from tests import attr_ref as A
from tests import grad_ref as R
from tests.conftest import load_golden


# ------------------------------------------------------------------------------------------------ the restatement ----
def _quadratic(B, L, seed=0):
    rng = np.random.default_rng(seed)
    c, d = torch.from_numpy(rng.standard_normal((L, 4))), torch.from_numpy(rng.standard_normal((L, 4)))
    x = rng.integers(0, 4, (B, L)).astype(np.uint8)
    x[0, 2:4] = 4                                                          # MASK: a zero one-hot row
    base = (0.25 + 0.1 * rng.standard_normal((B, L, 4)))
    return c, d, x, base, (lambda p: (c * p * p + d * p).sum(dim=(1, 2)))


@pytest.mark.parametrize("S", [2, 5])
@pytest.mark.parametrize("with_base", [False, True])
def test_integrated_gradients_of_a_quadratic_are_exact(S, with_base):
    """f(x) = sum c x^2 + d x: the integrand is linear in alpha, Gauss-Legendre with S >= 2 nodes integrates it exactly:
    attr = (x - b) (c (x + b) + d), and completeness holds."""
    B, L = 3, 7
    c, d, x, base, f = _quadratic(B, L)
    base = base if with_base else None
    res = A.attributions_ref(f, x, "integratedgradients", base, A.quadrature_ref(S))
    oh = A.onehot_ref(x, np.float64)
    b = np.zeros_like(oh) if base is None else base
    want = (oh - b) * (c.numpy() * (oh + b) + d.numpy())
    assert np.abs(res["attr"] - want.transpose(0, 2, 1)).max() <= 1e-12
    assert np.abs(res["delta"]).max() <= 1e-12
    assert np.abs(res["attr"].reshape(B, -1).sum(1) - (res["score_x"] - res["score_base"])).max() <= 1e-12
    if base is None:
        assert (res["attr"][0, :, 2:4] == 0).all()                        # MASK columns


def test_one_pass_methods_equal_the_closed_form_gradient():
    B, L = 3, 7
    c, d, x, base, f = _quadratic(B, L, seed=1)
    oh = A.onehot_ref(x, np.float64)
    grad = 2 * c.numpy() * oh + d.numpy()
    assert np.abs(A.attributions_ref(f, x, "gradient")["attr"] - grad.transpose(0, 2, 1)).max() <= 1e-12
    ixg = A.attributions_ref(f, x, "inputxgradient")["attr"]
    assert np.abs(ixg - (oh * grad).transpose(0, 2, 1)).max() <= 1e-12
    assert (ixg[0, :, 2:4] == 0).all() and (A.attributions_ref(f, x, "gradient")["attr"][0, :, 2:4] != 0).all()
    ixb = A.attributions_ref(f, x, "inputxgradient", base)["attr"]       # with a baseline a MASK column is -baseline * gradient
    assert np.abs(ixb - ((oh - base) * grad).transpose(0, 2, 1)).max() <= 1e-12 and (ixb[0, :, 2:4] != 0).all()


def test_quadrature_is_gauss_legendre_on_the_unit_interval():
    for S in (1, 4, 50):
        a, w = A.quadrature_ref(S)
        assert a.shape == w.shape == (S,) and abs(w.sum() - 1.0) <= 1e-14 and (a > 0).all() and (a < 1).all() and (np.diff(a) > 0).all()
        for deg in range(0, 2 * S):                                        # exact to degree 2 S - 1
            assert abs((w * a ** deg).sum() - 1.0 / (deg + 1)) <= 1e-13
    a32, w32 = A.quadrature_ref(50, np.float32)
    assert a32.dtype == np.float32 and np.array_equal(a32, A.quadrature_ref(50)[0].astype(np.float32))


def test_path_restatement_rows_pads_and_exact_onehot():
    x = np.array([[0, 3, 4], [2, 5, 1]], np.uint8)
    al = np.array([0.25, 1.0], np.float32)
    out, err = A.path_ref(x, None, al, 1, 3, n_pad=2)
    assert out.shape == (5, 3, 4) and out.dtype == np.float32 and err == 1
    assert np.array_equal(out[0], A.onehot_ref(x[0])) and np.array_equal(out[2], A.onehot_ref(x[1]))      # alpha = 1: the one-hot
    assert np.array_equal(out[1], A.onehot_ref(x[1]) * np.float32(0.25)) and np.array_equal(out[3:], out[[0, 0]])
    assert (out[0, 2] == 0).all() and (out[2, 1] == 0).all()              # MASK, and a token > 4 acts as MASK
    assert A.path_ref(x, None, al, 0, 2)[1] == 0                          # row 0 alone holds no bad token
    base = np.full((3, 4), 0.5, np.float32)
    out, _ = A.path_ref(x, base, al, 0, 1)
    assert np.array_equal(out[0], base + np.float32(0.25) * (A.onehot_ref(x[0]) - base))


@pytest.mark.parametrize("mode", [A.GRADIENT, A.TIMES_INPUT])
def test_fold_is_independent_of_the_pass_cuts(mode):
    rng = np.random.default_rng(3)
    B, L, S = 3, 70, 5
    x = rng.integers(0, 5, (B, L)).astype(np.uint8)
    grad = rng.standard_normal((B * S, L, 4)).astype(np.float32)
    w = rng.standard_normal(S).astype(np.float32)
    base = rng.standard_normal((B, L, 4)).astype(np.float32)

    def run(cuts):
        acc, attr, rs = (np.full(s, np.nan, np.float32) for s in ((B, L, 4), (B, 4, L), (B,)))
        r0 = 0
        for n in cuts:
            A.fold_ref(grad[r0:], 16.0, w, x, base, r0, n, mode, acc, attr, rs)
            r0 += n
        assert r0 == B * S and not np.isnan(attr).any()
        return acc.tobytes(), attr.tobytes(), rs.tobytes()
    want = run([15])
    for cuts in ([1] * 15, [4, 4, 4, 3], [7, 8], [5, 5, 5], [2, 13]):     # inside a row's steps and at row boundaries
        assert run(cuts) == want, cuts


def test_rowsum_restatement_is_the_sum():
    rng = np.random.default_rng(4)
    for L in (1, 63, 64, 65, 200):
        a = rng.standard_normal((L, 4)).astype(np.float32)
        assert abs(float(A.rowsum_ref(a)) - a.astype(np.float64).sum()) <= 4 * L * 2.0 ** -23 * np.abs(a).sum()
    assert A.rowsum_ref(np.arange(8, dtype=np.float32).reshape(2, 4)) == 28.0


@pytest.mark.parametrize("L", [50, 200])
@pytest.mark.parametrize("n", [1, 2, 64, 2048])
def test_power_of_two_row_counts_undo_the_mean_exactly(n, L):
    """The claim DESIGN 4j rests on, in float32 itself: the host's factor fl(1 / (n L)) (float product n * L, float division) is
    fl(1 / L) scaled by the power of two 1 / n, so n * (g * fl(1 / (n L))) has the bits of g * fl(1 / L)."""
    g = np.random.default_rng(n * 1000 + L).standard_normal(4096).astype(np.float32)
    g[:4] = [1.0, -3.5, 1e-20, 7e19]                                       # normal magnitudes, far from under- and overflow
    f_n = np.float32(1.0) / (np.float32(n) * np.float32(L))
    f_1 = np.float32(1.0) / (np.float32(1) * np.float32(L))
    got = (np.float32(n) * (g * f_n).astype(np.float32)).astype(np.float32)
    assert got.tobytes() == (g * f_1).astype(np.float32).tobytes()
    if n > 1:                                                              # ... and a row count that is no power of two does not
        f_3 = np.float32(1.0) / (np.float32(3 * n) * np.float32(L))
        assert (np.float32(3 * n) * (g * f_3).astype(np.float32)).astype(np.float32).tobytes() != (g * f_1).astype(np.float32).tobytes()


# ------------------------------------------------------------------------------------------------------ the entries ----
def test_attr_entries_refuse_bad_arguments_without_a_device():
    from svdd_amd import _lib
    L_ = _lib.lib()
    assert _lib.ABI_VERSION == 17 and L_.svdd_abi_version() == 17
    for name in ("svdd_attr_path", "svdd_attr_fold"):
        assert name in _lib.EXPORTS
        sig = _lib.SIGNATURES[name]
        assert sig[-1] is _lib.vp and sig[-1] is not _lib.STREAM and _lib.STREAM not in sig      # the stream is the caller's (`on_stream`)
    p = [ctypes.c_void_p(4096 * (i + 1)) for i in range(8)]               # non-NULL pointers that are never dereferenced

    def path(**kw):
        a = dict(x=p[0], baseline=None, baseline_rows=0, alpha=p[1], B=2, L=8, S=3, r0=0, n_rows=6, n_pad=2, out=p[2], err=None, stream=None)
        a.update(kw)
        return L_.svdd_attr_path(*a.values())
    for what, kw in {"B = 0": dict(B=0), "B < 0": dict(B=-1), "L = 0": dict(L=0), "S = 0": dict(S=0), "n_rows = 0": dict(n_rows=0),
                     "n_rows < 0": dict(n_rows=-1), "n_pad < 0": dict(n_pad=-1), "r0 < 0": dict(r0=-1), "past B S": dict(r0=1),
                     "past B S (2)": dict(n_rows=7), "x null": dict(x=None), "alpha null": dict(alpha=None), "out null": dict(out=None),
                     "baseline rows 0": dict(baseline=p[3], baseline_rows=0), "baseline rows 3": dict(baseline=p[3], baseline_rows=3),
                     "2^40 positions": dict(L=1 << 30, n_rows=1, n_pad=1 << 10)}.items():
        assert path(**kw) == _lib.E_ARG, what

    def fold(**kw):
        a = dict(grad=p[0], scale=1.0, weight=p[1], x=p[2], baseline=None, baseline_rows=0, B=2, L=8, S=3, r0=0, n_rows=6,
                 mode=_lib.ATTR_TIMES_INPUT, acc=p[3], attr=p[4], rowsum=None, stream=None)
        a.update(kw)
        return L_.svdd_attr_fold(*a.values())
    for what, kw in {"B = 0": dict(B=0), "L = 0": dict(L=0), "L < 0": dict(L=-4), "S = 0": dict(S=0), "n_rows = 0": dict(n_rows=0),
                     "r0 < 0": dict(r0=-1), "past B S": dict(r0=1), "past B S (2)": dict(n_rows=7), "mode 2": dict(mode=2),
                     "mode -1": dict(mode=-1), "grad null": dict(grad=None), "weight null": dict(weight=None), "x null": dict(x=None),
                     "acc null": dict(acc=None), "attr null": dict(attr=None), "baseline rows 0": dict(baseline=p[5], baseline_rows=0),
                     "baseline rows 3": dict(baseline=p[5], baseline_rows=3), "attr is acc": dict(attr=p[3]),
                     "attr is grad": dict(attr=p[0]), "acc is grad": dict(acc=p[0])}.items():
        assert fold(**kw) == _lib.E_ARG, what


# ------------------------------------------------------------------------------------------------------- the python ----
def _tiny():
    from svdd_amd.config import Config, ModelConfig, SamplingConfig
    from svdd_amd.diffusion import Diffusion
    torch.manual_seed(0)
    return Diffusion(Config(model=ModelConfig(hidden_dim=16, num_cnn_stacks=1, length=20), sampling=SamplingConfig(steps=4))).eval()


def test_attributions_refuses_bad_arguments_without_a_device():
    from svdd_amd import ops
    d = _tiny()
    emb = head = lambda t: t                                               # noqa: E731  (never called)
    x = torch.randint(0, 5, (2, 20), generator=torch.Generator().manual_seed(1))
    call = lambda **kw: d.attributions(x, emb, head, **kw)                 # noqa: E731
    with pytest.raises(ops.SvddError, match="GPU"):                        # a CPU tensor: no CPU fallback
        call()
    with pytest.raises(ValueError, match="method"):
        call(method="deepshap")
    for bad in (torch.zeros(20, 3), torch.zeros(3, 20, 4), torch.zeros(4, 20), torch.zeros(2, 20, 4, 1)):
        with pytest.raises(ValueError, match="baseline"):
            call(method="integratedgradients", baseline=bad)
    with pytest.raises(ValueError, match="baseline"):
        call(baseline=torch.zeros(20, 4, dtype=torch.float64))
    with pytest.raises(ValueError, match="baseline"):
        call(baseline=np.zeros((20, 4), np.float32))
    for bad in (0, -3):
        with pytest.raises(ValueError, match="n_steps"):
            call(method="integratedgradients", n_steps=bad)
    with pytest.raises(ValueError, match="quadrature"):
        call(method="integratedgradients", quadrature=(torch.ones(3), torch.ones(4)))
    with pytest.raises(ValueError, match="quadrature"):
        call(method="integratedgradients", quadrature=(torch.ones(2, 2), torch.ones(2, 2)))
    with pytest.raises(ValueError, match="quadrature"):
        call(method="integratedgradients", quadrature=torch.ones(3))
    for bad in (0, -1):
        with pytest.raises(ValueError, match="chunk_rows"):
            call(chunk_rows=bad)
    for method in ("gradient", "inputxgradient"):
        with pytest.raises(ValueError, match="return_delta"):
            call(method=method, return_delta=True)
    with pytest.raises(ValueError):
        d.attributions(x[0], emb, head)
    with pytest.raises(ops.SvddError, match="GPU"):                        # n_steps is ignored by the one-pass methods: the next check speaks
        call(method="gradient", n_steps=0)


def test_public_signatures():
    import inspect
    from svdd_amd.diffusion import Diffusion
    from svdd_amd.harness import BaseModel
    assert list(inspect.signature(Diffusion.attributions).parameters) == [
        "self", "x", "pre_scorer_embedding", "pre_scorer_head", "reward_model", "method", "baseline", "n_steps", "quadrature",
        "chunk_rows", "return_delta"]
    sig = inspect.signature(Diffusion.attributions).parameters
    assert sig["method"].default == "inputxgradient" and sig["n_steps"].default == 50 and sig["baseline"].default is None
    assert list(inspect.signature(BaseModel.get_attributions).parameters)[:3] == ["self", "samples", "method"]
    assert inspect.signature(BaseModel.get_attributions).parameters["method"].default == "inputxgradient"
    assert Diffusion.ATTR_CHUNK_ROWS == 1024


# ----------------------------------------------------------------------------------------------------- the fixtures ----
@pytest.mark.parametrize("name,task", [("g38_attr_tiny.npz", "rna"), ("g39_attr_full.npz", "dna")])
def test_recorded_reference_attributions_equal_the_restatement_on_our_modules(name, task):
    """The reference's nets in float64 (recorded) against attributions_ref on this project's modules of the same seeded weights,
    cast to float64: two implementations of the same net, the same rule."""
    from svdd_amd import synthetic
    g = load_golden(name)
    _, emb, head, _ = synthetic.build(task, "cpu")
    for nm, mod in (("embedding", emb), ("head", head)):
        sums = np.array([float(p.double().sum()) for p in mod.state_dict().values()])
        assert np.allclose(sums, g[nm + "_param_sums"], rtol=0, atol=1e-6), nm
    emb, head = copy.deepcopy(emb).double(), copy.deepcopy(head).double()
    f = lambda p: head(emb(p))                                             # noqa: E731
    x, quad = g["x"], (g["alphas"], g["weights"])
    assert (x == 4).any() and g["gradient"].shape == (x.shape[0], 4, x.shape[1])
    assert np.abs(A.attributions_ref(f, x, "gradient")["attr"] - g["gradient"]).max() <= 1e-9
    assert np.abs(A.attributions_ref(f, x, "inputxgradient")["attr"] - g["inputxgradient"]).max() <= 1e-9
    for key, base in (("zero", None), ("base", g["baseline"])):
        res = A.attributions_ref(f, x, "integratedgradients", base, quad)
        assert np.abs(res["attr"] - g["ig_" + key]).max() <= 1e-9, key
        assert np.abs(res["score_x"] - g["score_x"]).max() <= 1e-9 and np.abs(res["score_base"] - g["score_" + key]).max() <= 1e-9
        assert np.abs(res["delta"] - g["delta_" + key]).max() <= 1e-9, key
    mask = np.broadcast_to((x == 4)[:, None, :], g["ig_zero"].shape)
    assert (g["ig_zero"][mask] == 0).all() and (g["inputxgradient"][mask] == 0).all() and (g["gradient"][mask] != 0).any()


# ------------------------------------------------------------------------- the fused-route inputs stay within the kink cap ----
@pytest.mark.parametrize("name", list(A.FUSED_CASES))
def test_fused_case_kink_sequences_within_cap(name):
    """The pass tests/test_attr_gpu.py compares with float64 (interpolants from a non-zero baseline, padded to a power of two of
    rows): the sequences with a tail pre-activation within 2e-6 of zero, by the float64 reference alone, stay within seq_cap."""
    from svdd_amd import synthetic
    from svdd_amd.fused import FusedValueNet
    task, L, B, S = A.FUSED_CASES[name]
    _, emb, head, _ = synthetic.build(task, "cpu")
    p = R.to(torch.float64, R.params_of(FusedValueNet(emb, head)))
    x, base, al, _ = A.fused_inputs(name)
    n = B * S
    rows = A.pass_rows(n)
    xp = torch.from_numpy(A.path_ref(x, base, al, 0, n, rows - n)[0]).double()
    res = R.value_grad(xp, p, [m.double() for m in R.free_masks(xp, p)])
    assert int(R.tail_kink_seqs(res["z"]).sum()) <= R.seq_cap(rows)


@pytest.mark.parametrize("name,task", [("g38_attr_tiny.npz", "rna"), ("g39_attr_full.npz", "dna")])
def test_fixture_kink_sequences_within_cap(name, task):
    """The recorded inputs: per table (zero and non-zero baseline) the tail-kink interpolants, by the float64 reference alone, stay
    within seq_cap of the one pass they run in; tests/test_attr_gpu.py leaves those steps out of its comparison with the recording."""
    from svdd_amd import synthetic
    from svdd_amd.fused import FusedValueNet
    g = load_golden(name)
    _, emb, head, _ = synthetic.build(task, "cpu")
    p = R.to(torch.float64, R.params_of(FusedValueNet(emb, head)))
    rows = A.pass_rows(g["x"].shape[0] * g["alphas"].size)
    for key, base in (("zero", None), ("base", g["baseline"])):
        count, steps = A.kink_steps(g["x"], base, g["alphas"], p)
        assert count <= R.seq_cap(rows) and len(steps) <= count, (count, steps)
        assert (count, steps) == A.FIXTURE_KINK_STEPS[(name, key)]
