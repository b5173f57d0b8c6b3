"""CPU checks of Ledidi design: tests/ledidi_ref.py against something independent (torch autograd through the relaxed
graph, torch.optim.AdamW), its fp32 form against its float64 form, the Philox counter layout, the entry's table and refusals, the
public arguments, design_pick, and the sign test's precondition in float64."""
import copy
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import e2e_parity
from tests import ledidi_ref as R
from tests.conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGN_CASE = dict(task="rna", L=50, B=8, S=10, l=0.0, max_iter=39, x_seed=5)      # 40 iterations, no early stopping; the GPU sign test's


@pytest.fixture(scope="module")
def tiny64():
    """The reference's 8-channel value net (tests/golden/nets_tiny.npz) in float64 on the CPU, L = 50."""
    _, emb, head = e2e_parity.tiny_engine(load_golden("nets_tiny.npz"), 50, 8, "cpu")
    emb, head = copy.deepcopy(emb).double(), copy.deepcopy(head).double()
    for m in (emb, head):
        for p in m.parameters():
            p.requires_grad_(False)
    return emb, head


def _net_fns(emb, head, dt=torch.float64):
    def score_fn(tok):
        with torch.no_grad():
            oh = torch.from_numpy(R.onehot(np.asarray(tok))).to(dt)
            return head(emb(oh)).reshape(oh.shape[0], -1)[:, 0].numpy()

    def grad_fn(xin):
        x = torch.from_numpy(np.asarray(xin)).to(dt).requires_grad_(True)
        s = head(emb(x)).reshape(x.shape[0], -1)[:, 0]
        return torch.autograd.grad(s.sum(), x)[0].numpy(), 1.0
    return score_fn, grad_fn


def _torch_total(emb, head, X, w, u, tau, l, eps, target):
    """The `ledidi` package's forward and losses, in torch float64: -> (total, hard tokens [S, L], scores [S])."""
    S = u.shape[0]
    logits = torch.log(X + eps) + w
    g = -torch.log(1e-10 - torch.log(u + 1e-10))
    y = torch.softmax((logits[None] + g) / tau, dim=-1)
    hard = torch.nn.functional.one_hot(y.argmax(-1), 4).to(y.dtype)
    x_hat = hard + (y - y.detach())                                         # straight-through; the forward value is the one-hot EXACTLY
    #                                                                         ((hard + y) - y is 1 - 1e-16 at some kept bases, where sign() is then -1)
    sc = head(emb(x_hat)).reshape(S, -1)[:, 0]
    out = -sc.mean() if target is None else ((sc - target) ** 2).mean()
    inp = (x_hat - X[None]).abs().sum() / (2 * S)
    return out + l * inp, y.argmax(-1), sc


@pytest.mark.parametrize("target", [None, 0.3], ids=["maximise", "target"])
@pytest.mark.parametrize("tau", [1.0, 0.5])
def test_float64_restatement_equals_torch_autograd(tiny64, tau, target):
    """The weight gradient (softmax Jacobian through the straight-through estimator, the L1 sign term, coef_s) to 1e-12 relative, and
    one torch.optim.AdamW step on a float64 parameter to 1e-12."""
    emb, head = tiny64
    L, S, l, eps = 50, 4, 0.1, 1e-4
    rng = np.random.default_rng([3, int(tau * 10), 0 if target is None else 1])
    x0 = rng.integers(0, 4, L).astype(np.uint8)
    w0 = 6.0 * rng.standard_normal((L, 4))                                   # weights large enough that samples carry edits
    u = rng.random((S, L, 4)).astype(np.float32)
    X = torch.from_numpy(R.onehot(x0)).double()
    w = torch.nn.Parameter(torch.from_numpy(w0.copy()))
    opt = torch.optim.AdamW([w], lr=1.0)
    total, tok_t, sc_t = _torch_total(emb, head, X, w, torch.from_numpy(u).double(), tau, l, eps, target)
    total.backward()
    cfg = R.Cfg(S, tau=tau, l=l, eps=eps, dtype=np.float64)
    ed = np.ones(L, bool)
    tok, y, edits = R.sample(x0, ed, w0, u, cfg)
    assert np.array_equal(tok, tok_t.numpy()) and int(edits.sum()) > 0
    score_fn, grad_fn = _net_fns(emb, head)
    sc = score_fn(tok)
    assert np.allclose(sc, sc_t.detach().numpy(), rtol=1e-12, atol=0)
    out, inp, tot = R.losses(sc, edits, target, cfg)
    assert abs(tot - float(total.detach())) <= 1e-12 * abs(float(total.detach()))
    gw = R.weight_grad(x0, tok, y, grad_fn(R.onehot(tok))[0], sc, target, 1.0, cfg)
    want = w.grad.numpy()
    assert np.abs(gw - want).max() <= 1e-12 * np.abs(want).max(), np.abs(gw - want).max()
    opt.step()
    w1, _, _ = R.adamw(w0, np.zeros_like(w0), np.zeros_like(w0), gw, 0, cfg)
    assert np.abs(w1 - w.detach().numpy()).max() <= 1e-12 * np.abs(w1).max()


def test_float64_host_loop_equals_five_torch_iterations(tiny64):
    """Five iterations under replayed noise, AdamW state carried: the same tokens every iteration, weights within 1e-10."""
    emb, head = tiny64
    L, S, l, eps, tau, iters = 50, 3, 0.1, 1e-4, 1.0, 5
    rng = np.random.default_rng(12)
    x0 = rng.integers(0, 4, (1, L)).astype(np.uint8)
    noise = rng.random((iters, 1, S, L, 4)).astype(np.float32)
    X = torch.from_numpy(R.onehot(x0[0])).double()
    w = torch.nn.Parameter(torch.zeros(L, 4, dtype=torch.float64))
    opt = torch.optim.AdamW([w], lr=1.0)
    toks = []
    for i in range(iters):
        opt.zero_grad()
        total, tok_t, _ = _torch_total(emb, head, X, w, torch.from_numpy(noise[i, 0]).double(), tau, l, eps, None)
        toks.append(tok_t.numpy())
        total.backward()
        opt.step()
    cfg = R.Cfg(S, tau=tau, l=l, eps=eps, patience=100, dtype=np.float64)
    seen = []
    score_fn, grad_fn = _net_fns(emb, head)

    def spy(tok):
        if tok.shape[0] == S:
            seen.append(np.array(tok))
        return score_fn(tok)
    st, n_iter, trace = R.run(x0, spy, grad_fn, cfg, iters - 1, noise=noise)
    assert n_iter == iters and len(seen) == iters and trace.shape == (iters, 1, 3)
    for a, b in zip(seen, toks):
        assert np.array_equal(a, b)
    assert np.abs(st.w[0] - w.detach().numpy()).max() <= 1e-10


def test_fp32_restatement_against_float64_after_one_step():
    """One whole step (sample, weight gradient, AdamW) in the kernel's fp32 order against float64: the weights' error is within 8 x
    the error of a second, differently associated fp32 form: a computed bar, no fixed number."""
    L, S = 200, 10
    rng = np.random.default_rng(31)
    x0 = rng.integers(0, 4, L).astype(np.uint8)
    ed = np.ones(L, bool)
    u = rng.random((S, L, 4)).astype(np.float32)
    grad = (1e-3 * rng.standard_normal((S, L, 4))).astype(np.float32)
    sc = rng.standard_normal(S).astype(np.float32)
    w0 = (0.5 * rng.standard_normal((L, 4))).astype(np.float32)
    m0, v0 = (1e-3 * rng.standard_normal((L, 4))).astype(np.float32), (1e-6 * rng.random((L, 4))).astype(np.float32)
    res = {}
    for name, dt, alt in (("f32", np.float32, False), ("alt", np.float32, True), ("f64", np.float64, False)):
        cfg = R.Cfg(S, tau=0.5, l=0.1, dtype=dt)
        tok, y, _ = R.sample(x0, ed, w0.astype(dt), u, cfg, alt=alt)
        w1, m1, v1 = R.update(x0, ed, tok, y, grad, sc.astype(dt), dt(0.25), w0.astype(dt), m0.astype(dt), v0.astype(dt), 3, 16.0,
                              cfg, alt=alt)
        res[name] = (tok, w1.astype(np.float64))
        assert w1.dtype == dt and y.dtype == dt
    assert np.array_equal(res["f32"][0], res["f64"][0]) and np.array_equal(res["alt"][0], res["f64"][0])
    w64 = res["f64"][1]
    err = np.abs(res["f32"][1] - w64).max()
    bar = 8.0 * np.abs(res["alt"][1] - w64).max()
    print(f"ERR ledidi_ref fp32 one step {err:.3e} bar {bar:.1e}")
    assert 0 < err <= bar


def test_philox_restatement_blocks_are_distinct_and_on_their_own_stream_word():
    """The known answer of Philox4x32-10; one block per (design, iteration, sample, position), iterations beyond 16 bits and a row
    offset beyond 32 bits included; word 3's low byte is a stream word no documented entry uses."""
    zero = R.philox4x32_10(np.zeros((1, 4), np.uint32), 0, 0)[0]
    assert [int(v) for v in zero] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    ones = R.philox4x32_10(np.full((1, 4), 0xFFFFFFFF, np.uint32), 0xFFFFFFFF, 0xFFFFFFFF)[0]
    assert [int(v) for v in ones] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    blocks = [R.counters(row, it, 64, 1024).reshape(-1, 4) for row in (0, 1, (1 << 32) + 1) for it in (0, 65535, 65536, 65537, 2 ** 32 - 1)]
    allc = np.concatenate(blocks)
    assert len(np.unique(allc.view([("c", np.uint32, 4)]))) == len(allc) == 15 * 64 * 1024
    assert R.LEDIDI_STREAM not in R.EXISTING_STREAM_WORDS and ((allc[:, 3] & 0xFF) == R.LEDIDI_STREAM).all()
    assert not np.isin(allc[:, 3], R.EXISTING_STREAM_WORDS).any()            # the other entries' word 3 is 0..3 as a whole
    u = R.uniforms(2024, (1 << 32) + 1, 65536, 3, 5)
    assert u.shape == (3, 5, 4) and u.dtype == np.float32 and (u >= 0).all() and (u < 1).all()
    assert not np.array_equal(u, R.uniforms(2024, (1 << 32) + 1, 0, 3, 5))    # 65536 is not iteration 0
    assert not np.array_equal(u, R.uniforms(2024, 1, 65536, 3, 5))
    hdr = open(os.path.join(ROOT, "include", "svdd_hip.h")).read()
    assert "s << 20 | j << 8 | 4" in hdr                                    # the documented layout is the restated one


def test_entry_is_in_the_table_with_the_headers_arity_and_refuses_bad_arguments():
    from svdd_amd import _lib, ops
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "svdd_hip.h")).read(), flags=re.S)
    (params,) = re.findall(r"\bint\s+svdd_ledidi_step\s*\(([^)]*)\)\s*;", hdr)
    names = [p.split()[-1].lstrip("*") for p in params.split(",")]
    sig = _lib.SIGNATURES["svdd_ledidi_step"]
    assert len(sig) == len(names) == 36 and names[-1] == "on_stream" and sig[-1] is _lib.vp and _lib.STREAM not in sig
    assert _lib.ABI_VERSION == 17 and callable(ops.ledidi_step)
    (body,) = re.findall(r"typedef struct svdd_ledidi_cfg \{(.*?)\}", hdr, flags=re.S)
    fields = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.split(None, 1)[1].split(",")]
    assert fields == [n for n, _ in _lib.SvddLedidiCfg._fields_]
    L_ = _lib.lib()
    p = [ctypes.c_void_p(4096 * (i + 1)) for i in range(24)]
    cfg = _lib.SvddLedidiCfg(tau=1.0, l=0.1, patience=3)
    rng = _lib.SvddRng(_lib.RNG_PHILOX, 0, None, 1, 0, 0, 0)

    def call(**kw):
        a = dict(x0=p[0], editable=None, grad=p[1], sc=p[2], target=None, cfg=ctypes.byref(cfg), rng=ctypes.byref(rng), B=2, L=8, S=3,
                 d0=0, nd=2, n_pad=2, iter=0, sample=1, w=p[3], m=p[4], v=p[5], y=p[6], tok=p[7], xin=p[8], edits=p[9],
                 best_total=p[10], best_output=p[11], best_input=p[12], best_iter=p[13], x_best=p[14], score_best=p[15], wo=p[16],
                 stopped=p[17], live=p[18], trace_total=None, trace_out=None, trace_in=None, err=None, stream=None)
        a.update(kw)
        return L_.svdd_ledidi_step(*a.values())
    bad_tau = _lib.SvddLedidiCfg(tau=0.0, l=0.1, patience=3)
    nan_tau = _lib.SvddLedidiCfg(tau=float("nan"), l=0.1, patience=3)
    replay_null = _lib.SvddRng(_lib.RNG_REPLAY, 0, None, 0, 0, 0, 0)
    replay_rows = _lib.SvddRng(_lib.RNG_REPLAY, 0, 4096, 0, 0, 0, 2)
    replay_odd = _lib.SvddRng(_lib.RNG_REPLAY, 0, 4100, 0, 0, 0, 0)
    odd = ctypes.c_void_p(4096 + 4)
    for what, kw in {"B = 0": dict(B=0), "nd = 0": dict(nd=0), "d0 < 0": dict(d0=-1), "past B": dict(d0=1), "L = 0": dict(L=0),
                     "L = 1025": dict(L=1025), "S = 0": dict(S=0), "S = 65": dict(S=65), "n_pad < 0": dict(n_pad=-1),
                     "iter < 0": dict(iter=-1), "x0 null": dict(x0=None), "cfg null": dict(cfg=None), "w null": dict(w=None),
                     "m null": dict(m=None), "v null": dict(v=None), "y null": dict(y=None), "tok null": dict(tok=None),
                     "xin null": dict(xin=None), "edits null": dict(edits=None), "tau 0": dict(cfg=ctypes.byref(bad_tau)),
                     "tau nan": dict(cfg=ctypes.byref(nan_tau)), "sc null": dict(sc=None), "best_total null": dict(best_total=None),
                     "x_best null": dict(x_best=None), "score_best null": dict(score_best=None), "wo null": dict(wo=None),
                     "stopped null": dict(stopped=None), "live null": dict(live=None), "nothing to do": dict(grad=None, sample=0),
                     "rng null": dict(rng=None), "replay without uniforms": dict(rng=ctypes.byref(replay_null)),
                     "replay rows": dict(rng=ctypes.byref(replay_rows)), "uniforms misaligned": dict(rng=ctypes.byref(replay_odd)),
                     "grad misaligned": dict(grad=odd), "xin misaligned": dict(xin=odd), "y misaligned": dict(y=odd),
                     "w misaligned": dict(w=odd)}.items():
        assert call(**kw) == _lib.E_ARG, what


def _tiny():
    from svdd_amd.config import Config, ModelConfig, SamplingConfig
    from svdd_amd.diffusion import Diffusion
    torch.manual_seed(0)
    return Diffusion(Config(model=ModelConfig(hidden_dim=16, num_cnn_stacks=1, length=20), sampling=SamplingConfig(steps=4))).eval()


def test_ledidi_validates_its_arguments_before_it_needs_a_device():
    from svdd_amd import ops
    from svdd_amd.diffusion import Diffusion, LedidiResult                  # noqa: F401
    from svdd_amd.harness import BaseModel
    d = _tiny()
    emb = head = lambda t: t                                               # noqa: E731  (never called)
    x = torch.randint(0, 4, (2, 20), generator=torch.Generator().manual_seed(1))
    call = lambda xx=x, **kw: d.ledidi(xx, emb, head, **kw)                # noqa: E731
    with pytest.raises(ops.SvddError, match="GPU"):                        # everything valid, a CPU tensor: no CPU fallback
        call()
    masked = x.clone()
    masked[1, 3] = 4
    for bad in (masked, x.float(), x[0], torch.zeros((1, 1025), dtype=torch.long), -x - 1):
        with pytest.raises(ValueError, match="x "):
            call(bad)
    for name, bads in {"tau": (0, -1.0, float("nan")), "batch_size": (0, 65), "max_iter": (-1, 2 ** 31), "eps": (0, -1e-4),
                       "lr": (-1.0, float("inf")), "l": (-0.1,), "early_stopping_iter": (0,), "check_every": (0,), "chunk_rows": (0, -4),
                       "positions": ([20], [-1], [3, 3]), "target": ([1.0, 2.0, 3.0], float("nan")),
                       "noise": (torch.zeros(3, 2, 10, 20, 4), torch.zeros(1001, 2, 10, 20), np.zeros(4))}.items():
        for bad in bads:
            with pytest.raises(ValueError, match=name):
                call(**{name: bad})
    with pytest.raises(ops.SvddError, match="GPU"):                        # valid forms of the same arguments
        call(positions=torch.tensor([0, 7, 19]), target=torch.tensor([0.5, 1.0]), max_iter=2, batch_size=1,
             noise=torch.zeros(3, 2, 1, 20, 4))
    with pytest.raises(TypeError):
        call(x, 5)                                                          # everything after reward_model is keyword-only
    p = inspect.signature(Diffusion.ledidi).parameters
    assert list(p) == ["self", "x", "pre_scorer_embedding", "pre_scorer_head", "reward_model", "max_iter", "batch_size", "tau", "l", "lr",
                       "eps", "early_stopping_iter", "positions", "target", "chunk_rows", "check_every", "return_trace", "noise"]
    assert [p[k].default for k in ("max_iter", "batch_size", "tau", "l", "lr", "eps", "early_stopping_iter", "check_every")] == \
        [1000, 10, 1.0, 0.1, 1.0, 1e-4, 100, 32]
    assert list(inspect.signature(BaseModel.ledidi).parameters)[:2] == ["self", "samples"]


def test_ledidi_refuses_a_motif_reward():
    from svdd_amd import motifs
    d = _tiny()
    guided = object.__new__(motifs.GuidedReward)                           # never run: the refusal looks at the type alone
    with pytest.raises(TypeError, match="ledidi"):
        d.ledidi(torch.zeros((1, 20), dtype=torch.long), None, None, reward_model=guided)


def test_design_pick_takes_the_lowest_sample_among_ties():
    from svdd_amd.diffusion import LedidiResult, design_pick
    x0 = torch.tensor([[0, 1, 2, 3], [3, 3, 3, 3], [1, 1, 1, 1]], dtype=torch.uint8)
    xb = x0[:, None, :].repeat(1, 3, 1)
    xb[0, 1, 0], xb[0, 2, 0], xb[0, 2, 1] = 2, 2, 0                         # design 0: samples 1 and 2 tie at the top
    xb[1, 0, 3], xb[1, 2, 0] = 0, 1
    sc = torch.tensor([[0.5, 2.0, 2.0], [1.0, float("nan"), 3.0], [float("nan")] * 3])
    z = torch.zeros(3)
    res = LedidiResult(xb, sc, z, z, z, torch.zeros(3, dtype=torch.int32), 1, None, x0, z)
    tok, score, edits = design_pick(res)
    assert torch.equal(tok, torch.stack([xb[0, 1], xb[1, 2], xb[2, 0]])) and edits.tolist() == [1, 1, 0]
    assert score[:2].tolist() == [2.0, 3.0] and bool(torch.isnan(score[2]))
    tok, score, edits = design_pick(res, target=1.0)                        # closest to the target; |0.5 - 1| = 0.5 < 1
    assert torch.equal(tok[:2], torch.stack([xb[0, 0], xb[1, 0]])) and score[:2].tolist() == [0.5, 1.0]
    tok, score, _ = design_pick(res, target=torch.tensor([2.0, 3.0, 0.0]))
    assert torch.equal(tok[0], xb[0, 1]) and torch.equal(tok[1], xb[1, 2])
    with pytest.raises(ValueError, match="target"):
        design_pick(res, target=[1.0, 2.0])


def sign_case_inputs():
    c = SIGN_CASE
    return np.random.default_rng(c["x_seed"]).integers(0, 4, (c["B"], c["L"])).astype(np.uint8)


def test_sign_test_precondition_holds_in_float64_on_five_noise_seeds():
    """The GPU sign test's configuration ("rna" net, L = 50, B = 8, S = 10, l = 0, 40 iterations, no early stopping) through the
    float64 restatement with the net in float64 on the CPU, Philox seeds 0..4: the mean over designs of the last iteration's mean
    sample score is above the first's in all five. SVDD_LEDIDI_PROFILE=<path> writes the five lines there."""
    from svdd_amd import synthetic
    c = SIGN_CASE
    _, emb, head, _ = synthetic.build(c["task"], "cpu")
    emb, head = copy.deepcopy(emb).double().eval(), copy.deepcopy(head).double().eval()
    score_fn, grad_fn = _net_fns(emb, head)
    x0 = sign_case_inputs()
    cfg = R.Cfg(c["S"], l=c["l"], patience=c["max_iter"] + 2, dtype=np.float64)
    lines = []
    for seed in range(5):
        _, n_iter, trace = R.run(x0, score_fn, grad_fn, cfg, c["max_iter"], philox=(seed, 0))
        assert n_iter == c["max_iter"] + 1
        first, last = -trace[0, :, 1].mean(), -trace[-1, :, 1].mean()       # l = 0: the output loss is minus the mean sample score
        lines.append(f"ledidi_fp64 seed {seed} first {first:.9e} last {last:.9e} gain {last - first:.9e}")
        print(lines[-1])
        assert last > first, lines[-1]
    if os.environ.get("SVDD_LEDIDI_PROFILE"):
        with open(os.environ["SVDD_LEDIDI_PROFILE"], "w") as f:
            f.write("float64 restatement (tests/ledidi_ref.py), seed-44 rna net in float64 on the CPU, L = 50, B = 8, S = 10, l = 0, "
                    "40 iterations: mean sample score of the first and the last iteration\n" + "\n".join(lines) + "\n")
