"""No GPU: motif-guided SVDD-PM decoding.

  restatement  tests/motif_reward_ref.py's term against a brute-force Python loop over every window of every row, on random small
               cases (both strands and forward only, L below some widths, caps and floors of 0, negative coefficients, a token 4)
  MotifReward  quantisation of float weights, the default margin floor, {name: value} dicts, the 2^62 bound, refusals
  entry        svdd_motif_reward refuses every bad argument before it touches a device; ABI 17; explicit stream
  python       ops.motif_reward / MotifReward / GuidedReward refuse bad arguments before any launch and say "GPU" without a device;
               the gradient samplers and attributions refuse a GuidedReward with a TypeError; signatures; the --guide_* flags
"""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

from svdd_amd import motifs
from tests import motif_reward_ref as RR

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "motifs_tiny.meme")


@pytest.fixture(scope="module")
def tiny():
    return motifs.load_meme(FIXTURE, pvalue=1e-2)


# ------------------------------------------------------------------------------------------------ the restatement ----
def _brute_term(x, mset, c, both):
    """Row by row, motif by motif, window by window, with Python ints."""
    out = []
    for row in x:
        row = [0 if t > 3 else int(t) for t in row]
        T = 0
        for m in range(len(mset.width)):
            w, thr = int(mset.width[m]), int(mset.threshold[m])
            hits, best = 0, None
            for p in range(len(row) - w + 1):
                scores = [sum(int(mset.pwm[m][i][row[p + i]]) for i in range(w))]
                if both:
                    scores.append(sum(int(mset.pwm[m][w - 1 - i][3 - row[p + i]]) for i in range(w)))
                hits += sum(s >= thr for s in scores)
                best = max(scores + ([] if best is None else [best]))
            margin = -int(c.margin_floor[m]) if best is None else max(min(best - thr, 0), -int(c.margin_floor[m]))
            T += int(c.hit_coef[m]) * min(hits, int(c.hit_cap[m])) + int(c.margin_coef[m]) * margin
        out.append(T)
    return out


@pytest.mark.parametrize("seed,L,widths", [(0, 1, (1, 2)), (1, 9, (1, 3, 9, 12)), (2, 20, (4, 8, 16, 17, 20)), (3, 37, (32, 5, 1))])
def test_restatement_equals_the_brute_force(seed, L, widths):
    rng = np.random.default_rng(seed)
    mset, c = RR.random_case(rng, widths)
    x = rng.integers(0, 4, (5, L))
    if L > 1:
        x[2, 1] = 4                                                       # read as 0
    for both in (True, False):
        got = RR.term_ref(x, mset, c.hit_coef, c.hit_cap, c.margin_coef, c.margin_floor, both)
        assert got.dtype == np.int64 and got.tolist() == _brute_term(x, mset, c, both)
    if L < max(widths):                                                   # no window: exactly -margin_floor times the coefficient
        only = [m for m, w in enumerate(widths) if w > L]
        sub, _ = RR.random_case(rng, [widths[m] for m in only])
        z = np.zeros(len(only), np.int32)
        got = RR.term_ref(x, sub, z, z, z + 3, z + 7)
        assert got.tolist() == [-21 * len(only)] * 5


def test_score_is_two_fp32_operations():
    T = np.array([0, 1, -3, (1 << 40) + 1, -(1 << 52) - 12345, (1 << 24) + 1], np.int64)
    s = RR.score_ref(T, 2.0 ** -10)
    assert s.dtype == np.float32 and s[3] == np.float32(2.0 ** 30) and s[5] == np.float32(2.0 ** 14)    # (2^24 + 1 rounds to even)
    b = np.array([1.5, -2.0, 0.25, 3.0, 1e30, -16384.0], np.float32)
    assert np.array_equal(RR.score_ref(T, 2.0 ** -10, b), b + s) and RR.score_ref(T, 2.0 ** -10, b)[5] == 0.0


# --------------------------------------------------------------------------------------------------- MotifReward ----
def test_quantisation_floor_and_names(tiny):
    names = tiny.names
    mr = motifs.MotifReward(tiny, hit_weight={names[1]: 2.0, names[4]: -1.0}, margin_weight={names[5]: 0.01})
    assert mr.unit == 2.0 ** -10 and mr.both and len(mr) == 6
    assert mr.hit_coef.dtype == mr.margin_coef.dtype == mr.hit_cap.dtype == mr.margin_floor.dtype == np.int32
    assert mr.hit_coef.tolist() == [0, 2048, 0, 0, -1024, 0]              # unnamed motifs get 0
    assert mr.margin_coef.tolist() == [0, 0, 0, 0, 0, 10]                 # 0.01 * 1024 = 10.24
    assert mr.hit_cap.tolist() == [1] * 6
    assert mr.margin_floor.tolist() == RR.default_floor_ref(tiny)         # the threshold minus the lowest reachable score
    assert mr.bound == RR.bound_ref(mr.hit_coef, mr.hit_cap, mr.margin_coef, mr.margin_floor)
    w = [0.3, -0.7004, 1.0 / 3, 5e-4, 4.8828125e-4, 1.46484375e-3]        # the last two are ties at unit = 2^-10: half to even
    mr = motifs.MotifReward(tiny, hit_weight=w, margin_weight=np.array(w[::-1]), hit_cap=[0, 1, 2, 3, 4, 5], margin_floor=7, unit=2.0 ** -10)
    assert mr.hit_coef.tolist() == RR.quantise_ref(w, 2.0 ** -10) == [307, -717, 341, 1, 0, 2]
    assert mr.margin_coef.tolist() == RR.quantise_ref(w[::-1], 2.0 ** -10)
    assert mr.hit_cap.tolist() == [0, 1, 2, 3, 4, 5] and mr.margin_floor.tolist() == [7] * 6
    mr = motifs.MotifReward(tiny, hit_weight=1.0, hit_cap={names[0]: 3}, margin_floor={names[2]: 0}, unit=0.25, strands="forward")
    assert mr.hit_coef.tolist() == [4] * 6 and mr.hit_cap.tolist() == [3, 1, 1, 1, 1, 1] and not mr.both
    floor = RR.default_floor_ref(tiny)
    assert mr.margin_floor.tolist() == floor[:2] + [0] + floor[3:]        # unnamed motifs keep the default
    assert motifs.MotifReward(tiny).hit_coef.tolist() == [0] * 6          # nothing given: the zero objective


def test_motif_reward_refuses(tiny):
    names = tiny.names
    with pytest.raises(ValueError, match="MotifSet"):
        motifs.MotifReward(tiny.pwm)
    with pytest.raises(ValueError, match="strands"):
        motifs.MotifReward(tiny, strands="reverse")
    for unit in (0, -1.0, float("inf"), float("nan"), True, "1", 0.1, 1e-60):   # 0.1 is not an fp32 number; 1e-60 underflows
        with pytest.raises(ValueError, match="unit"):
            motifs.MotifReward(tiny, unit=unit)
    with pytest.raises(ValueError, match="no motif named"):
        motifs.MotifReward(tiny, hit_weight={"HNF1A": 1.0})
    with pytest.raises(ValueError, match="hit_weight"):
        motifs.MotifReward(tiny, hit_weight=[1.0, 2.0])
    with pytest.raises(ValueError, match="margin_weight"):
        motifs.MotifReward(tiny, margin_weight={names[0]: float("nan")})
    with pytest.raises(ValueError, match="hit_cap"):
        motifs.MotifReward(tiny, hit_cap=-1)
    with pytest.raises(ValueError, match="hit_cap"):
        motifs.MotifReward(tiny, hit_cap=1.5)
    with pytest.raises(ValueError, match="margin_floor"):
        motifs.MotifReward(tiny, margin_floor={names[0]: -3})
    with pytest.raises(ValueError, match="int32"):
        motifs.MotifReward(tiny, hit_weight=3e6)                          # 3e6 * 1024 > 2^31
    # the int64 bound: sum |hit_coef| hit_cap + |margin_coef| margin_floor < 2^62
    big = (1 << 31) - 1
    ok = motifs.MotifReward(tiny, hit_weight={names[0]: float(big)}, hit_cap={names[0]: big}, unit=1.0)
    assert ok.bound == big * big < 1 << 62
    with pytest.raises(ValueError, match="2\\^62"):
        motifs.MotifReward(tiny, hit_weight=[float(big)] * 2 + [0.0] * 4, hit_cap=big, margin_weight={names[2]: -float(big)},
                           margin_floor=big, unit=1.0)
    with pytest.raises(ValueError, match="MotifReward"):
        motifs.GuidedReward(None, tiny)
    with pytest.raises(ValueError, match="callable"):
        motifs.GuidedReward(3.0, motifs.MotifReward(tiny))
    with pytest.raises(ValueError, match="already"):
        motifs.GuidedReward(motifs.GuidedReward(None, motifs.MotifReward(tiny)), motifs.MotifReward(tiny))


# ------------------------------------------------------------------------------------------------------ the entry ----
def test_reward_entry_refuses_bad_arguments_without_a_device():
    from svdd_amd import _lib
    L_ = _lib.lib()
    assert _lib.ABI_VERSION == 17 and L_.svdd_abi_version() == 17
    assert "svdd_motif_reward" in _lib.EXPORTS
    sig = _lib.SIGNATURES["svdd_motif_reward"]
    assert len(sig) == 19 and sig[-1] is _lib.vp and _lib.STREAM not in sig                       # the stream is the caller's
    assert sig[14] is _lib.f32 and [i for i, t in enumerate(sig) if t is _lib.i32] == [1, 2, 7, 8]
    p = [ctypes.c_void_p(4096 * (i + 1)) for i in range(13)]             # non-NULL pointers that are never dereferenced

    def reward(**kw):
        a = dict(tok=p[0], n=4, L=20, count=p[1], pwm=p[2], width=p[3], threshold=p[4], M=3, both=1, hit_coef=p[5], hit_cap=p[6],
                 margin_coef=p[7], margin_floor=p[8], base=p[9], unit=ctypes.c_float(0.5), score=p[10], term=p[11], err=p[12], stream=None)
        a.update(kw)
        return L_.svdd_motif_reward(*a.values())
    for what, kw in {"n = 0": dict(n=0), "n < 0": dict(n=-1), "L = 0": dict(L=0), "L < 0": dict(L=-3), "L = 1025": dict(L=1025),
                     "M = 0": dict(M=0), "M < 0": dict(M=-2), "tok null": dict(tok=None), "pwm null": dict(pwm=None),
                     "width null": dict(width=None), "threshold null": dict(threshold=None), "hit_coef null": dict(hit_coef=None),
                     "hit_cap null": dict(hit_cap=None), "margin_coef null": dict(margin_coef=None),
                     "margin_floor null": dict(margin_floor=None), "no output": dict(score=None, term=None),
                     "no output, forward, no count": dict(score=None, term=None, both=0, count=None, base=None, err=None)}.items():
        assert reward(**kw) == _lib.E_ARG, what


# ----------------------------------------------------------------------------------------------------- the python ----
def test_wrappers_refuse_bad_arguments_before_any_launch(tiny):
    from svdd_amd import ops
    mr = motifs.MotifReward(tiny, hit_weight=1.0)
    x = torch.randint(0, 4, (4, 20), generator=torch.Generator().manual_seed(0))
    bad = x.clone()
    bad[1, 3] = 4
    with pytest.raises(ValueError, match="token"):
        mr.term(bad)                                                       # MASK is not a finished sequence
    with pytest.raises(ValueError, match="integer"):
        mr.term(x.float())
    with pytest.raises(ValueError, match=r"\[N, L\]"):
        mr.term(x[0])
    with pytest.raises(ValueError, match="1024"):
        mr.term(torch.zeros(1, 1025, dtype=torch.uint8))
    for rows in (0, -4, 1.5):
        with pytest.raises(ValueError, match="chunk_rows"):
            mr.term(x, chunk_rows=rows)
    gr = motifs.GuidedReward(None, mr)
    with pytest.raises(ValueError, match="onehot"):
        gr(torch.zeros(4, 20))
    with pytest.raises(ValueError, match="onehot"):
        gr(torch.zeros(4, 20, 5))
    if not torch.cuda.is_available():
        with pytest.raises(ops.SvddError, match="GPU"):
            mr.term(x)                                                     # valid arguments: no CPU fallback
        with pytest.raises(ops.SvddError, match="GPU"):
            mr.to_device()
        with pytest.raises(ops.SvddError, match="GPU"):
            mr.term_tokens(x.to(torch.uint8))
        with pytest.raises(ops.SvddError, match="GPU"):
            gr(torch.nn.functional.one_hot(x, 4).float())
        with pytest.raises(ops.SvddError, match="GPU"):
            gr.forward_tokens(x.to(torch.uint8))
    # the raw wrapper takes device tensors only
    t = ops.MotifTables(torch.from_numpy(tiny.pwm), torch.from_numpy(tiny.width), torch.from_numpy(tiny.threshold))
    c = ops.MotifCoefs(*(torch.from_numpy(a) for a in (mr.hit_coef, mr.hit_cap, mr.margin_coef, mr.margin_floor)))
    tok = x.to(torch.uint8)
    with pytest.raises(ops.SvddError, match="GPU"):
        ops.motif_reward(tok, t, c, mr.unit)
    with pytest.raises(ops.SvddError, match="MotifTables"):
        ops.motif_reward(tok, tiny, c, mr.unit)
    with pytest.raises(ops.SvddError, match="MotifCoefs"):
        ops.motif_reward(tok, t, mr, mr.unit)
    for unit in (0.0, -1.0, float("nan"), torch.tensor(0.5), True):
        with pytest.raises(ops.SvddError, match="unit"):
            ops.motif_reward(tok, t, c, unit)


def test_gradient_samplers_refuse_a_guided_reward(tiny):
    """DPS, classifier guidance and the attributions differentiate their net: a GuidedReward raises a TypeError that says so, before
    anything is launched (here: on a machine without a GPU, before the GPU is asked for)."""
    from svdd_amd.config import rna_config
    from svdd_amd.diffusion import Diffusion
    d = Diffusion(rna_config(hidden_dim=16, num_cnn_stacks=1)).eval()
    gr = motifs.GuidedReward(None, motifs.MotifReward(tiny, hit_weight=1.0))
    x = torch.zeros(2, 50, dtype=torch.long)
    with pytest.raises(TypeError, match="not differentiable"):
        d.controlled_sample_DPS(gr, 1e5, num_steps=2, eval_sp_size=2)
    with pytest.raises(TypeError, match="not differentiable"):
        d.controlled_sample_classfier(gr, None, num_steps=2, eval_sp_size=2, guidance_scale=1.5)
    with pytest.raises(TypeError, match="not differentiable"):
        d.controlled_sample_classfier(None, gr, num_steps=2, eval_sp_size=2, guidance_scale=1.5)
    with pytest.raises(TypeError, match="not differentiable"):
        d.attributions(x, None, None, reward_model=gr)
    with pytest.raises(TypeError, match="not differentiable"):
        d.attributions(x, gr, None)
    # the wrapper is what reward_callable hands the loops, and a base of None qualifies for the skipping loop
    rc = d.reward_callable(gr)
    assert isinstance(rc, motifs.GuidedReward) and rc.reward_model is None and rc.motif_reward is gr.motif_reward
    d.fuse_nets = d.skip_unchanged = True
    assert d._can_skip(rc, 50, 4) and not d._can_skip(rc, 50, 1)
    assert not d._can_skip(motifs.GuidedReward(lambda oh: oh, gr.motif_reward), 50, 4)    # an opaque net takes no device-side count


def test_public_signatures_and_flags():
    from svdd_amd import cli, ops
    from svdd_amd.harness import BaseModel
    sig = lambda f: list(inspect.signature(f).parameters)                  # noqa: E731
    dflt = lambda f: {k: v.default for k, v in inspect.signature(f).parameters.items() if v.default is not inspect.Parameter.empty}   # noqa: E731
    assert sig(ops.motif_reward) == ["tok", "mset_dev", "coefs", "unit", "count", "base", "out", "term", "err", "both_strands"]
    assert dflt(ops.motif_reward) == dict(count=None, base=None, out=None, term=None, err=None, both_strands=True)
    assert sig(motifs.MotifReward.__init__) == ["self", "mset", "hit_weight", "margin_weight", "hit_cap", "margin_floor", "unit", "strands"]
    assert dflt(motifs.MotifReward.__init__) == dict(hit_weight=None, margin_weight=None, hit_cap=1, margin_floor=None, unit=2 ** -10,
                                                     strands="both")
    assert sig(motifs.MotifReward.term)[:2] == ["self", "x"]
    assert sig(motifs.MotifReward.term_tokens) == ["self", "tok", "count", "base", "out"]
    assert sig(motifs.GuidedReward.__init__) == ["self", "reward_model", "motif_reward"]
    assert sig(motifs.GuidedReward.forward_tokens) == ["self", "tok", "count"] and sig(motifs.GuidedReward.__call__) == ["self", "onehot"]
    assert sig(BaseModel.controlled_decode_motif) == ["self", "gen_batch_num", "sample_M", "motif_reward", "options"]
    assert dflt(BaseModel.controlled_decode_motif) == dict(options="True")
    # the flags: absent from the default namespace (which is what it was), present when given
    flags = ("guide_motifs", "guide_weights", "guide_margin")
    for method in cli.SUFFIX:
        ns = cli.build_parser(method).parse_args([])
        assert not any(hasattr(ns, f) for f in flags)
        assert sorted(vars(ns)) == sorted(["task", "reward_name", "batch_size", "sample_M", "val_batch_num", "seed", "method", "tweedie",
                                           "alpha", "guidance_scale", "model", "precision", "rng", "diffusion_ckpt",
                                           "load_checkpoint_path", "reward_ckpt", "out_dir", "eval_nll", "presample"])
    given = ["--guide_motifs", FIXTURE, "--guide_weights", "MT0002.1=+2,MT0005.1=-1", "--guide_margin", "MT0006.1=0.01"]
    ns = cli.build_parser("tweedie").parse_args(given)
    assert (ns.guide_motifs, ns.guide_weights, ns.guide_margin) == (FIXTURE, "MT0002.1=+2,MT0005.1=-1", "MT0006.1=0.01")
    mr = cli.guide_reward(ns)
    assert mr.hit_coef.tolist() == [0, 2048, 0, 0, -1024, 0] and mr.margin_coef.tolist() == [0, 0, 0, 0, 0, 10]
    assert cli.guide_reward(cli.build_parser("tweedie").parse_args([])) is None
    # refused for every other method, and when incomplete or malformed, before a model is built
    for method in ("mc", "tds", "dps", "classfier"):
        with pytest.raises(SystemExit):
            cli.main(method, given)
        with pytest.raises(ValueError, match="--method tweedie"):
            cli.run(cli.build_parser(method).parse_args(given))
        with pytest.raises(ValueError, match="--method tweedie"):
            cli.run(cli.build_parser(method).parse_args(given[2:4]))
    with pytest.raises(ValueError, match="needs --guide_motifs"):
        cli.run(cli.build_parser("tweedie").parse_args(given[2:]))
    with pytest.raises(ValueError, match="--guide_weights, --guide_margin or both"):
        cli.run(cli.build_parser("tweedie").parse_args(given[:2]))
    with pytest.raises(SystemExit):
        cli.main("tweedie", given[:2])
    for text in ("MT0002.1", "MT0002.1=two", "=3", " , "):
        with pytest.raises(ValueError, match="NAME=NUMBER"):
            cli.run(cli.build_parser("tweedie").parse_args(given[:2] + ["--guide_weights", text]))
    with pytest.raises(ValueError, match="no motif named"):
        cli.run(cli.build_parser("tweedie").parse_args(given[:2] + ["--guide_weights", "HNF1A=1"]))
