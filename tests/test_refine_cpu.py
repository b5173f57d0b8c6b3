"""CPU tests of template-constrained design / re-mask refinement: the t_start schedule, the numpy restatement's own properties
(tests/refine_ref.py) and the refusals that need no GPU."""
import inspect

import numpy as np
import pytest
import torch

from tests import refine_ref as RR


def _todays_table(noise, num_steps, eps=1e-5):
    """move_chance_table as it stood before t_start existed, verbatim."""
    timesteps = torch.linspace(1, eps, num_steps + 1)
    dt = (1 - eps) / num_steps
    t = timesteps[:num_steps].view(-1, 1)
    sigma_t, _ = noise(t)
    sigma_s, _ = noise(t - dt)
    mct = 1 - torch.exp(-sigma_t.squeeze(-1))
    mcs = 1 - torch.exp(-sigma_s.squeeze(-1))
    return torch.stack([mct, mcs, mct - mcs], dim=1), timesteps, dt


def test_schedule_t_start_one_is_todays_table_byte_for_byte(golden):
    from svdd_amd.noise_schedule import LogLinearNoise, move_chance_table
    noise = LogLinearNoise()
    for S in (128, 39, 16, 8, 1):
        for eps in (1e-5, 1e-3):
            want, ts_w, dt_w = _todays_table(noise, S, eps)
            for got, ts, dt in (move_chance_table(noise, S, eps), move_chance_table(noise, S, eps, t_start=1.0),
                                move_chance_table(noise, S, eps, 1.0)):
                assert got.numpy().tobytes() == want.numpy().tobytes() and ts.numpy().tobytes() == ts_w.numpy().tobytes()
                assert dt == dt_w
    g = golden("g3_schedule.npz")                  # ... and still the reference's recorded one
    tab, ts, _ = move_chance_table(noise, 16, t_start=1.0)
    assert np.abs(tab.numpy() - g["S16"][:, 3:6]).max() <= 6e-8 and np.array_equal(ts[:16].numpy(), g["S16"][:, 0])


@pytest.mark.parametrize("t_start,S", [(0.3, 39), (0.3, 8), (0.5, 1), (0.05, 7)])
def test_schedule_from_t_start_equals_the_fp32_torch_restatement(t_start, S):
    from svdd_amd.noise_schedule import LogLinearNoise, move_chance_table
    eps = 1e-5
    tab, ts, dt = move_chance_table(LogLinearNoise(), S, eps, t_start=t_start)
    assert tab.numpy().tobytes() == RR.schedule_torch(S, eps, t_start).tobytes()
    assert ts.numpy().tobytes() == torch.linspace(t_start, eps, S + 1).numpy().tobytes() and dt == (t_start - eps) / S
    t = tab.numpy()
    assert np.all(t[:, 0] > t[:, 1]) and np.all(t[:, 1] >= 0) and abs(float(t[0, 0]) - (1 - 1e-3) * t_start) < 1e-6
    assert np.allclose(t[1:, 0], t[:-1, 1], atol=2e-7)            # the move chance a step ends on is the one the next starts from


def test_diffusion_schedule_cache_is_keyed_by_t_start():
    from svdd_amd.config import dna_config
    from svdd_amd.diffusion import Diffusion
    d = Diffusion(dna_config(hidden_dim=16, num_cnn_stacks=1))
    full, _, _ = d._schedule(8, 1e-5)
    part, _, _ = d._schedule(8, 1e-5, 0.3)
    assert full.tobytes() == d._schedule(8, 1e-5, 1.0)[0].tobytes() and full.tobytes() != part.tobytes()
    assert part.tobytes() == RR.schedule_torch(8, 1e-5, 0.3).tobytes()
    assert (8, 1e-5, 1.0) in d._sched_cache and (8, 1e-5, 0.3) in d._sched_cache
    assert abs(d._move_chance(0.3) - float(part[0, 0])) == 0.0    # renoise's scalar is the first step's move chance, same fp32 ops


def _case(B=7, L=37, seed=0):
    rng = np.random.default_rng(seed)
    x_new = rng.integers(0, 4, (B, L)).astype(np.uint8)
    x_old = rng.integers(0, 4, (B, L)).astype(np.uint8)
    u = rng.random((B, L), dtype=np.float32)
    frozen = (rng.random((B, L)) < 0.4).astype(np.uint8)
    return x_new, x_old, u, frozen


def test_ref_frozen_positions_are_never_masked():
    x_new, _, u, frozen = _case()
    for mc in (0.0, 0.3, 1.0):
        x_t, nm = RR.remask(x_new, u, mc, frozen)
        assert np.array_equal(x_t[frozen != 0], x_new[frozen != 0])
        assert np.array_equal(nm, (x_t == RR.MASK).sum(1))
    assert np.array_equal(RR.remask(x_new, u, 1.0, np.ones_like(frozen))[0], x_new)


def test_ref_move_chance_zero_masks_nothing_and_one_masks_every_open_position():
    x_new, _, u, frozen = _case()
    x_t, nm = RR.remask(x_new, u, 0.0, frozen)
    assert np.array_equal(x_t, x_new) and not nm.any()
    x_t, nm = RR.remask(x_new, u, 1.0, frozen)
    assert np.all(x_t[frozen == 0] == RR.MASK) and np.array_equal(nm, (frozen == 0).sum(1))
    x_t, nm = RR.remask(x_new, u, 1.0)
    assert np.all(x_t == RR.MASK) and np.all(nm == x_new.shape[1])
    # a MASK token of the input stays MASK, frozen or not, and is counted
    x_in = x_new.copy()
    x_in[:, 0] = RR.MASK
    fz = frozen.copy()
    fz[:, 0] = 1
    x_t, nm = RR.remask(x_in, u, 0.0, fz)
    assert np.all(x_t[:, 0] == RR.MASK) and np.all(nm == 1)
    # the compare is strict and in fp32
    assert RR.remask(np.zeros((1, 2), np.uint8), np.array([[0.25, np.nextafter(np.float32(0.25), np.float32(0))]], np.float32), 0.25)[0].tolist() == [[0, 4]]


def test_ref_ties_and_nan_keep_the_old_row():
    x_new, x_old, _, _ = _case(B=7)
    sn = np.array([1.0, 1.0, np.nan, 2.0, -np.inf, np.inf, 0.5], np.float32)
    so = np.array([1.0, 0.5, 0.0, np.nan, -np.inf, 1e30, np.inf], np.float32)
    x_keep, sk, acc = RR.accept(x_new, x_old, sn, so)
    assert acc.tolist() == [0, 1, 0, 0, 0, 1, 0]
    for b, a in enumerate(acc):
        assert np.array_equal(x_keep[b], x_new[b] if a else x_old[b])
        assert sk[b].tobytes() == (sn[b] if a else so[b]).tobytes()
    # nothing judged: the new row is kept
    for kw in (dict(), dict(x_old=x_old), dict(x_old=x_old, score_old=so), dict(score_new=sn, score_old=so)):
        x_keep, sk, acc = RR.accept(x_new, **kw)
        assert np.array_equal(x_keep, x_new) and acc.all()
    assert RR.boundary(np.full((1, 3), 5, np.uint8), np.ones((1, 3), np.float32), 0.5)["err"] == 1


def test_ref_philox_stream_is_its_own():
    """The mask's counters share no (c0, c1, c2, c3) with svdd_propose's (word 3: 1 against 0), differ between rounds, and a row's
    uniforms depend on its global index only."""
    B, L, seed = 5, 50, 1234
    mine = set(zip(*[np.asarray(c).reshape(-1).tolist() for c in RR.philox_counters(3, B, L, 2)]))
    for step in (0, 2):
        for m in (0, 1):
            theirs = set(zip(*[np.asarray(c).reshape(-1).tolist() for c in RR.propose_counters(3, B, L, step, m)]))
            assert not mine & theirs
    assert {c[3] for c in mine} == {RR.REFINE_STREAM} and RR.REFINE_STREAM not in (0, 2, 3)
    u0, u1 = RR.philox_uniforms(seed, 0, B, L, 0), RR.philox_uniforms(seed, 0, B, L, 1)
    assert u0.shape == (B, L) and u0.dtype == np.float32 and np.all((u0 >= 0) & (u0 < 1)) and (u0 != u1).mean() > 0.99
    assert np.array_equal(RR.philox_uniforms(seed, 3, 2, L, 0), u0[3:5])
    assert np.array_equal(RR.philox_uniforms(seed, 0, B, 7, 0), u0[:, :7])           # a block tail is the same block, cut
    assert (RR.philox_uniforms(seed, 0, B, L, 0)[:, :, None] != RR.propose_uniforms(seed, 0, B, L, 0)).all(-1).mean() > 0.99


def test_new_sampler_api_surface():
    from svdd_amd.config import dna_config
    from svdd_amd.diffusion import Diffusion
    from svdd_amd.harness import BaseModel
    d = Diffusion(dna_config(hidden_dim=16, num_cnn_stacks=1))
    want = {
        "decode_sample_from": ["x_init", "t_start", "num_steps", "eps"],
        "controlled_sample_from": ["x_init", "pre_scorer_embedding", "pre_scorer_head", "t_start", "num_steps", "eps", "sample_M"],
        "renoise": ["x0", "t", "frozen", "round"],
        "refine": ["x0", "pre_scorer_embedding", "pre_scorer_head", "rounds", "t_renoise", "num_steps", "eps", "sample_M", "frozen",
                   "accept", "reward_model"],
    }
    for name, params in want.items():
        assert list(inspect.signature(getattr(d, name)).parameters) == params, name
    p = inspect.signature(d.controlled_sample_from).parameters
    assert (p["t_start"].default, p["num_steps"].default, p["eps"].default, p["sample_M"].default) == (1.0, None, 1e-5, 10)
    assert inspect.signature(d.refine).parameters["accept"].default == "improve"
    assert list(inspect.signature(BaseModel.controlled_decode_refine).parameters) == ["self", "gen_batch_num", "sample_M", "rounds",
                                                                                       "t_renoise", "frozen"]


def test_from_state_entry_points_refuse_the_cpu():
    from svdd_amd import ops
    from svdd_amd.config import rna_config
    from svdd_amd.diffusion import Diffusion
    d = Diffusion(rna_config(hidden_dim=16, num_cnn_stacks=1)).eval()
    x = torch.zeros((2, d.config.model.length), dtype=torch.uint8)
    for call in (lambda: d.decode_sample_from(x), lambda: d.controlled_sample_from(x, lambda v: v, lambda v: v, sample_M=2),
                 lambda: d.renoise(x, 0.3), lambda: d.refine(x, lambda v: v, lambda v: v, 1, 0.3)):
        with pytest.raises(ops.SvddError):
            call()
    with pytest.raises(ops.SvddError):
        ops.refine_remask(x, 0.3, ops.Rng())
