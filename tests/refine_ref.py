"""numpy restatements of the round boundary of re-mask refinement (svdd_refine_remask, include/svdd_hip.h): the accept rule, the
re-mask from given uniforms (q_xt, reference diffusion_gosai.py:738-749, under a frozen mask), the kernel's Philox counters, and
the schedule of a decode that starts at t_start (the fp32 torch restatement of :1036-1038, :1176-1187). Test infrastructure: lives
under tests/, not in the product package."""
import numpy as np

from tests.elbo_ref import philox4x32_10, u24

MASK = 4
REFINE_STREAM = 1            # counter word 3: 0 = propose / classifier, 2 = the multinomial select, 3 = ELBO, 1 = the refinement mask


def accept(x_new, x_old=None, score_new=None, score_old=None):
    """-> (x_keep u8 [B, L], score_keep f32 [B] | None, accepted i32 [B]). A row takes its new version iff score_new > score_old
    (a NaN and a tie keep the old row); with x_old, score_new or score_old missing nothing is judged and the new row is kept."""
    x_new = np.asarray(x_new, np.uint8)
    B = x_new.shape[0]
    if x_old is None or score_new is None or score_old is None:
        return x_new.copy(), None if score_new is None else np.asarray(score_new, np.float32).copy(), np.ones(B, np.int32)
    sn, so = np.asarray(score_new, np.float32), np.asarray(score_old, np.float32)
    with np.errstate(invalid="ignore"):
        take = sn > so
    return (np.where(take[:, None], x_new, np.asarray(x_old, np.uint8)).astype(np.uint8), np.where(take, sn, so).astype(np.float32),
            take.astype(np.int32))


def remask(x_keep, u, move_chance, frozen=None):
    """-> (x_t u8 [B, L], nmasked i32 [B]): MASK iff u < move_chance and the position is not frozen; a MASK token stays MASK.
    The compare is fp32 against fp32, as in the kernel. nmasked counts the MASK tokens of x_t."""
    x_keep = np.asarray(x_keep, np.uint8)
    hit = np.asarray(u, np.float32) < np.float32(move_chance)
    if frozen is not None:
        hit &= np.asarray(frozen) == 0
    x_t = np.where(hit | (x_keep == MASK), MASK, x_keep).astype(np.uint8)
    return x_t, (x_t == MASK).sum(1).astype(np.int32)


def philox_counters(row_offset, B, L, round):
    """The counter words (c0, c1, c2, c3) of the kernel's blocks: arrays [B, ceil(L / 4)]; block j feeds positions 4 j .. 4 j + 3."""
    nb = (L + 3) // 4
    grow = np.arange(B, dtype=np.uint64) + np.uint64(row_offset)
    j = np.arange(nb, dtype=np.uint64)
    c0 = np.broadcast_to((grow & np.uint64(0xFFFFFFFF))[:, None], (B, nb))
    c1 = np.broadcast_to((grow >> np.uint64(32))[:, None], (B, nb))
    c2 = np.broadcast_to(((np.uint64(round) << np.uint64(16)) | j)[None, :], (B, nb))
    return c0, c1, c2, np.full((B, nb), REFINE_STREAM, np.uint64)


def philox_uniforms(seed, row_offset, B, L, round):
    """The mask uniforms f32 [B, L] of rows row_offset .. row_offset + B - 1 in round `round`."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    words = philox4x32_10(*philox_counters(row_offset, B, L, round), seed & 0xFFFFFFFF, seed >> 32)
    return np.stack([u24(v) for v in words], axis=-1).reshape(B, -1)[:, :L]


def propose_counters(row_offset, B, L, step, m=0):
    """The counter words of svdd_propose's draw (row, position, step, m): arrays [B, L] (svdd_kernels.hip philox_uniform5)."""
    pos = (np.arange(B, dtype=np.uint64)[:, None] + np.uint64(row_offset)) * np.uint64(L) + np.arange(L, dtype=np.uint64)[None, :]
    c2 = np.full((B, L), ((int(step) << 16) | int(m)) & 0xFFFFFFFF, np.uint64)
    return pos & np.uint64(0xFFFFFFFF), pos >> np.uint64(32), c2, np.zeros((B, L), np.uint64)


def propose_uniforms(seed, row_offset, B, L, step, m=0):
    """The first four uniforms (categories 0..3) of each of svdd_propose's draws: f32 [B, L, 4]."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    words = philox4x32_10(*propose_counters(row_offset, B, L, step, m), seed & 0xFFFFFFFF, seed >> 32)
    return np.stack([u24(v) for v in words], axis=-1)


def boundary(x_new, u, move_chance, frozen=None, x_old=None, score_new=None, score_old=None):
    """The whole launch -> dict(x_keep, score_keep, accepted, x_t, nmasked, err)."""
    x_keep, score_keep, acc = accept(x_new, x_old, score_new, score_old)
    x_t, nm = remask(x_keep, u, move_chance, frozen)
    return dict(x_keep=x_keep, score_keep=score_keep, accepted=acc, x_t=x_t, nmasked=nm, err=int((x_keep > MASK).any()))


def schedule_torch(num_steps, eps, t_start, noise_eps=1e-3):
    """(mct, mcs, mct - mcs) fp32 [S, 3] of a decode over linspace(t_start, eps, S + 1): the reference's per-step scalars
    (:1176-1187 with noise_schedule.py:126-145) restated with fp32 torch ops."""
    import torch
    ts = torch.linspace(t_start, eps, num_steps + 1)
    dt = (t_start - eps) / num_steps
    t = ts[:num_steps].view(-1, 1)
    sigma_t = -torch.log1p(-(1 - noise_eps) * t)
    sigma_s = -torch.log1p(-(1 - noise_eps) * (t - dt))
    mct = 1 - torch.exp(-sigma_t.squeeze(-1))
    mcs = 1 - torch.exp(-sigma_s.squeeze(-1))
    return torch.stack([mct, mcs, mct - mcs], dim=1).numpy()
