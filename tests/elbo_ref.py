"""Float64 / numpy restatements of the ELBO scoring path (reference diffusion_gosai.py:1660-1669 _sample_t, :738-749 q_xt,
:1709-1757 _forward_pass_diffusion, :1759-1779 _loss, :50-71 metrics; noise_schedule.py:126-145 LogLinear) and of the Philox
stream of svdd_elbo_mask (include/svdd_hip.h). Test infrastructure: lives under tests/, not in the product package."""
import numpy as np

MASK = 4
NEG_INF = -1000000.0
ELBO_STREAM = 3


# ------------------------------------------------------------------------------------ steps 1-5 in float64
def scalars64(e, eps=1e-3, antithetic=True):
    """Step 1-2 from the uniforms e [n] of torch.rand(n): (t, sigma, dsigma, move_chance, w) in float64."""
    e = np.asarray(e, np.float64)
    n = e.shape[0]
    if antithetic:
        e = np.mod(e / n + np.arange(n) / n, 1.0)
    t = (1 - eps) * e + eps
    sigma = -np.log1p(-(1 - eps) * t)
    dsigma = (1 - eps) / (1 - (1 - eps) * t)
    mc = 1 - np.exp(-sigma)
    return t, sigma, dsigma, mc, dsigma / np.expm1(sigma)


def mask(x0, u, mc):
    """Step 3: xt = MASK where u < move_chance of the row, else x0."""
    return np.where(np.asarray(u) < np.asarray(mc).reshape(-1, 1), MASK, np.asarray(x0)).astype(np.uint8)


def subs_logp64(logits, xt):
    """Diffusion._subs_parameterization (diffusion_gosai.py:286-304) in float64: logits [n, L, 5] -> log p [n, L, 5]."""
    z = np.asarray(logits, np.float64).copy()
    z[..., MASK] += NEG_INF
    mx = z.max(-1, keepdims=True)
    lp = z - (np.log(np.exp(z - mx).sum(-1, keepdims=True)) + mx)
    xt = np.asarray(xt)
    un = xt != MASK
    fixed = np.full(z.shape, NEG_INF)
    np.put_along_axis(fixed, np.minimum(xt, 3)[..., None].astype(np.int64), 0.0, axis=-1)
    return np.where(un[..., None], fixed, lp)


def token_nll64(logits, xt, x0, w):
    """Step 4: -log p(x0 | xt) * w per token [n, L] (0 where xt is unmasked: SUBS gives log p = 0 there)."""
    lp = subs_logp64(logits, xt)
    lx = np.take_along_axis(lp, np.asarray(x0, np.int64)[..., None], axis=-1)[..., 0]
    return -lx * np.asarray(w, np.float64).reshape(-1, 1)


def loss64(nlls):
    """Step 5 with an all-ones attention mask: sum / count."""
    return float(np.sum(nlls, dtype=np.float64) / np.asarray(nlls).size)


def metrics64(token_nlls):
    nll = float(np.sum(token_nlls, dtype=np.float64) / np.asarray(token_nlls).size)
    return {"nll": nll, "bpd": nll / np.log(2.0), "ppl": float(np.exp(nll))}


# ------------------------------------------------------------------------------------ replayed draws against a recorded run
def check_replayed_draw(rec, call, e, u, t, mc, w, xt):
    """A replay-mode draw (t, move_chance, w fp32 [n], xt [n, L]; e, u: the replayed torch.rand(n), torch.rand(n, L)) against the
    reference's recorded call `call` of fixture case `rec`. t is pure fp32 arithmetic: bit for bit on any host. move_chance and w go
    through torch's CPU exp / log1p / expm1, whose vectorised code differs between CPU generations by an ulp: they must be bit for bit
    the reference's fp32 ops evaluated on THIS host (restated with torch below), and within one ulp of exp (2^-24 absolute on
    move_chance, 4 ulp relative on w) of the recorded run. xt must be the mask rule on this host's move_chance; a position may differ
    from the recorded xt only where u lies between the two move_chance values."""
    import torch
    assert np.array_equal(np.asarray(t, np.float32).view(np.uint32), rec["t"][call].view(np.uint32)), "t"
    n = e.shape[0]
    ee = torch.from_numpy(np.asarray(e, np.float32))
    ee = (ee / n + torch.arange(n) / n) % 1
    tt = (1 - 1e-3) * ee + 1e-3
    sigma = -torch.log1p(-(1 - 1e-3) * tt)
    dsigma = (1 - 1e-3) / (1 - (1 - 1e-3) * tt)
    mc_host = (1 - torch.exp(-sigma[:, None])).numpy().reshape(-1)
    w_host = (dsigma / torch.expm1(sigma)).numpy()
    assert np.array_equal(np.asarray(mc, np.float32).view(np.uint32), mc_host.view(np.uint32)), "move_chance (this host's torch ops)"
    assert np.array_equal(np.asarray(w, np.float32).view(np.uint32), w_host.view(np.uint32)), "w (this host's torch ops)"
    mc_rec = rec["move_chance"][call]
    assert np.abs(mc_host.astype(np.float64) - mc_rec).max() <= 2.0 ** -24, "move_chance vs the recorded run"
    assert np.abs(w_host.astype(np.float64) / rec["w"][call] - 1).max() <= 4 * 2.0 ** -23, "w vs the recorded run"
    u = np.asarray(u)
    assert np.array_equal(np.asarray(xt), mask(rec["x0"], u, mc_host)), "xt (mask rule)"
    lo, hi = np.minimum(mc_host, mc_rec)[:, None], np.maximum(mc_host, mc_rec)[:, None]
    differs = np.asarray(xt) != rec["xt"][call]
    assert np.all((u[differs] >= np.broadcast_to(lo, u.shape)[differs]) & (u[differs] < np.broadcast_to(hi, u.shape)[differs])), "xt"
    return int(differs.sum()), int((mc_host != mc_rec).sum())


# ------------------------------------------------------------------------------------ Philox4x32-10
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Vectorised Philox4x32-10 (the kernels' philox4x32_10): uint32 arrays in, four uint32 arrays out."""
    M = np.uint64(0xFFFFFFFF)
    c = [np.asarray(v, np.uint64) & M for v in (c0, c1, c2, c3)]
    k0, k1 = np.uint64(k0) & M, np.uint64(k1) & M
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k0) & M, p1 & M, ((p0 >> np.uint64(32)) ^ c[3] ^ k1) & M, p0 & M]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M, (k1 + np.uint64(0xBB67AE85)) & M
    return [v.astype(np.uint32) for v in c]


def u24(r):
    return ((np.asarray(r, np.uint32) >> np.uint32(8)).astype(np.float64) / 16777216.0).astype(np.float32)


def philox_elbo(seed, row_offset, n, L, K, eps=1e-3):
    """svdd_elbo_mask's Philox draws for rows r = k n + b: (t, move_chance, w) f32 [n K] and the mask uniforms f32 [n K, L]."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    k = np.repeat(np.arange(K, dtype=np.uint64), n)
    grow = np.tile(np.arange(n, dtype=np.uint64), K) + np.uint64(row_offset)
    lo, hi = grow & np.uint64(0xFFFFFFFF), grow >> np.uint64(32)
    w0 = philox4x32_10(lo, hi, k << np.uint64(16), np.full(n * K, ELBO_STREAM), k0, k1)[0]
    e = u24(w0).astype(np.float64) / K + k.astype(np.float64) / K
    e = np.where(e >= 1.0, e - 1.0, e)
    t = ((1.0 - eps) * e + eps).astype(np.float32)
    mc = ((1.0 - eps) * t.astype(np.float64)).astype(np.float32)
    w = (1.0 / t.astype(np.float64)).astype(np.float32)
    nb = (L + 3) // 4
    j = np.arange(1, nb + 1, dtype=np.uint64)
    words = philox4x32_10(lo[:, None], hi[:, None], (k << np.uint64(16))[:, None] | j[None, :], np.full((n * K, nb), ELBO_STREAM),
                          k0, k1)
    u = np.stack([u24(v) for v in words], axis=-1).reshape(n * K, 4 * nb)[:, :L]
    return t, mc, w, u
