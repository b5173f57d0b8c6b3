"""Plain restatements of gradient attributions (include/svdd_hip.h: svdd_attr_path / svdd_attr_fold), written from the
header's description. Nothing of svdd_amd is imported.

  path_ref / fold_ref   numpy, in the dtype of their inputs: on float32 arrays every operation rounds once, in the stated order, and
                        the result must equal the kernels' bit for bit; on float64 arrays they are the reference of a whole call
  quadrature_ref        Gauss-Legendre on [0, 1] in float64 (captum's default rule), rounded once to float32 on request
  attributions_ref      float64 attributions of any differentiable torch function, by torch autograd
"""
import numpy as np
import torch

GRADIENT, TIMES_INPUT = 0, 1
WAVE = 64


def onehot_ref(x, dtype=np.float32):
    """tokens [...] -> [..., 4]; a token > 3 (MASK, or anything above it) gives a zero row."""
    x = np.asarray(x)
    return (x[..., None] == np.arange(4)).astype(dtype)


def _base(baseline, B, L, dtype):
    if baseline is None:
        return np.zeros((B, L, 4), dtype)
    baseline = np.asarray(baseline, dtype)
    return np.broadcast_to(baseline, (B, L, 4)) if baseline.ndim == 2 else baseline


def path_ref(x, baseline, alpha, r0, n_rows, n_pad=0):
    """Rows r0 .. r0 + n_rows - 1 of the B * S (row, step) pairs, pair r = (b, k) = (r // S, r % S): base + alpha[k] * (onehot - base)
    as sub, mul, add; then n_pad copies of row 0. -> ([n_rows + n_pad, L, 4], err: a token > 4 was seen)."""
    x = np.asarray(x)
    alpha = np.asarray(alpha)
    dtype = alpha.dtype
    B, L = x.shape
    S = alpha.size
    assert 0 <= r0 and n_rows > 0 and r0 + n_rows <= B * S and n_pad >= 0
    base, oh = _base(baseline, B, L, dtype), onehot_ref(x, dtype)
    out = np.empty((n_rows + n_pad, L, 4), dtype)
    rows = set()
    for i in range(n_rows):
        b, k = divmod(r0 + i, S)
        rows.add(b)
        d = (oh[b] - base[b]).astype(dtype)
        m = (alpha[k] * d).astype(dtype)
        out[i] = (base[b] + m).astype(dtype)
    out[n_rows:] = out[0]
    if n_pad:
        rows.add(r0 // S)
    return out, int(any((x[b] > 4).any() for b in rows))


def rowsum_ref(attr_blc):
    """The kernel's row sum of attr [L, 4] (position-major): lane j adds its positions l = j, j + 64, ... (channels 0..3 inside a
    position) onto 0, then the 64 partial sums meet in an xor butterfly with offsets 32 .. 1."""
    dtype = attr_blc.dtype
    v = np.zeros(WAVE, dtype)
    for l in range(attr_blc.shape[0]):
        for c in range(4):
            v[l % WAVE] = v[l % WAVE] + attr_blc[l, c]
    lanes = np.arange(WAVE)
    off = WAVE // 2
    while off:
        v = (v + v[lanes ^ off]).astype(dtype)
        off //= 2
    return v[0]


def fold_ref(grad, scale, weight, x, baseline, r0, n_rows, mode, acc, attr, rowsum=None):
    """One pass folded in place: acc [B, L, 4], attr [B, 4, L], rowsum [B] | None (arrays of grad's dtype). grad [>= n_rows, L, 4]:
    rows beyond n_rows are not read."""
    x = np.asarray(x)
    weight = np.asarray(weight)
    dtype = grad.dtype
    B, L = x.shape
    S = weight.size
    assert 0 <= r0 and n_rows > 0 and r0 + n_rows <= B * S
    scale = dtype.type(scale)
    base, oh = _base(baseline, B, L, dtype), onehot_ref(x, dtype)
    for i in range(n_rows):
        b, k = divmod(r0 + i, S)
        a = np.zeros((L, 4), dtype) if k == 0 else acc[b]
        acc[b] = (a + (weight[k] * (scale * grad[i]).astype(dtype)).astype(dtype)).astype(dtype)
        if k == S - 1:
            fin = acc[b] if mode == GRADIENT else ((oh[b] - base[b]).astype(dtype) * acc[b]).astype(dtype)
            attr[b] = fin.T
            if rowsum is not None:
                rowsum[b] = rowsum_ref(fin)


def quadrature_ref(n_steps, dtype=np.float64):
    node, weight = np.polynomial.legendre.leggauss(int(n_steps))
    return ((1.0 + node) / 2.0).astype(dtype), (weight / 2.0).astype(dtype)


def attributions_ref(score_fn, x, method, baseline=None, quadrature=None, dtype=torch.float64):
    """Attributions of score_fn by torch autograd, in `dtype` (float64: the reference; float32: what sizes a bar). score_fn: a
    differentiable map from a `dtype` torch tensor [n, L, 4] to n scores (task 0 of [n, T, 1]). x [B, L] tokens (numpy), baseline
    None / [L, 4] / [B, L, 4], quadrature = (alphas, weights) for "integratedgradients".
    -> dict(attr [B, 4, L], and for integrated gradients score_x [B], score_base [B], delta [B]), numpy arrays of `dtype`."""
    x = np.asarray(x)
    B, L = x.shape
    npt = np.float64 if dtype == torch.float64 else np.float32
    oh = torch.from_numpy(onehot_ref(x, npt))
    base = torch.from_numpy(np.ascontiguousarray(_base(baseline, B, L, npt)))

    def grad_at(p):
        p = p.clone().requires_grad_(True)
        (g,) = torch.autograd.grad(score_fn(p).reshape(p.shape[0], -1)[:, 0].sum(), p)
        return g

    if method == "gradient":
        return {"attr": grad_at(oh).permute(0, 2, 1).numpy()}
    if method == "inputxgradient":
        return {"attr": ((oh - base) * grad_at(oh)).permute(0, 2, 1).numpy()}
    assert method == "integratedgradients"
    alphas, weights = quadrature
    a_t, w_t = (torch.from_numpy(np.asarray(v, npt)) for v in (alphas, weights))
    grads = grad_at((base[None] + a_t[:, None, None, None] * (oh - base)[None]).reshape(-1, L, 4)).reshape(-1, B, L, 4)   # all steps at once
    acc = torch.zeros_like(oh)
    for k in range(len(w_t)):
        acc = acc + w_t[k] * grads[k]
    attr = ((oh - base) * acc).permute(0, 2, 1).numpy()
    with torch.no_grad():
        sx, sb = (score_fn(t).reshape(B, -1)[:, 0].numpy() for t in (oh, base))
    return {"attr": attr, "score_x": sx, "score_base": sb, "delta": attr.reshape(B, -1).sum(1) - (sx - sb)}


# ------------------------------------------------------------------- inputs of the fused-route cases (shared by the CPU and GPU files)
# name -> (task of svdd_amd.synthetic.build, L, B, S): one gradient pass each (15 pairs padded to 16 rows; 8 pairs).
FUSED_CASES = {"rna": ("rna", 50, 3, 5), "dna": ("dna", 200, 2, 4)}
# Input seeds: the first of 0..9 whose pass keeps the float64 reference's tail-kink sequences within grad_ref.seq_cap
# (tests/test_attr_cpu.py checks the cap for these very inputs).
FUSED_SEED = {"rna": 0, "dna": 0}


def fused_inputs(name, seed=None):
    """-> (x u8 [B, L] with a MASK stretch in row 0, baseline f32 [L, 4] (non-zero), alphas f32 [S], weights f32 [S]: Gauss-Legendre)."""
    _, L, B, S = FUSED_CASES[name]
    rng = np.random.default_rng([17, L, B, S, FUSED_SEED[name] if seed is None else seed])
    x = rng.integers(0, 4, (B, L)).astype(np.uint8)
    x[0, L // 4: L // 4 + 5] = 4
    baseline = (0.25 + 0.05 * rng.standard_normal((L, 4))).astype(np.float32)
    alphas, weights = quadrature_ref(S, np.float32)
    return x, baseline, alphas, weights


def pass_rows(n):
    """The fused route's row count for a pass that holds all n pairs: the next power of two."""
    return 1 << (n - 1).bit_length()


def kink_steps(x, baseline, alphas, p64):
    """By the float64 reference alone: the interpolants of an integrated-gradients table (one pass, padded to pass_rows) that are
    tail-kink sequences of grad_ref (a tail pre-activation within 2e-6 of zero: an fp32 evaluation may take the ReLU on either side).
    p64: grad_ref.params_of(net) in float64. -> (number of such (row, step) pairs, the sorted steps k that have one in any row)."""
    from tests import grad_ref as R
    x = np.asarray(x)
    B, _ = x.shape
    al = np.asarray(alphas, np.float32)
    n = B * al.size
    xp = torch.from_numpy(path_ref(x, baseline, al, 0, n, pass_rows(n) - n)[0]).double()
    z = R.value_grad(xp, p64, [m.double() for m in R.free_masks(xp, p64)])["z"]
    pairs = R.tail_kink_seqs(z)[:n].nonzero().flatten().tolist()
    return len(pairs), sorted({r % al.size for r in pairs})


# (fixture, table) -> kink_steps of the recorded inputs on the seed-44 nets: (tail-kink interpolants, their steps). Written down so that
# the GPU file need not recompute them (3 s per table); tests/test_attr_cpu.py holds this table to kink_steps and to the cap.
FIXTURE_KINK_STEPS = {("g38_attr_tiny.npz", "zero"): (0, []), ("g38_attr_tiny.npz", "base"): (0, []),
                      ("g39_attr_full.npz", "zero"): (3, [24, 26, 40]), ("g39_attr_full.npz", "base"): (5, [2, 10, 11, 31, 40])}
