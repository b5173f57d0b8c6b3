"""Float64 restatements and shared set-up for the tests of the Enformer-shaped value trunk (svdd_amd/enformer_value.py,
svdd_amd/fused_trunk.py, csrc/svdd_trunk.hip). Not a test module: imported by the CPU and GPU trunk tests."""
import torch

from svdd_amd.enformer_value import _relative_shift


def randomise(emb, head, seed):
    """Non-trivial BatchNorm statistics, attention output projections (zero at init) and pooling logits."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    with torch.no_grad():
        for m in emb.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                m.weight.copy_(1.0 + 0.2 * torch.randn(m.num_features, generator=g))
                m.bias.copy_(0.1 * torch.randn(m.num_features, generator=g))
        for blk in emb.transformer_tower:
            w = blk.mha.to_out.weight
            w.copy_(torch.randn(w.shape, generator=g) * (w.shape[1] ** -0.5))
            blk.mha.to_out.bias.copy_(torch.randn(w.shape[0], generator=g) * 0.05)
        for blk in emb.conv_tower.blocks:
            pw = blk[1].pool.to_attn_logits.weight
            pw.add_((torch.randn(pw.shape, generator=g) * 0.05).to(pw.device))


def attn_small_ref(qkv, rel_k, content_bias, pos_bias, n, T, heads, dk, dv):
    """What svdd_trunk_attn_small computes, in the dtype of its inputs: qkv [n T, heads (2 dk + dv)] = [q | k | v], rel_k
    [heads, 2 T - 1, dk], biases [heads, dk] -> [n T, heads dv]. The relative shift is the module's own."""
    nq = heads * dk
    q = qkv[:, :nq].reshape(n, T, heads, dk).transpose(1, 2) * dk ** -0.5
    k = qkv[:, nq:2 * nq].reshape(n, T, heads, dk).transpose(1, 2)
    v = qkv[:, 2 * nq:].reshape(n, T, heads, dv).transpose(1, 2)
    cb, pb = content_bias.reshape(1, heads, 1, dk), pos_bias.reshape(1, heads, 1, dk)
    rel = _relative_shift(torch.einsum("bhid,hjd->bhij", q + pb, rel_k))
    logits = torch.matmul(q + cb, k.transpose(-1, -2)) + rel
    return torch.matmul(torch.softmax(logits, dim=-1), v).transpose(1, 2).reshape(n * T, heads * dv)


def gelu(x):
    return x * torch.sigmoid(1.702 * x)


def act(x, a):
    return x if a == 0 else torch.relu(x) if a == 1 else gelu(x)
