"""Inputs and the fp64 reference of the attention-core tests (tests/test_attention_gpu.py at D = 64,
tests/test_attn_dims_gpu.py at D = 32 and 128).  No product imports."""
import math

import torch
import torch.nn.functional as F


def is_mfma(B, Nq, H):
    """Which kernel launch_attention picks (kernels_attn.hip): the matrix cores from Nq >= 128 and at least 16 blocks of 128
    queries, else the vector kernel."""
    return Nq >= 128 and ((Nq + 127) // 128) * H * B >= 16


def rel(a, b):
    return float((a.double() - b).norm() / b.norm().clamp(min=1e-300))


def inputs(D, family, B, Nq, H, Hkv, null, n0, n1, seed, marker=None):
    """fp32 CPU tensors q [B,Nq,H,D], null_kv [2,D] | None, k0 / v0 [B,n0,Hkv,D], k1 / v1 [B,n1,Hkv,D] and the scale.
    marker: index into the key list cat(null, seg0, seg1) of the key that gets the large logit."""
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen)
    q = rn(B, Nq, H, D) * 0.5
    nkv = rn(2, D) if null else None
    k0, v0, k1, v1 = rn(B, n0, Hkv, D), rn(B, n0, Hkv, D), rn(B, n1, Hkv, D), rn(B, n1, Hkv, D)
    Nk = int(null) + n0 + n1
    scale = D ** -0.5
    if family == "plain":
        pass
    elif family == "cos16":   # attn_qk_norm = 1: unit q and k, logits in [-16, 16]
        q, k0, k1 = F.normalize(q, dim=-1), F.normalize(k0, dim=-1), F.normalize(k1, dim=-1)
        if null:
            nkv[0] = F.normalize(nkv[0], dim=-1)
        scale = 16.0
    elif family == "ascending":   # key norms rise along the key list: the running maximum moves in every tile
        f = lambda j: 0.5 + 3.5 * j / max(Nk - 1, 1)
        if null:
            nkv[0] *= f(0)
        k0 *= f(int(null) + torch.arange(n0, dtype=torch.float32))[None, :, None, None]
        k1 *= f(int(null) + n0 + torch.arange(n1, dtype=torch.float32))[None, :, None, None]
    elif family == "marker":
        # every query has 2 u in it, the marked key is c u: its logit is c scale (2 +- noise) = ln(Nk) + 1 (+- 15 %), so the key
        # holds about e / (1 + e) of the softmax whatever Nk; its value row is unlike any other and differs in every column
        u = F.normalize(rn(D), dim=-1)
        q = rn(B, Nq, H, D) * (0.3 * 8 * scale) + 2 * u
        c = (math.log(Nk) + 1) / (2 * scale)
        vm = 3 + torch.arange(D, dtype=torch.float32) / 16
        j = marker
        if null and j == 0:
            nkv[0], nkv[1] = c * u, vm
        elif j < int(null) + n0:
            k0[:, j - int(null)], v0[:, j - int(null)] = c * u, vm
        else:
            k1[:, j - int(null) - n0], v1[:, j - int(null) - n0] = c * u, vm
    else:
        raise ValueError(family)
    return q, nkv, k0, v0, k1, v1, scale


def reference(q, nkv, k0, v0, k1, v1, scale, dtype=torch.float64):
    """softmax(scale q k^T) v over cat(null, seg0, seg1) in `dtype`, K / V expanded over the heads; one head at a time."""
    B, Nq, H, D = q.shape
    ks, vs = [], []
    if nkv is not None:
        ks.append(nkv[0].expand(B, 1, H, D))
        vs.append(nkv[1].expand(B, 1, H, D))
    for k, v in ((k0, v0), (k1, v1)):
        if k.shape[1]:
            ks.append(k.expand(B, k.shape[1], H, D))
            vs.append(v.expand(B, v.shape[1], H, D))
    K, V = torch.cat(ks, dim=1).to(dtype), torch.cat(vs, dim=1).to(dtype)
    out = torch.empty(B, Nq, H, D, dtype=dtype)
    for h in range(H):
        sim = torch.einsum("bid,bjd->bij", q[:, :, h].to(dtype), K[:, :, h]) * scale
        out[:, :, h] = torch.einsum("bij,bjd->bid", sim.softmax(dim=-1), V[:, :, h])
    return out
