"""The plain-PyTorch multi-head attention that the ViT attention kernel tests compare against, and the same mathematics
with the roundings the bf16 kernels declare (the reference's own rounding floor).  Neither touches the library."""
from collections import namedtuple

import torch

AttentionRef = namedtuple("AttentionRef", "out lse dqkv")
AttentionRef.__doc__ = """out [B,N,H*hd], lse [B,H,N] (the kernels' layout), dqkv [B,N,3,H,hd]."""


def bf16(t):
    """Round to bf16 (nearest even), keeping the dtype."""
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


def _split(qkv, dO, b0, b1, N, H, hd, dtype):
    """q, k, v, dO of images b0..b1 as [nb, H, N, hd] in `dtype`."""
    x = qkv[b0:b1].to(dtype).reshape(b1 - b0, N, 3, H, hd).permute(2, 0, 3, 1, 4)
    return x[0], x[1], x[2], dO[b0:b1].to(dtype).reshape(b1 - b0, N, H, hd).permute(0, 2, 1, 3)


def torch_attention(qkv, dO, B, N, H, hd, scale, dtype=torch.float64, images_per_chunk=None):
    """softmax(scale * q k^T) v on qkv [B,N,3*H*hd] and its autograd gradient for dO [B,N,H*hd], in `dtype` on the
    CPU, `images_per_chunk` images at a time (images are independent).  Returns an AttentionRef."""
    step = images_per_chunk or B
    out = torch.empty((B, N, H * hd), dtype=dtype)
    lse = torch.empty((B, H, N), dtype=dtype)
    dqkv = torch.empty((B, N, 3, H, hd), dtype=dtype)
    for b0 in range(0, B, step):
        b1 = min(B, b0 + step)
        x = qkv[b0:b1].to(dtype).reshape(b1 - b0, N, 3, H, hd).clone().requires_grad_(True)
        q, k, v = x.permute(2, 0, 3, 1, 4)
        s = (q @ k.transpose(-2, -1)) * scale
        o = (s.softmax(-1) @ v).transpose(1, 2).reshape(b1 - b0, N, H * hd)
        o.backward(dO[b0:b1].to(dtype).reshape(b1 - b0, N, H * hd))
        out[b0:b1] = o.detach()
        lse[b0:b1] = s.detach().logsumexp(-1)
        dqkv[b0:b1] = x.grad
    return AttentionRef(out, lse, dqkv)


def emulated_attention(qkv, dO, B, N, H, hd, scale, dtype=torch.float64, images_per_chunk=None, rounding=True):
    """The same mathematics in `dtype` with only the roundings the bf16 kernels declare:
      forward   P~ = bf16(exp(s - rowmax)) feeds P~ V, the row sum l is taken from the unrounded exponentials,
                O = bf16(P~ V / l);
      backward  delta = rowsum(dO * O) from the rounded O; P = exp(s - lse), dS = P (dO V^T - delta) unrounded;
                dV = bf16(bf16(P)^T dO), dK = bf16(scale * bf16(dS)^T Q), dQ = bf16(scale * bf16(dS) K).
    lse carries no rounding.  With rounding=False this is the closed-form gradient, equal to autograd."""
    r = bf16 if rounding else (lambda t: t)
    step = images_per_chunk or B
    out = torch.empty((B, N, H * hd), dtype=dtype)
    lse = torch.empty((B, H, N), dtype=dtype)
    dqkv = torch.empty((B, N, 3, H, hd), dtype=dtype)
    for b0 in range(0, B, step):
        b1 = min(B, b0 + step)
        q, k, v, do = _split(qkv, dO, b0, b1, N, H, hd, dtype)
        s = (q @ k.transpose(-2, -1)) * scale
        m = s.amax(-1, keepdim=True)
        pu = (s - m).exp()
        l = pu.sum(-1, keepdim=True)
        o = r((r(pu) @ v) / l)
        ls = m + l.log()
        p = (s - ls).exp()
        delta = (do * o).sum(-1, keepdim=True)
        ds = p * (do @ v.transpose(-2, -1) - delta)
        dv = r(r(p).transpose(-2, -1) @ do)
        dk = r(scale * (r(ds).transpose(-2, -1) @ q))
        dq = r(scale * (r(ds) @ k))
        out[b0:b1] = o.permute(0, 2, 1, 3).reshape(b1 - b0, N, H * hd)
        lse[b0:b1] = ls.squeeze(-1)
        dqkv[b0:b1] = torch.stack((dq, dk, dv)).permute(1, 3, 0, 2, 4)
    return AttentionRef(out, lse, dqkv)


# ------------------------------------------------------------------------------------------------ inputs ---
def gen(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator("cpu").manual_seed(seed)) * scale


def normal_inputs(B, N, H, hd, seed):
    """bf16-rounded unit-normal qkv [B,N,3*H*hd] and dO [B,N,H*hd] (fp32 tensors holding bf16 values)."""
    return bf16(gen((B, N, 3 * H * hd), seed)), bf16(gen((B, N, H * hd), seed + 1))


def leak_inputs(B, N, H, hd, scale, seed, depth=9.0):
    """Inputs on which a zero-padded key (score 0) would dominate every softmax row: per head a fixed direction u
    with scale * |u|^2 = depth, q rows u + 0.1 noise, k rows -u + noise, v rows 1 + noise (unit-normal noise), so that
    every real score is about -depth.  bf16-rounded, like normal_inputs."""
    g = torch.Generator("cpu").manual_seed(seed)
    u = torch.randn((1, 1, 1, H, hd), generator=g)
    u = u / u.norm(dim=-1, keepdim=True) * (depth / scale) ** 0.5
    x = torch.randn((B, N, 3, H, hd), generator=g)
    x[:, :, 0] = u[:, :, 0] + 0.1 * x[:, :, 0]
    x[:, :, 1] = -u[:, :, 0] + x[:, :, 1]
    x[:, :, 2] = 1.0 + x[:, :, 2]
    return bf16(x.reshape(B, N, 3 * H * hd)), bf16(torch.randn((B, N, H * hd), generator=g))


def leaked_key_effect(qkv, B, N, H, hd, scale):
    """rel-to-max change of the float64 O when one extra all-zero key / value row joins every softmax."""
    x = qkv.double().reshape(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)
    q, k, v = x[0], x[1], x[2]
    z = torch.zeros((B, H, 1, hd), dtype=torch.float64)
    o = ((q @ k.transpose(-2, -1)) * scale).softmax(-1) @ v
    o1 = ((q @ torch.cat((k, z), 2).transpose(-2, -1)) * scale).softmax(-1) @ torch.cat((v, z), 2)
    return ((o1 - o).abs().max() / o.abs().max()).item()


def pair_scales(B, H):
    """2^k per (image, head) pair, k cycling through -3 .. 3 over the pair index b * H + h (period 7)."""
    return torch.pow(2.0, ((torch.arange(B * H) % 7) - 3).float()).view(B, 1, H, 1)


def pair_scaled_inputs(B, N, H, hd, seed):
    """normal_inputs with v and dO of pair (b, h) multiplied by pair_scales (powers of two: exact in bf16)."""
    qkv, do = normal_inputs(B, N, H, hd, seed)
    sc = pair_scales(B, H)
    x = qkv.view(B, N, 3, H, hd)
    x[:, :, 2] *= sc
    return qkv, (do.view(B, N, H, hd) * sc).reshape(B, N, H * hd)


# ----------------------------------------------------------------------------------------------- metrics ---
def rel(got, want, denom=None):
    """max |got - want| / max |want| in float64 (`denom`, if given, replaces max |want|; 1 if that is zero)."""
    d = want.abs().max().item() if denom is None else denom
    return (got.double() - want.double()).abs().max().item() / (d if d > 0 else 1.0)


def grad_denoms(dqkv):
    """max |dq|, |dk|, |dv| of a reference dqkv [B,N,3,H,hd]; a gradient that is identically zero (dq and dk at
    N = 1: one key, dS = 0) is measured against max |dv| instead."""
    d = [dqkv[:, :, i].abs().max().item() for i in range(3)]
    return [x if x > 0 else d[2] for x in d]


def bias_sums(dqkv):
    """per-image column sums [B,3,H,hd] of dqkv [B,N,3,H,hd]: the qkv-bias gradient pieces."""
    return dqkv.double().sum(1)


def per_pair_rel(got, want):
    """[B,H] rel-to-max error within each (image, head) block of [B,N,H,hd] tensors."""
    g, w = got.double(), want.double()
    return (g - w).abs().amax((1, 3)) / w.abs().amax((1, 3))


def errors(got, want):
    """dict of the rel-to-max errors of an AttentionRef-like `got` against `want`: out, lse, dq, dk, dv and the
    per-image bias sums bq, bk, bv (bk, whose reference is rounding noise around zero, relative to max |bq ref|)."""
    e = {"out": rel(got.out, want.out), "lse": rel(got.lse, want.lse)}
    den = grad_denoms(want.dqkv)
    for i, nm in enumerate("qkv"):
        e["d" + nm] = rel(got.dqkv[:, :, i], want.dqkv[:, :, i], den[i])
    bg, bw = bias_sums(got.dqkv), bias_sums(want.dqkv)
    qden = bw[:, 0].abs().max().item() or bw[:, 2].abs().max().item()
    e["bq"] = rel(bg[:, 0], bw[:, 0], qden)
    e["bk"] = rel(bg[:, 1], bw[:, 1], qden)
    e["bv"] = rel(bg[:, 2], bw[:, 2])
    return e


# --------------------------------------------------------------------------------------------- the cases ---
def sweep_ns(any_n):
    """Section 1's sequence lengths: 1..40, 47, 49, each multiple of 32 up to 256 with its two neighbours, the ViT
    lengths, and for the paths that take any N the streamed lengths."""
    ns = set(range(1, 41)) | {47, 49, 100, 145, 196, 197, 224}
    for m in range(32, 257, 32):
        ns |= {m - 1, m, m + 1}
    ns = {n for n in ns if n <= 256}
    if any_n:
        ns |= {257, 288, 289, 300, 384, 385, 512, 513, 577, 785, 1025}
    return sorted(ns)


LEAK_NS = [1, 5, 31, 33, 145, 197, 225, 255]
LEAK_NS_STREAM = [257, 385, 577]
