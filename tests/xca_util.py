"""The plain-PyTorch cross-covariance attention (XCiT's XCA, the reference's models/xcit.py:243-254) that the XCA kernel
tests compare against, and the closed-form backward with the roundings the bf16 kernels declare.  Neither touches the
library nor the reference tree."""
from collections import namedtuple

import torch
import torch.nn.functional as F

from vit_attn_util import bf16, gen, normal_inputs, rel  # noqa: F401  (same metric and input style as the ViT attention tests)

XcaRef = namedtuple("XcaRef", "out stat dqkv dtemp")
XcaRef.__doc__ = """out [B,N,H*hd], stat [B,H,hd+2,hd] (Gh rows, r_q, r_k: the kernels' layout), dqkv [B,N,3,H,hd], dtemp [H]."""

EPS = 1e-12


def _stat(q, k):
    """[B,H,hd+2,hd] from q, k [B,H,hd,N] (channels x tokens)."""
    rq = q.norm(dim=-1).clamp_min(EPS)
    rk = k.norm(dim=-1).clamp_min(EPS)
    gh = (q @ k.transpose(-2, -1)) / (rq.unsqueeze(-1) * rk.unsqueeze(-2))
    return torch.cat((gh, rq.unsqueeze(-2), rk.unsqueeze(-2)), dim=-2)


def torch_xca(qkv, dO, temperature, B, N, H, hd, dtype=torch.float64):
    """The reference's lines under autograd in `dtype` on the CPU: qkv [B,N,3*H*hd], dO [B,N,H*hd], temperature [H]."""
    x = qkv.to(dtype).reshape(B, N, 3, H, hd).clone().requires_grad_(True)
    t = temperature.to(dtype).reshape(H, 1, 1).clone().requires_grad_(True)
    q, k, v = x.permute(2, 0, 3, 1, 4)
    q = q.transpose(-2, -1)
    k = k.transpose(-2, -1)
    v = v.transpose(-2, -1)
    qn = F.normalize(q, dim=-1)
    kn = F.normalize(k, dim=-1)
    attn = (qn @ kn.transpose(-2, -1)) * t
    attn = attn.softmax(dim=-1)
    o = (attn @ v).permute(0, 3, 1, 2).reshape(B, N, H * hd)
    o.backward(dO.to(dtype).reshape(B, N, H * hd))
    return XcaRef(o.detach(), _stat(q.detach(), k.detach()), x.grad, t.grad.reshape(H))


def emulated_xca(qkv, dO, temperature, B, N, H, hd, dtype=torch.float64, rounding=True):
    """The closed form in `dtype` with only the roundings the bf16 kernels declare: A -> bf16 before V A^T and dO A,
    M -> bf16 before the dQ and dK products, O, dQ, dK, dV -> bf16 on store.  stat and dtemp carry no rounding.  With
    rounding=False this is the closed-form gradient, equal to autograd."""
    r = bf16 if rounding else (lambda t: t)
    x = qkv.to(dtype).reshape(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)
    Q, K, V = x[0], x[1], x[2]                                   # [B,H,N,hd]
    dOh = dO.to(dtype).reshape(B, N, H, hd).permute(0, 2, 1, 3)  # [B,H,N,hd]
    tau = temperature.to(dtype).reshape(1, H, 1, 1)
    rq = Q.norm(dim=-2).clamp_min(EPS)                           # [B,H,hd]
    rk = K.norm(dim=-2).clamp_min(EPS)
    rr = rq.unsqueeze(-1) * rk.unsqueeze(-2)
    Gh = (Q.transpose(-2, -1) @ K) / rr
    A = (tau * Gh).softmax(-1)
    O = r(V @ r(A).transpose(-2, -1))
    dA = dOh.transpose(-2, -1) @ V
    dV = r(dOh @ r(A))
    dS = A * (dA - (A * dA).sum(-1, keepdim=True))
    dtemp = (dS * Gh).sum((0, 2, 3))
    dG = tau * dS
    c = (dG * Gh).sum(-1)
    e = (dG * Gh).sum(-2)
    M = dG / rr
    dQ = r(K @ r(M).transpose(-2, -1) - Q * (c / rq ** 2).unsqueeze(-2))
    dK = r(Q @ r(M) - K * (e / rk ** 2).unsqueeze(-2))
    out = O.permute(0, 2, 1, 3).reshape(B, N, H * hd)
    stat = torch.cat((Gh, rq.unsqueeze(-2), rk.unsqueeze(-2)), dim=-2)
    dqkv = torch.stack((dQ, dK, dV)).permute(1, 3, 0, 2, 4)
    return XcaRef(out, stat, dqkv, dtemp)


def xca_errors(got, want, grads=True):
    """rel-to-max errors of an XcaRef-like `got` against `want`: out, stat (Gh block and the two norm rows together with it
    would mix scales, so gh / rq / rk separately) and, with grads, dq, dk, dv, dtemp."""
    hd = want.stat.shape[-1]
    e = {"out": rel(got.out, want.out), "gh": rel(got.stat[..., :hd, :], want.stat[..., :hd, :]),
         "rq": rel(got.stat[..., hd, :], want.stat[..., hd, :]), "rk": rel(got.stat[..., hd + 1, :], want.stat[..., hd + 1, :])}
    if grads:
        for i, nm in enumerate("qkv"):
            e["d" + nm] = rel(got.dqkv[:, :, i], want.dqkv[:, :, i])
        e["dtemp"] = rel(got.dtemp, want.dtemp)
    return e


SWEEP_HD = (32, 48, 64)
# the issue's lengths, the neighbours of the kernels' steps (16-token product tiles, 32-token reduction steps, the
# 128-token streamed chunk, the 256-token resident limit of the backward) and the patch-8 / 384-pixel length
SWEEP_N = sorted({2, 3, 4, 5, 7, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 196, 255, 256, 257, 576, 784})
SWEEP_TEMPERATURE = (0.25, 1.0, 4.0)
LONG_CASE = (1, 2304, 2, 32)


def sweep_cases():
    """(B, N, H, hd, seed, temperature) of section 1."""
    cs = [(2, N, 3, hd, 1000 * hd + N, SWEEP_TEMPERATURE) for hd in SWEEP_HD for N in [1] + SWEEP_N]
    B, N, H, hd = LONG_CASE
    cs.append((B, N, H, hd, 1000 * hd + N, SWEEP_TEMPERATURE[:H]))
    return cs


PAIRS_CASE = (40, 196, 8, 48)
PAIRS_TEMPERATURE = (-2.0, 8.0, 1.0, 0.5, 1.0, 2.0, 4.0, 1.0)


# ------------------------------------------------------------------------------------------------ the module ---
MODULE_KEYS = ("temperature", "qkv.weight", "qkv.bias", "proj.weight", "proj.bias")


def module_ref(x, dy, state, heads, rounding=False, dtype=torch.float64):
    """The XCA module (qkv Linear, XCA, proj Linear) and its gradients in `dtype`: {"y", "dx", "grad/<key>"}.  With
    rounding, the bf16 mode's stage boundaries: x, the two weights, qkv, the attention output, dy and the gradient
    entering the op are rounded to bf16, and the op applies its declared roundings (emulated_xca)."""
    r = bf16 if rounding else (lambda t: t)
    B, N, C = x.shape
    hd = C // heads
    temp = state["temperature"].to(dtype).reshape(heads)
    Wq, bq = r(state["qkv.weight"].to(dtype)), state["qkv.bias"].to(dtype)
    Wp, bp = r(state["proj.weight"].to(dtype)), state["proj.bias"].to(dtype)
    xr = r(x.to(dtype).reshape(B * N, C))
    qkv = r(xr @ Wq.T + bq)
    d = r(dy.to(dtype).reshape(B * N, C))
    datt = r(d @ Wp)
    op = emulated_xca(qkv.reshape(B, N, 3 * C), datt.reshape(B, N, C), temp, B, N, heads, hd, dtype=dtype, rounding=rounding)
    att = op.out.reshape(B * N, C)
    dqkv = op.dqkv.reshape(B * N, 3 * C)
    return {"y": (att @ Wp.T + bp).reshape(B, N, C), "dx": (dqkv @ Wq).reshape(B, N, C),
            "grad/temperature": op.dtemp.reshape(heads, 1, 1), "grad/qkv.weight": dqkv.T @ xr, "grad/qkv.bias": dqkv.sum(0),
            "grad/proj.weight": d.T @ att, "grad/proj.bias": d.sum(0)}


def rel_fixture(got, want):
    """rel against a fixture entry: a whole tensor, or the sample and the row sums of a sampled one (fixture_codec)."""
    if hasattr(want, "sample"):
        g = got.detach().double().cpu()
        return max(rel(g.reshape(-1)[::want.stride], want.sample), rel(g.sum(-1), want.rows))
    return rel(got.detach().cpu(), want)
