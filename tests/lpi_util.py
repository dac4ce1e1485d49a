"""The plain-PyTorch local patch interaction (XCiT's LPI, the reference's models/xcit.py:132-141) that the LPI kernel tests
compare against, and the closed form with the roundings the bf16 kernels declare.  Neither touches the library nor the
reference tree.

The op DEFINES its batch statistics, its eval path and its backward over u = gelu(conv1(x)) as stored in the compute dtype:
the stored u is an operand of everything after it.  So "the same rounded operands" are x, dy and, in bf16, that stored u:
torch_lpi(..., u_stored=t) gives every line after the GELU the values t (the op's own stored tensor, or the emulation's)
with a straight-through gradient; gelu' is still taken at the unrounded conv output, which the kernels recompute from x.
The u it returns is always the unrounded gelu(conv1(x)), which the stored tensor is checked against.  With u_stored=None
it is the reference's lines verbatim."""
from collections import namedtuple

import torch
import torch.nn.functional as F

from vit_attn_util import bf16, gen, rel  # noqa: F401  (same metric and input style as the ViT attention tests)

GRAD_KEYS = ("conv1.weight", "conv1.bias", "bn.weight", "bn.bias", "conv2.weight", "conv2.bias")
BUF_KEYS = ("bn.running_mean", "bn.running_var", "bn.num_batches_tracked")
STATE_KEYS = GRAD_KEYS[:4] + BUF_KEYS + GRAD_KEYS[4:]
MOMENTUM, EPS = 0.1, 1e-5

LpiRef = namedtuple("LpiRef", "out u mean rstd dx grads running_mean running_var")
LpiRef.__doc__ = """out, u, dx [B,H*W,C]; mean, rstd [C] (the kernels' stat rows); grads {key: tensor} in the parameters'
shapes; running_mean / running_var after the forward (unchanged in eval mode)."""


def _grid(t, B, H, W):
    return t.reshape(B, H, W, -1).permute(0, 3, 1, 2)


def _tok(t):
    B, C, H, W = t.shape
    return t.permute(0, 2, 3, 1).reshape(B, H * W, C)


def torch_lpi(x, dy, p, B, H, W, training=True, dtype=torch.float64, u_stored=None):
    """The reference's lines (F.conv2d with groups=C, F.gelu, F.batch_norm, F.conv2d) under autograd in `dtype` on the CPU,
    on the token-major x, dy [B,H*W,C]; p holds the nine state entries."""
    C = x.shape[-1]
    xg = x.to(dtype).clone().requires_grad_(True)
    q = {k: p[k].to(dtype).clone().requires_grad_(True) for k in GRAD_KEYS}
    rm, rv = p["bn.running_mean"].to(dtype).clone(), p["bn.running_var"].to(dtype).clone()
    c = F.conv2d(_grid(xg, B, H, W), q["conv1.weight"], q["conv1.bias"], padding=1, groups=C)
    u = F.gelu(c)
    u_exact = u.detach()
    if u_stored is not None:
        u = u + (_grid(u_stored.to(dtype), B, H, W) - u_exact)
    ud = u.detach()
    mean = ud.mean((0, 2, 3)) if training else rm.clone()
    var = ud.var((0, 2, 3), unbiased=False) if training else rv.clone()
    z = F.batch_norm(u, rm, rv, q["bn.weight"], q["bn.bias"], training, MOMENTUM, EPS)
    out = _tok(F.conv2d(z, q["conv2.weight"], q["conv2.bias"], padding=1, groups=C))
    out.backward(dy.to(dtype))
    return LpiRef(out.detach(), _tok(u_exact), mean, (var + EPS).rsqrt(), xg.grad, {k: t.grad for k, t in q.items()}, rm, rv)


def _taps(t, w):
    """depthwise 3x3 cross-correlation of t [B,C,H,W] with w [C,9], zero padding: sum_t w[t] t[p + t]."""
    B, C, H, W = t.shape
    tp = F.pad(t, (1, 1, 1, 1))
    out = torch.zeros_like(t)
    for i in range(3):
        for j in range(3):
            out = out + w[:, 3 * i + j].view(1, C, 1, 1) * tp[:, :, i:i + H, j:j + W]
    return out


def _taps_t(t, w):
    """its transpose: sum_t w[t] t[p - t]."""
    return _taps(t, w.flip(-1))


def _tap_grads(a, b):
    """[C,9]: sum_p a[p] b[p + t]."""
    B, C, H, W = a.shape
    bp = F.pad(b, (1, 1, 1, 1))
    return torch.stack([(a * bp[:, :, i:i + H, j:j + W]).sum((0, 2, 3)) for i in range(3) for j in range(3)], dim=-1)


def emulated_lpi(x, dy, p, B, H, W, training=True, dtype=torch.float64, rounding=True):
    """The closed form in `dtype` with exactly the roundings the bf16 kernels declare: u, out and dx on store, and the one
    staged intermediate dc = dL/dc (dx is summed from the rounded dc; conv1's bias and tap gradients from the unrounded
    one).  With rounding=False this is the closed-form gradient, equal to autograd.  The variance is two-pass."""
    r = bf16 if rounding else (lambda t: t)
    C = x.shape[-1]
    M = B * H * W
    xg, dg = _grid(x.to(dtype), B, H, W), _grid(dy.to(dtype), B, H, W)
    w1, w2 = p["conv1.weight"].to(dtype).reshape(C, 9), p["conv2.weight"].to(dtype).reshape(C, 9)
    b1, b2 = p["conv1.bias"].to(dtype).view(1, C, 1, 1), p["conv2.bias"].to(dtype).view(1, C, 1, 1)
    gamma, beta = p["bn.weight"].to(dtype).view(1, C, 1, 1), p["bn.bias"].to(dtype).view(1, C, 1, 1)
    rm, rv = p["bn.running_mean"].to(dtype).clone(), p["bn.running_var"].to(dtype).clone()
    c = _taps(xg, w1) + b1
    u = r(F.gelu(c))
    if training:
        mean = u.mean((0, 2, 3))
        var = ((u - mean.view(1, C, 1, 1)) ** 2).mean((0, 2, 3))
        rm = (1 - MOMENTUM) * rm + MOMENTUM * mean
        rv = (1 - MOMENTUM) * rv + MOMENTUM * var * (M / max(M - 1, 1))
    else:
        mean, var = rm.clone(), rv.clone()
    rstd = 1 / (var + EPS).sqrt()
    uh = (u - mean.view(1, C, 1, 1)) * rstd.view(1, C, 1, 1)
    z = uh * gamma + beta
    out = r(_taps(z, w2) + b2)
    dz = _taps_t(dg, w2)
    dbeta, dgamma = dz.sum((0, 2, 3)), (dz * uh).sum((0, 2, 3))
    if training:
        du = gamma * rstd.view(1, C, 1, 1) * (dz - dbeta.view(1, C, 1, 1) / M - uh * dgamma.view(1, C, 1, 1) / M)
    else:
        du = gamma * rstd.view(1, C, 1, 1) * dz
    cdf = 0.5 * (1 + torch.erf(c * 0.7071067811865476))
    pdf = torch.exp(-0.5 * c * c) * 0.3989422804014327
    dc = du * (cdf + c * pdf)
    dx = r(_taps_t(r(dc), w1))
    grads = {"conv1.weight": _tap_grads(dc, xg).reshape(C, 1, 3, 3), "conv1.bias": dc.sum((0, 2, 3)), "bn.weight": dgamma,
             "bn.bias": dbeta, "conv2.weight": _tap_grads(dg, z).reshape(C, 1, 3, 3), "conv2.bias": dg.sum((0, 2, 3))}
    return LpiRef(_tok(out), _tok(u), mean, rstd, _tok(dx), grads, rm, rv)


ACT_KEYS = ("out", "u", "dx")                 # tensors in the compute dtype
STAT_KEYS = ("mean", "rstd")


def lpi_errors(got, want, training=True):
    """rel-to-max errors of an LpiRef-like `got` against `want`; the running buffers only where the forward moves them."""
    e = {k: rel(getattr(got, k), getattr(want, k)) for k in ACT_KEYS + STAT_KEYS}
    for k in GRAD_KEYS:
        e[k] = rel(got.grads[k], want.grads[k])
    if training:
        e["running_mean"] = rel(got.running_mean, want.running_mean)
        e["running_var"] = rel(got.running_var, want.running_var)
    return e


# ------------------------------------------------------------------------------------------------ inputs ---
def make_params(C, seed):
    """conv weights ~ N(0, 0.3), gamma = 1 +- 0.3, non-zero biases, non-default running buffers (fp32)."""
    return {"conv1.weight": gen((C, 1, 3, 3), seed, 0.3), "conv1.bias": gen((C,), seed + 1, 0.2),
            "bn.weight": 1 + gen((C,), seed + 2, 0.3).clamp(-0.9, 0.9), "bn.bias": gen((C,), seed + 3, 0.2),
            "bn.running_mean": gen((C,), seed + 4, 0.2), "bn.running_var": 0.5 + gen((C,), seed + 5).abs(),
            "bn.num_batches_tracked": torch.tensor(5), "conv2.weight": gen((C, 1, 3, 3), seed + 6, 0.3),
            "conv2.bias": gen((C,), seed + 7, 0.2)}


def make_inputs(B, H, W, C, seed):
    """bf16-rounded unit-normal x and dy [B,H*W,C] (fp32 tensors holding bf16 values)."""
    return bf16(gen((B, H * W, C), seed)), bf16(gen((B, H * W, C), seed + 1))


SWEEP_C = (8, 72, 192)
SWEEP_GRIDS = ((2, 1, 1), (3, 1, 5), (3, 5, 1), (2, 2, 3), (2, 3, 3), (2, 7, 9), (2, 14, 14), (2, 28, 28))
BIG_GRID_CASE = (1, 48, 48, 16)
# the kernels have ONE decomposition for every grid size (no resident / banded switch, no slice-width change with the
# grid), so there are no path-change neighbours to add; the channel-tile width changes with C only: C = 8 is one
# 16-byte group in bf16 (two in fp32), 72 is a ragged tile (9 groups of 16; 18 of 32 in fp32), 192 is two bf16 tiles /
# three fp32 tiles.


def sweep_cases():
    """(B, H, W, C, seed) of section 1."""
    cs = [(B, H, W, C, 100 * C + 10 * H + W) for C in SWEEP_C for (B, H, W) in SWEEP_GRIDS]
    B, H, W, C = BIG_GRID_CASE
    cs.append((B, H, W, C, 100 * C + 10 * H + W))
    return cs


WIDE_CASE = (40, 14, 14, 512)
STRESS_CASE = (4, 14, 14, 64)


def stress_params(C, seed):
    """section 3: channel 3 has conv1.bias = 8 (mean >> spread), channel 5 a zero conv1 weight (u constant)."""
    p = make_params(C, seed)
    p["conv1.bias"][3] = 8.0
    p["conv1.weight"][5] = 0.0
    return p


# ------------------------------------------------------------------------------------------------ the module ---
def module_ref(x, dy, state, H, W, training=True, rounding=False, dtype=torch.float64):
    """The LPI module and its gradients in `dtype`: {"y", "dx", "grad/<key>", "buf/<key>"}.  With rounding, the bf16 mode:
    x and dy are rounded to bf16 on entry and the op applies its declared roundings (emulated_lpi)."""
    r = bf16 if rounding else (lambda t: t)
    B = x.shape[0]
    ref = emulated_lpi(r(x.to(dtype)), r(dy.to(dtype)), state, B, H, W, training=training, dtype=dtype, rounding=rounding)
    out = {"y": ref.out, "dx": ref.dx, "buf/bn.running_mean": ref.running_mean, "buf/bn.running_var": ref.running_var}
    out.update({"grad/" + k: v for k, v in ref.grads.items()})
    return out
