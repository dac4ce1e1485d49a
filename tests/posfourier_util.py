"""Float64 restatement of XCiT's Fourier positional encoding (the reference's models/xcit.py:20-55) for the kernel and module
tests, its closed-form backward, the float32 closed form and the float64 emulation with the roundings the "bf16" path
declares.  Neither touches the library nor the reference tree; tests/golden/pos_fourier.npz pins it to the reference's class.

The table: for the pixel (y, x) of an H x W grid, channel c < 32 is feature j = c of the coordinate y, channel c >= 32
feature j = c - 32 of x; feature j of coordinate i on an axis of n pixels is t = (i + 1) / (n + 1e-6) * 2 pi / T^(2 (j // 2) / 32),
sin(t) for even j, cos(t) for odd j.  The module computes out = x + (table W^T + b), broadcast over the batch.

Declared roundings of compute_dtype "bf16": the feature table, the weight shadow, and dpos (the batch sum of dout) as the
operand of the weight-gradient product.  The bias, the encoding, the sum x + pos and both gradients are fp32."""
import math

import numpy as np
import torch

from vit_attn_util import bf16, gen, rel  # noqa: F401

HIDDEN, TEMPERATURE = 32, 10000.0
TABLE_GRIDS = ((1, 1), (1, 7), (7, 1), (3, 5), (14, 14), (28, 28))
FIXTURE_GRIDS = {"g3x5": (3, 5), "g4x4": (4, 4)}


def features(H, W, dtype=torch.float64):
    """the [H*W, 64] table by the reference's lines in `dtype` (float64: the tests' reference)"""
    y = torch.arange(1, H + 1, dtype=dtype).view(H, 1).expand(H, W)
    x = torch.arange(1, W + 1, dtype=dtype).view(1, W).expand(H, W)
    y = y / (H + 1e-6) * (2 * math.pi)
    x = x / (W + 1e-6) * (2 * math.pi)
    dim_t = torch.arange(HIDDEN, dtype=dtype)
    dim_t = TEMPERATURE ** (2 * torch.div(dim_t, 2, rounding_mode="floor") / HIDDEN)
    px, py = x[:, :, None] / dim_t, y[:, :, None] / dim_t
    px = torch.stack((px[:, :, 0::2].sin(), px[:, :, 1::2].cos()), dim=3).flatten(2)
    py = torch.stack((py[:, :, 0::2].sin(), py[:, :, 1::2].cos()), dim=3).flatten(2)
    return torch.cat((py, px), dim=2).reshape(H * W, 2 * HIDDEN)


def features_np32(H, W):
    """the same table in numpy float32, every step rounded to float32 in the reference's order: the yardstick of what
    float32 sin / cos / pow give"""
    f = np.float32
    y = np.broadcast_to(np.arange(1, H + 1, dtype=f).reshape(H, 1), (H, W))
    x = np.broadcast_to(np.arange(1, W + 1, dtype=f).reshape(1, W), (H, W))
    y = y / (f(H) + f(1e-6)) * f(2 * math.pi)
    x = x / (f(W) + f(1e-6)) * f(2 * math.pi)
    j = np.arange(HIDDEN, dtype=f)
    dim_t = np.power(f(TEMPERATURE), f(2) * np.floor(j / f(2)) / f(HIDDEN)).astype(f)
    px, py = (x[:, :, None] / dim_t).astype(f), (y[:, :, None] / dim_t).astype(f)
    out = np.empty((H, W, 2 * HIDDEN), dtype=f)
    out[:, :, 0:HIDDEN:2], out[:, :, 1:HIDDEN:2] = np.sin(py[:, :, 0::2]), np.cos(py[:, :, 1::2])
    out[:, :, HIDDEN::2], out[:, :, HIDDEN + 1::2] = np.sin(px[:, :, 0::2]), np.cos(px[:, :, 1::2])
    return torch.from_numpy(out.reshape(H * W, 2 * HIDDEN))


def table_f32_error():
    """the worst max |numpy float32 - float64| over TABLE_GRIDS (max |table| is 1, so it is the relative metric too)"""
    return max((features_np32(H, W).double() - features(H, W)).abs().max().item() for H, W in TABLE_GRIDS)


def torch_posenc(x, dy, w, b, H, W, dtype=torch.float64):
    """out = x + (features W^T + b) under autograd in `dtype`: {"out", "pos", "dx", "grad/weight", "grad/bias"}"""
    xg = x.to(dtype).clone().requires_grad_(True)
    wg = w.to(dtype).reshape(w.shape[0], -1).clone().requires_grad_(True)
    bg = b.to(dtype).clone().requires_grad_(True)
    pos = features(H, W, dtype) @ wg.t() + bg
    out = xg + pos
    out.backward(dy.to(dtype))
    return {"out": out.detach(), "pos": pos.detach(), "dx": xg.grad, "grad/weight": wg.grad.reshape(w.shape), "grad/bias": bg.grad}


def closed_posenc(x, dy, w, b, H, W, dtype=torch.float64, emulate=False):
    """The module's own steps in `dtype`: pos = feat W^T + b, out = x + pos; dpos = sum_b dy, dbias = sum_n dpos,
    dW = dpos^T feat, dx = dy.  dtype float32: the float32 closed form (numpy-float32 table).  emulate: the declared bf16
    roundings (docstring) in otherwise-`dtype` arithmetic."""
    r = bf16 if emulate else (lambda t: t)
    feat = (features_np32(H, W) if dtype == torch.float32 else features(H, W)).to(dtype)
    feat = r(feat)
    w2 = r(w.to(dtype).reshape(w.shape[0], -1))
    pos = feat @ w2.t() + b.to(dtype)
    dpos = dy.to(dtype).sum(0)
    return {"out": x.to(dtype) + pos, "pos": pos, "dx": dy.to(dtype), "grad/weight": (r(dpos).t() @ feat).reshape(w.shape),
            "grad/bias": dpos.sum(0)}


KEYS = ("out", "pos", "grad/weight", "grad/bias")


def errors(got, want, keys=KEYS):
    return {k: rel(got[k], want[k]) for k in keys}


def fixture_case(fx, name):
    """(x, dy, weight, bias, (H, W), want) of one grid of tests/golden/pos_fourier.npz"""
    import fixture_codec as FC
    d = FC.group(fx, name)
    H, W = (int(v) for v in d["grid"].tolist())
    want = {"pos": d["pos"], "out": d["x"] + d["pos"], "grad/weight": d["grad/token_projection.weight"],
            "grad/bias": d["grad/token_projection.bias"]}
    return d["x"], d["dy"], d["state/token_projection.weight"], d["state/token_projection.bias"], (H, W), want


def measure(x, dy, w, b, H, W):
    """(float32 closed form's error, bf16 emulation's error) against float64 on the same inputs, per tensor"""
    ref = torch_posenc(x, dy, w, b, H, W)
    return (errors(closed_posenc(x, dy, w, b, H, W, torch.float32), ref),
            errors(closed_posenc(x, dy, w, b, H, W, torch.float64, emulate=True), ref))
