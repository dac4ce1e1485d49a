"""Generate the golden vectors that pin the oracle to the REFERENCE's CaiT attention at 384-pixel sequence lengths.

Like gen_golden_window12.py: runs only in the build container (needs the reference checkout), imports the reference's
models/cait.py unchanged under the timm stand-in (oracle/timm_shim), runs its Attention_talking_head over 576 tokens and
its Class_Attention over 577 tokens (cait_S24 at 384 x 384: D = 384, 8 heads, hd = 48) in fp32 on the CPU, and stores
data only, in the compact forms of tests/fixture_codec.py.  Inputs and weights sit on coarse power-of-two grids (int8
storage, few distinct values) so that each .npz stays well under 1 MB; large results keep a fixed sample and row sums.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_cait_long.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from gen_golden import cait, grads, rnd, seeded_  # noqa: E402  (puts the reference on the path)
from fixture_codec import pow2_scale, put_f, put_q8, quantize  # noqa: E402

D, H = 384, 8
X_SCALE = 1.0 / 8.0      # inputs: N(0, 1) on a 1/8 grid
COARSE = 16.0            # the D x D weights: a grid 16x coarser than the finest int8 grid of their range (|k| <= 8)


def quantize_params_(module):
    scales = {}
    with torch.no_grad():
        for n, p in module.named_parameters():
            scales[n] = pow2_scale(p) * (COARSE if p.numel() > 4096 else 1.0)     # the head mixes and biases: fine
            p.copy_(quantize(p, scales[n]))
    return scales


def save(name, out):
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes, {len(out)} arrays)")


def store(out, module, scales, x, dy, y, dx):
    put_q8(out, "x", x, X_SCALE)
    put_q8(out, "dy", dy, X_SCALE)
    for n, p in module.named_parameters():
        put_q8(out, "state/" + n, p.detach(), scales[n])
    put_f(out, "y", y)
    put_f(out, "dx", dx)
    for n, g in grads(module).items():
        put_f(out, "grad/" + n, g)


# Attention_talking_head (models/cait.py:87-128) over one image of 576 tokens
def talking_heads_576():
    th = seeded_(cait.Attention_talking_head(dim=D, num_heads=H, qkv_bias=True), 61)
    with torch.no_grad():                           # mixes near the identity, as trained ones are
        th.proj_l.weight.mul_(6.0).add_(torch.eye(H))
        th.proj_w.weight.mul_(6.0).add_(torch.eye(H))
    scales = quantize_params_(th)
    x, dy = quantize(rnd((1, 576, D), 62), X_SCALE), quantize(rnd((1, 576, D), 63), X_SCALE)
    xr = x.clone().requires_grad_(True)
    y = th(xr)
    y.backward(dy)
    out = {}
    store(out, th, scales, x, dy, y, xr.grad)
    save("talking_heads_576", out)


# Class_Attention (models/cait.py:21-55): the CLS row against 577 tokens, two images
def class_attention_577():
    ca = seeded_(cait.Class_Attention(dim=D, num_heads=H, qkv_bias=True), 64)
    scales = quantize_params_(ca)
    x, dy = quantize(rnd((2, 577, D), 65), X_SCALE), quantize(rnd((2, 1, D), 66), X_SCALE)
    xr = x.clone().requires_grad_(True)
    y = ca(xr)
    y.backward(dy)
    out = {}
    store(out, ca, scales, x, dy, y, xr.grad)
    save("class_attention_577", out)


if __name__ == "__main__":
    torch.set_num_threads(4)
    talking_heads_576(); class_attention_577()
