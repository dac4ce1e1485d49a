"""Generate the window-12 golden vectors that pin the oracle to the REFERENCE implementation at window 12.

Like gen_golden.py: runs only in the build container (needs the reference checkout), imports the reference's
models/swin.py unchanged under the timm stand-in (oracle/timm_shim), runs it on seeded inputs / weights in fp32 on
the CPU and stores data only, in the compact forms of tests/fixture_codec.py (inputs and weights on an exact int8
grid, large results as a fixed sample plus row sums).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_window12.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from gen_golden import grads, rnd, seeded_, swin  # noqa: E402  (puts the reference on the path)
from fixture_codec import pow2_scale, put_f, put_i16, put_q8, quantize  # noqa: E402

X_SCALE = 1.0 / 32.0     # inputs: N(0, 1) on a 1/32 grid


def quantize_params_(module):
    """every parameter onto its own power-of-two int8 grid (the reference then runs on exactly those values)"""
    scales = {}
    with torch.no_grad():
        for n, p in module.named_parameters():
            scales[n] = pow2_scale(p)
            p.copy_(quantize(p, scales[n]))
    return scales


def save(name, out):
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes, {len(out)} arrays)")


# WindowAttention(dim=64, window 12, 2 heads, hd 32) over the 8 windows of two 24x24 images, with and without the
# shift-6 mask of that grid (models/swin.py:208-229)
def window_attention_ws12():
    wa = seeded_(swin.WindowAttention(dim=64, window_size=(12, 12), num_heads=2), 31)
    with torch.no_grad():
        wa.relative_position_bias_table.copy_(rnd(wa.relative_position_bias_table.shape, 32, 0.5))
    scales = quantize_params_(wa)
    x, dy = quantize(rnd((8, 144, 64), 33), X_SCALE), quantize(rnd((8, 144, 64), 34), X_SCALE)
    blk = swin.SwinTransformerBlock(dim=64, input_resolution=(24, 24), num_heads=2, window_size=12, shift_size=6)
    mask = blk.attn_mask.clone()                    # [4, 144, 144] of 0 / -100
    out = {}
    put_q8(out, "x", x, X_SCALE)
    put_q8(out, "dy", dy, X_SCALE)
    put_q8(out, "mask", mask, -100.0)
    put_i16(out, "state/relative_position_index", wa.relative_position_index)
    for n, p in wa.named_parameters():
        put_q8(out, "state/" + n, p.detach(), scales[n])
    for masked in (False, True):
        sfx = "_masked" if masked else ""
        wa.zero_grad()
        xr = x.clone().requires_grad_(True)
        y = wa(xr, mask) if masked else wa(xr)
        y.backward(dy)
        put_f(out, "y" + sfx, y)
        put_f(out, "dx" + sfx, xr.grad)
        for n, g in grads(wa).items():
            put_f(out, f"grad{sfx}/{n}", g)
    save("window_attention_ws12", out)


# a two-stage window-12 SwinTransformer: stage 1 (24x24) has shifted windows, stage 2 (12x12) clamps to shift 0
def swin_tiny_ws12():
    s = swin.SwinTransformer(img_size=96, patch_size=4, in_chans=3, num_classes=10, embed_dim=32, depths=[2, 2],
                             num_heads=[1, 2], window_size=12, drop_path_rate=0.0)
    seeded_(s, 35)
    scales = quantize_params_(s)
    x = quantize(rnd((2, 3, 96, 96), 36), X_SCALE)
    y = torch.randint(0, 10, (2,), generator=torch.Generator("cpu").manual_seed(37))
    logits = s(x)
    loss = F.cross_entropy(logits, y)
    loss.backward()
    out = {"labels": y.numpy()}
    put_q8(out, "x", x, X_SCALE)
    put_i16(out, "relative_position_index", s.layers[0].blocks[0].attn.relative_position_index)
    put_q8(out, "attn_mask", s.layers[0].blocks[1].attn_mask, -100.0)
    for n, p in s.named_parameters():
        put_q8(out, "state/" + n, p.detach(), scales[n])
    put_f(out, "logits", logits)
    put_f(out, "loss", loss)
    for n, g in grads(s).items():
        put_f(out, "grad/" + n, g, limit=1024)
    save("swin_tiny_ws12", out)


if __name__ == "__main__":
    torch.set_num_threads(4)
    window_attention_ws12(); swin_tiny_ws12()
