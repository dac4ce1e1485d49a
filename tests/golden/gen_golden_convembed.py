"""Generate the golden vectors that pin the ConvPatchEmbed test reference to the REFERENCE implementation's class.

Like gen_golden_lpi.py: runs only in the build container (needs the reference checkout), imports the reference's
models/xcit.py unchanged under the timm stand-in (oracle/timm_shim), runs its ConvPatchEmbed class (with its SyncBatchNorm,
which runs in a single CPU process in train and eval mode) in fp32 on the CPU on seeded, grid-quantised images and
parameters with non-trivial norm weights / biases and non-default starting running buffers, and stores data only, in the
forms of tests/fixture_codec.py, for two configurations:
    p16: patch 16, embed_dim 64, image [2, 3, 32, 32]  (grids 16 -> 8 -> 4 -> 2)
    p8:  patch 8,  embed_dim 64, image [2, 3, 24, 40]  (12x20 -> 6x10 -> 3x5: the last stage sees an odd width)
Per configuration: x, dy, the state, the train-mode tokens y, every parameter gradient, the buffers after that forward, and
y_eval: the eval-mode tokens on the updated buffers.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_convembed.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from gen_golden import grads, rnd, seeded_  # noqa: E402  (puts the reference on the path)
from gen_golden_window12 import X_SCALE, quantize_params_, save  # noqa: E402
from fixture_codec import put_f, put_i16, put_q8, quantize  # noqa: E402
from models import xcit  # noqa: E402  (the reference's own file)

EMBED = 64
CONFIGS = {"p16": (16, (2, 3, 32, 32)), "p8": (8, (2, 3, 24, 40))}
BUF_SCALE = 1.0 / 64.0


def conv_embed(out, name, patch, shape, seed):
    m = seeded_(xcit.ConvPatchEmbed(img_size=shape[2], patch_size=patch, embed_dim=EMBED), seed)
    stages = [s for s in m.proj if isinstance(s, torch.nn.Sequential)]
    with torch.no_grad():
        for k, (conv, bn) in enumerate(stages):
            C, fan = conv.weight.shape[0], conv.weight.shape[1] * 9
            conv.weight.copy_(rnd(conv.weight.shape, seed + 10 * k + 1, fan ** -0.5))
            bn.weight.copy_(1 + rnd((C,), seed + 10 * k + 2, 0.3).clamp(-0.9, 0.9))
            bn.bias.copy_(rnd((C,), seed + 10 * k + 3, 0.2))
            bn.running_mean.copy_(quantize(rnd((C,), seed + 10 * k + 4, 0.2), BUF_SCALE))
            bn.running_var.copy_(quantize(0.5 + rnd((C,), seed + 10 * k + 5).abs(), BUF_SCALE))
            bn.num_batches_tracked.fill_(7 + k)
    scales = quantize_params_(m)
    x = quantize(rnd(shape, seed + 90), X_SCALE)
    m.train()
    y, (Hp, Wp) = m(x)
    dy = quantize(rnd(tuple(y.shape), seed + 91), X_SCALE)
    put_q8(out, name + "/x", x, X_SCALE)
    put_q8(out, name + "/dy", dy, X_SCALE)
    put_i16(out, name + "/grid", torch.tensor([Hp, Wp]))
    # the state as it was BEFORE the forward: the buffers were set above and the forward has moved them, so rebuild them
    for k, (conv, bn) in enumerate(stages):
        C = conv.weight.shape[0]
        put_q8(out, f"{name}/state/proj.{2 * k}.1.running_mean", quantize(rnd((C,), seed + 10 * k + 4, 0.2), BUF_SCALE), BUF_SCALE)
        put_q8(out, f"{name}/state/proj.{2 * k}.1.running_var", quantize(0.5 + rnd((C,), seed + 10 * k + 5).abs(), BUF_SCALE),
               BUF_SCALE)
        put_i16(out, f"{name}/state/proj.{2 * k}.1.num_batches_tracked", torch.tensor(7 + k))
    for n, p in m.named_parameters():
        put_q8(out, f"{name}/state/{n}", p.detach(), scales[n])
    y.backward(dy)
    put_f(out, name + "/y", y)
    for n, g in grads(m).items():
        put_f(out, f"{name}/grad/{n}", g)
    for n, b in m.named_buffers():
        (put_i16 if n.endswith("tracked") else put_f)(out, f"{name}/after/{n}", b)
    keys = "\n".join(f"{k} {tuple(v.shape)} {str(v.dtype).replace('torch.', '')}" for k, v in m.state_dict().items())
    out[name + "/keys"] = np.frombuffer(keys.encode(), dtype=np.uint8).copy()       # the reference's state-dict list, as text
    m.eval()
    with torch.no_grad():
        put_f(out, name + "/y_eval", m(x)[0])


if __name__ == "__main__":
    torch.set_num_threads(4)
    out = {}
    for i, (name, (patch, shape)) in enumerate(CONFIGS.items()):
        conv_embed(out, name, patch, shape, 700 + 100 * i)
    save("conv_patch_embed", out)
