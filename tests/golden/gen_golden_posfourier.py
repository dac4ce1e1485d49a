"""Generate the golden vectors that pin the positional-encoding test reference to the REFERENCE implementation's class.

Like gen_golden_convembed.py: runs only in the build container (needs the reference checkout), imports the reference's
models/xcit.py unchanged under the timm stand-in (oracle/timm_shim), runs its PositionalEncodingFourier class (hidden_dim 32,
dim 64) in fp32 on the CPU with seeded, grid-quantised parameters, the way XCiT.forward_features uses it
(x + pos.reshape(B, -1, N).permute(0, 2, 1)), and stores data only, in the forms of tests/fixture_codec.py, for two grids:
    g3x5: (3, 5)     g4x4: (4, 4)      B = 2
Per grid: x, dy, the state, the encoding pos as [Hp*Wp, dim], and the weight and bias gradients of x + pos for dy.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_posfourier.py
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

DIM, B = 64, 2
GRIDS = {"g3x5": (3, 5), "g4x4": (4, 4)}


def posenc(out, name, H, W, seed):
    m = seeded_(xcit.PositionalEncodingFourier(hidden_dim=32, dim=DIM), seed)
    with torch.no_grad():
        m.token_projection.weight.copy_(rnd(m.token_projection.weight.shape, seed + 1, 64 ** -0.5))
        m.token_projection.bias.copy_(rnd((DIM,), seed + 2, 0.2))
    scales = quantize_params_(m)
    x = quantize(rnd((B, H * W, DIM), seed + 90), X_SCALE)
    dy = quantize(rnd((B, H * W, DIM), seed + 91), X_SCALE)
    pos = m(B, H, W)
    y = x + pos.reshape(B, -1, H * W).permute(0, 2, 1)
    y.backward(dy)
    assert torch.equal(pos[0], pos[1])
    put_q8(out, name + "/x", x, X_SCALE)
    put_q8(out, name + "/dy", dy, X_SCALE)
    put_i16(out, name + "/grid", torch.tensor([H, W]))
    for n, p in m.named_parameters():
        put_q8(out, f"{name}/state/{n}", p.detach(), scales[n])
    put_f(out, name + "/pos", pos[0].reshape(DIM, H * W).t().contiguous())
    for n, g in grads(m).items():
        put_f(out, f"{name}/grad/{n}", g)
    keys = "\n".join(f"{k} {tuple(v.shape)} {str(v.dtype).replace('torch.', '')}" for k, v in m.state_dict().items())
    out[name + "/keys"] = np.frombuffer(keys.encode(), dtype=np.uint8).copy()       # the reference's state-dict list, as text


if __name__ == "__main__":
    torch.set_num_threads(4)
    out = {}
    for i, (name, (H, W)) in enumerate(GRIDS.items()):
        posenc(out, name, H, W, 1500 + 100 * i)
    save("pos_fourier", out)
