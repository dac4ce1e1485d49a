"""Generate the golden vectors that pin the XCA test reference to the REFERENCE implementation's XCA class.

Like gen_golden_window12.py: runs only in the build container (needs the reference checkout), imports the reference's
models/xcit.py unchanged under the timm stand-in (oracle/timm_shim), runs its XCA class in fp32 on the CPU on seeded,
grid-quantised input and weights with non-trivial temperatures, and stores data only, in the forms of
tests/fixture_codec.py: x, dy, the parameters, y, dx and the five parameter gradients (the two weight gradients as a
fixed sample plus row sums).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_xca.py
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from gen_golden import grads, rnd, seeded_  # noqa: E402  (puts the reference on the path)
from gen_golden_window12 import X_SCALE, quantize_params_, save  # noqa: E402
from fixture_codec import put_f, put_q8, quantize  # noqa: E402
from models import xcit  # noqa: E402  (the reference's own file)

DIM, HEADS, B, N = 96, 3, 2, 20


def xca():
    m = seeded_(xcit.XCA(DIM, num_heads=HEADS, qkv_bias=True), 41)
    with torch.no_grad():
        m.temperature.copy_(torch.tensor([0.5, 1.25, 3.0]).view(HEADS, 1, 1))
        m.qkv.bias.copy_(rnd(m.qkv.bias.shape, 42, 0.1))
        m.proj.bias.copy_(rnd(m.proj.bias.shape, 43, 0.1))
    scales = quantize_params_(m)
    x, dy = quantize(rnd((B, N, DIM), 44), X_SCALE), quantize(rnd((B, N, DIM), 45), X_SCALE)
    out = {}
    put_q8(out, "x", x, X_SCALE)
    put_q8(out, "dy", dy, X_SCALE)
    for n, p in m.named_parameters():
        put_q8(out, "state/" + n, p.detach(), scales[n])
    xr = x.clone().requires_grad_(True)
    y = m(xr)
    y.backward(dy)
    put_f(out, "y", y)
    put_f(out, "dx", xr.grad)
    for n, g in grads(m).items():
        put_f(out, "grad/" + n, g)
    save("xca", out)


if __name__ == "__main__":
    torch.set_num_threads(4)
    xca()
