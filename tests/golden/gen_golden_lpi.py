"""Generate the golden vectors that pin the LPI test reference to the REFERENCE implementation's LPI class.

Like gen_golden_xca.py: runs only in the build container (needs the reference checkout), imports the reference's
models/xcit.py unchanged under the timm stand-in (oracle/timm_shim), runs its LPI class (with its SyncBatchNorm, which
runs in a single CPU process in train and eval mode) in fp32 on the CPU on seeded, grid-quantised input and parameters
with non-trivial bn.weight / bn.bias and non-default starting running buffers, and stores data only, in the forms of
tests/fixture_codec.py: x, dy, the state, the train-mode y, dx and six parameter gradients, the three buffers after that
forward, and y_eval: the eval-mode output on the updated buffers.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_lpi.py
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
from fixture_codec import put_f, put_i16, put_q8, quantize  # noqa: E402
from models import xcit  # noqa: E402  (the reference's own file)

DIM, B, H, W = 96, 2, 3, 5
BUF_SCALE = 1.0 / 64.0


def lpi():
    m = seeded_(xcit.LPI(DIM), 51)
    with torch.no_grad():
        m.conv1.weight.copy_(rnd(m.conv1.weight.shape, 52, 0.3))
        m.conv2.weight.copy_(rnd(m.conv2.weight.shape, 53, 0.3))
        m.conv1.bias.copy_(rnd((DIM,), 54, 0.2))
        m.conv2.bias.copy_(rnd((DIM,), 55, 0.2))
        m.bn.weight.copy_(1 + rnd((DIM,), 56, 0.3).clamp(-0.9, 0.9))
        m.bn.bias.copy_(rnd((DIM,), 57, 0.2))
        m.bn.running_mean.copy_(quantize(rnd((DIM,), 58, 0.2), BUF_SCALE))
        m.bn.running_var.copy_(quantize(0.5 + rnd((DIM,), 59).abs(), BUF_SCALE))
        m.bn.num_batches_tracked.fill_(7)
    scales = quantize_params_(m)
    x, dy = quantize(rnd((B, H * W, DIM), 60), X_SCALE), quantize(rnd((B, H * W, DIM), 61), X_SCALE)
    out = {}
    put_q8(out, "x", x, X_SCALE)
    put_q8(out, "dy", dy, X_SCALE)
    for n, p in m.named_parameters():
        put_q8(out, "state/" + n, p.detach(), scales[n])
    put_q8(out, "state/bn.running_mean", m.bn.running_mean, BUF_SCALE)
    put_q8(out, "state/bn.running_var", m.bn.running_var, BUF_SCALE)
    put_i16(out, "state/bn.num_batches_tracked", m.bn.num_batches_tracked)
    m.train()
    xr = x.clone().requires_grad_(True)
    y = m(xr, H, W)
    y.backward(dy)
    put_f(out, "y", y)
    put_f(out, "dx", xr.grad)
    for n, g in grads(m).items():
        put_f(out, "grad/" + n, g)
    put_f(out, "after/bn.running_mean", m.bn.running_mean)
    put_f(out, "after/bn.running_var", m.bn.running_var)
    put_i16(out, "after/bn.num_batches_tracked", m.bn.num_batches_tracked)
    m.eval()
    with torch.no_grad():
        put_f(out, "y_eval", m(x, H, W))
    save("lpi", out)


if __name__ == "__main__":
    torch.set_num_threads(4)
    lpi()
