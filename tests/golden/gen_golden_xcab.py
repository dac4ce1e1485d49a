"""Generate the golden vectors that pin the XCABlock test reference to the REFERENCE implementation's class.

Like gen_golden_xcit_ca.py and gen_golden_lpi.py: runs only in the build container (needs the reference checkout), imports
the reference's models/xcit.py unchanged under the timm stand-in (oracle/timm_shim), runs its XCABlock class (dim 64, 2 heads,
mlp_ratio 2, qkv_bias, eta 0.5, LayerNorm eps 1e-6; its LPI's SyncBatchNorm runs in a single CPU process in train and eval
mode) in fp32 on the CPU on B = 2 images of a 3 x 5 grid, on seeded, grid-quantised inputs and parameters with the three
gammas (none 1, not all equal), the three norms' weights and biases, the temperature (not 1), the BN weight / bias perturbed
and non-default running buffers (num_batches_tracked = 7), and stores data only, in the forms of tests/fixture_codec.py:
x, dy, the state, the train-mode out, dx and every parameter gradient (the four Linear weight gradients as a sample of 1024
entries and their row sums), the three buffers after that forward, out_eval: the eval-mode output on the updated buffers,
and the reference's state-dict key / shape / dtype list as text.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_xcab.py
"""
import os
import sys
from functools import partial

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

DIM, HEADS, B, GRID, ETA, EPS, MLP_RATIO = 64, 2, 2, (3, 5), 0.5, 1e-6, 2.0
BUF_SCALE = 1.0 / 64.0
SEED = 2300


def block():
    m = seeded_(xcit.XCABlock(DIM, HEADS, mlp_ratio=MLP_RATIO, qkv_bias=True, eta=ETA,
                              norm_layer=partial(torch.nn.LayerNorm, eps=EPS)), SEED)
    bn = m.local_mp.bn
    with torch.no_grad():
        for k, (n, p) in enumerate(m.named_parameters()):
            if p.dim() == 2:
                p.copy_(rnd(p.shape, SEED + 10 + k, p.shape[1] ** -0.5))
            elif p.dim() == 4:
                p.copy_(rnd(p.shape, SEED + 10 + k, 0.3))
            elif n.endswith("conv1.bias") or n.endswith("conv2.bias"):
                p.copy_(rnd(p.shape, SEED + 10 + k, 0.2))
        for k, norm in enumerate((m.norm1, m.norm2, m.norm3, bn)):
            norm.weight.copy_(1 + rnd((DIM,), SEED + 40 + k, 0.3).clamp(-0.9, 0.9))
            norm.bias.copy_(rnd((DIM,), SEED + 50 + k, 0.2))
        for k, g in enumerate((m.gamma1, m.gamma2, m.gamma3)):
            g.copy_(ETA + rnd((DIM,), SEED + 60 + k, 0.2).clamp(-0.4, 0.4))
        m.attn.temperature.copy_(torch.tensor([0.75, 1.5]).view(HEADS, 1, 1))
        bn.running_mean.copy_(quantize(rnd((DIM,), SEED + 70, 0.2), BUF_SCALE))
        bn.running_var.copy_(quantize(0.5 + rnd((DIM,), SEED + 71).abs(), BUF_SCALE))
        bn.num_batches_tracked.fill_(7)
    scales = quantize_params_(m)
    N = GRID[0] * GRID[1]
    x, dy = quantize(rnd((B, N, DIM), SEED + 90), X_SCALE), quantize(rnd((B, N, DIM), SEED + 91), X_SCALE)
    out = {}
    put_q8(out, "x", x, X_SCALE)
    put_q8(out, "dy", dy, X_SCALE)
    put_i16(out, "heads", torch.tensor(HEADS))
    put_i16(out, "grid", torch.tensor(GRID))
    for n, p in m.named_parameters():
        put_q8(out, "state/" + n, p.detach(), scales[n])
    put_q8(out, "state/local_mp.bn.running_mean", bn.running_mean, BUF_SCALE)
    put_q8(out, "state/local_mp.bn.running_var", bn.running_var, BUF_SCALE)
    put_i16(out, "state/local_mp.bn.num_batches_tracked", bn.num_batches_tracked)
    keys = "\n".join(f"{k} {tuple(v.shape)} {str(v.dtype).replace('torch.', '')}" for k, v in m.state_dict().items())
    out["keys"] = np.frombuffer(keys.encode(), dtype=np.uint8).copy()       # the reference's state-dict list, as text
    m.train()
    xr = x.clone().requires_grad_(True)
    y = m(xr, *GRID)
    y.backward(dy)
    put_f(out, "out", y)
    put_f(out, "dx", xr.grad)
    for n, g in grads(m).items():
        put_f(out, "grad/" + n, g, limit=1024)
    put_f(out, "after/local_mp.bn.running_mean", bn.running_mean)
    put_f(out, "after/local_mp.bn.running_var", bn.running_var)
    put_i16(out, "after/local_mp.bn.num_batches_tracked", bn.num_batches_tracked)
    m.eval()
    with torch.no_grad():
        put_f(out, "out_eval", m(x, *GRID))
    save("xcab", out)


if __name__ == "__main__":
    torch.set_num_threads(4)
    block()
