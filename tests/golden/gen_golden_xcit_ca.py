"""Generate the golden vectors that pin the class-attention-block test reference to the REFERENCE implementation's class.

Like gen_golden_convembed.py: runs only in the build container (needs the reference checkout), imports the reference's
models/xcit.py unchanged under the timm stand-in (oracle/timm_shim), runs its ClassAttentionBlock class (dim 64, 2 heads, mlp_ratio 2,
qkv_bias, eta 0.5, LayerNorm eps 1e-6) in fp32 on the CPU on seeded, grid-quantised inputs and parameters, with the norm
weights / biases and both gammas perturbed (the gammas are neither 1 nor all equal), and stores data only, in the forms of
tests/fixture_codec.py, for two configurations on B = 2 images of a 2 x 3 grid (N1 = 7):
    tn:  tokens_norm=True      cls: tokens_norm=False
Per configuration: x, dy, the state, the output, dx and every parameter gradient (the four weight gradients as a sample of
1024 entries and their row sums).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_xcit_ca.py
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

DIM, HEADS, B, GRID, ETA, EPS, MLP_RATIO = 64, 2, 2, (2, 3), 0.5, 1e-6, 2.0
CONFIGS = {"tn": True, "cls": False}


def block(out, name, tokens_norm, seed):
    m = seeded_(xcit.ClassAttentionBlock(DIM, HEADS, mlp_ratio=MLP_RATIO, qkv_bias=True, eta=ETA, tokens_norm=tokens_norm,
                                         norm_layer=partial(torch.nn.LayerNorm, eps=EPS)), seed)
    with torch.no_grad():
        for k, p in enumerate(m.parameters()):
            if p.dim() == 2:
                p.copy_(rnd(p.shape, seed + 10 + k, p.shape[1] ** -0.5))
        for k, norm in enumerate((m.norm1, m.norm2)):
            norm.weight.copy_(1 + rnd((DIM,), seed + 40 + k, 0.3).clamp(-0.9, 0.9))
            norm.bias.copy_(rnd((DIM,), seed + 50 + k, 0.2))
        m.gamma1.copy_(ETA + rnd((DIM,), seed + 60, 0.2).clamp(-0.4, 0.4))
        m.gamma2.copy_(ETA + rnd((DIM,), seed + 61, 0.2).clamp(-0.4, 0.4))
    scales = quantize_params_(m)
    N1 = 1 + GRID[0] * GRID[1]
    x = quantize(rnd((B, N1, DIM), seed + 90), X_SCALE).requires_grad_(True)
    dy = quantize(rnd((B, N1, DIM), seed + 91), X_SCALE)
    # tokens_norm=False writes norm2's output over the view norm2 has just read (x[:, 0:1] = self.norm2(x[:, 0:1])), which
    # this PyTorch's autograd refuses at backward time; under allow_mutation_on_saved_tensors the saved input is cloned at
    # the write and the reference's own lines differentiate as written
    with torch.autograd.graph.allow_mutation_on_saved_tensors():
        y = m(x, *GRID)
        y.backward(dy)
    put_q8(out, name + "/x", x.detach(), X_SCALE)
    put_q8(out, name + "/dy", dy, X_SCALE)
    put_i16(out, name + "/heads", torch.tensor(HEADS))
    put_i16(out, name + "/tokens_norm", torch.tensor(int(tokens_norm)))
    for n, p in m.named_parameters():
        put_q8(out, f"{name}/state/{n}", p.detach(), scales[n])
    put_f(out, name + "/out", y)
    put_f(out, name + "/dx", x.grad)
    for n, g in grads(m).items():
        put_f(out, f"{name}/grad/{n}", g, limit=1024)
    keys = "\n".join(f"{k} {tuple(v.shape)} {str(v.dtype).replace('torch.', '')}" for k, v in m.state_dict().items())
    out[name + "/keys"] = np.frombuffer(keys.encode(), dtype=np.uint8).copy()       # the reference's state-dict list, as text


if __name__ == "__main__":
    torch.set_num_threads(4)
    out = {}
    for i, (name, tn) in enumerate(CONFIGS.items()):
        block(out, name, tn, 1700 + 100 * i)
    save("xcit_ca", out)
