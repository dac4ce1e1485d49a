"""XCiT's PositionalEncodingFourier and ClassAttentionBlock on one MI355X: the library's modules in bf16, forward (no_grad)
and forward + backward, beside a plain PyTorch composition of the reference's models/xcit.py:20-55 and :144-218 written here
(bf16 parameters and activations, autograd backward) on the same device, and the times of the element-wise kernels of
csrc/xcit_glue.hip on the module's own shapes with the bytes each moves.  Shapes: xcit_small_12_p16 (B 256, N1 197, D 384, 8
heads) and xcit_small_12_p8 (N1 785).  20 timed calls after 3, device events around the loop.  No pass / fail threshold.

    python tools/xcit_ca_bench.py        # one JSON line per shape

Run under a time limit (timeout -k 10 <s> python tools/xcit_ca_bench.py)."""
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

SHAPES = [("xcit_small_12_p16", 256, 14, 384, 8), ("xcit_small_12_p8", 256, 28, 384, 8)]      # name, batch, grid side, D, heads


def _time(fn, iters=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / iters


class ComposedPos(nn.Module):
    def __init__(self, dim, hidden=32, temperature=10000):
        super().__init__()
        self.token_projection = nn.Conv2d(hidden * 2, dim, kernel_size=1)
        self.hidden, self.temperature = hidden, temperature

    def forward(self, x, H, W):
        B, dev = x.shape[0], x.device
        y = torch.arange(1, H + 1, dtype=torch.float32, device=dev).view(1, H, 1).expand(B, H, W)
        xx = torch.arange(1, W + 1, dtype=torch.float32, device=dev).view(1, 1, W).expand(B, H, W)
        y, xx = y / (H + 1e-6) * 2 * math.pi, xx / (W + 1e-6) * 2 * math.pi
        dim_t = torch.arange(self.hidden, dtype=torch.float32, device=dev)
        dim_t = self.temperature ** (2 * (dim_t // 2) / self.hidden)
        px, py = xx[:, :, :, None] / dim_t, y[:, :, :, None] / dim_t
        px = torch.stack((px[:, :, :, 0::2].sin(), px[:, :, :, 1::2].cos()), dim=4).flatten(3)
        py = torch.stack((py[:, :, :, 0::2].sin(), py[:, :, :, 1::2].cos()), dim=4).flatten(3)
        pos = self.token_projection(torch.cat((py, px), dim=3).permute(0, 3, 1, 2).to(x.dtype))
        return x + pos.reshape(B, -1, H * W).permute(0, 2, 1)


class ComposedBlock(nn.Module):
    def __init__(self, dim, heads, eta=1.0, tokens_norm=True):
        super().__init__()
        self.norm1, self.norm2 = nn.LayerNorm(dim, eps=1e-6), nn.LayerNorm(dim, eps=1e-6)
        self.qkv, self.proj = nn.Linear(dim, 3 * dim), nn.Linear(dim, dim)
        self.fc1, self.fc2 = nn.Linear(dim, 4 * dim), nn.Linear(4 * dim, dim)
        self.gamma1, self.gamma2 = nn.Parameter(eta * torch.ones(dim)), nn.Parameter(eta * torch.ones(dim))
        self.heads, self.tokens_norm = heads, tokens_norm

    def forward(self, x):
        B, N, C = x.shape
        l = self.norm1(x)
        qkv = self.qkv(l).reshape(B, N, 3, self.heads, C // self.heads).permute(2, 0, 3, 1, 4)
        q, k, v = qkv[0], qkv[1], qkv[2]
        att = ((q[:, :, 0:1] * k).sum(-1) * (C // self.heads) ** -0.5).softmax(-1)
        cls = self.proj((att.unsqueeze(2) @ v).transpose(1, 2).reshape(B, 1, C))
        x = x + self.gamma1 * torch.cat([cls, l[:, 1:]], dim=1)
        x = self.norm2(x) if self.tokens_norm else torch.cat([self.norm2(x[:, 0:1]), x[:, 1:]], dim=1)
        cls = self.gamma2 * self.fc2(F.gelu(self.fc1(x[:, 0:1])))
        return x + torch.cat([cls, x[:, 1:]], dim=1)


def fwd_and_both(m, call, dout):
    with torch.no_grad():
        fwd = _time(call)

    def both():
        for p in m.parameters():
            p.grad = None
        call().backward(dout)
    return round(fwd, 1), round(_time(both), 1)


def glue_kernels(B, N1, D):
    """us and GB/s of each element-wise kernel on the block's shapes (bf16 operands, fp32 residual stream)"""
    from vit_torch_amd import ops
    bf, f32 = torch.bfloat16, torch.float32
    r = lambda *s, dtype=f32: torch.randn(s, device="cuda").to(dtype)      # noqa: E731
    x, G, x1, dl, l, a, da, g = r(B, N1, D), r(B, N1, D), r(B, N1, D), r(B, N1, D), r(B, N1, D, dtype=bf), r(B, D, dtype=bf), \
        r(B, D, dtype=bf), r(D)
    dg, pos = torch.empty(D, device="cuda"), r(N1 - 1, D)
    n = B * N1 * D
    cases = {"ca_merge_fwd": (lambda: ops.ca_merge_fwd(x, a, l, g, x1, B, N1, D), 10 * n),
             "ca_merge_bwd": (lambda: ops.ca_merge_bwd(G, l, a, g, da, dl, dg, B, N1, D), 10 * n),
             "ca_out_fwd": (lambda: ops.ca_out_fwd(x.view(B, N1 * D)[:, :D], x, a, g, x1, B, N1, D), 8 * n),
             "ca_out_bwd": (lambda: ops.ca_out_bwd(G, g, dl, da, B, N1, D), 8 * n),
             "add_rows_bcast": (lambda: ops.add_rows_bcast(xs, pos, xo, B, N1 - 1, D),
                                8 * B * (N1 - 1) * D)}
    xs, xo = r(B, N1 - 1, D), torch.empty((B, N1 - 1, D), device="cuda")
    out = {}
    for k, (fn, nbytes) in cases.items():
        us = _time(fn)
        out[k] = {"us": round(us, 1), "GBps": round(nbytes / us / 1e3, 0)}
    return out


def main():
    from vit_torch_amd import ClassAttentionBlock, PositionalEncodingFourier
    for name, B, side, D, heads in SHAPES:
        Np = side * side
        N1 = Np + 1
        g = torch.Generator("cuda").manual_seed(0)
        res = dict(shape=name, B=B, N1=N1, D=D, heads=heads)
        # positional encoding on the patch tokens
        xp, dp = torch.randn((B, Np, D), device="cuda", generator=g), torch.randn((B, Np, D), device="cuda", generator=g)
        m = PositionalEncodingFourier(dim=D, compute_dtype="bf16").cuda()
        res["pos_fwd_us"], res["pos_fwd_bwd_us"] = fwd_and_both(m, lambda: m(xp, side, side), dp)
        c = ComposedPos(D).cuda().to(torch.bfloat16)
        xb, db = xp.to(torch.bfloat16), dp.to(torch.bfloat16)
        res["pos_composed_fwd_us"], res["pos_composed_fwd_bwd_us"] = fwd_and_both(c, lambda: c(xb, side, side), db)
        del m, c, xp, dp, xb, db
        # the class-attention block
        x, dout = torch.randn((B, N1, D), device="cuda", generator=g), torch.randn((B, N1, D), device="cuda", generator=g)
        for tn in (True, False):
            tag = "tn" if tn else "cls"
            m = ClassAttentionBlock(D, heads, qkv_bias=True, eta=1.0, tokens_norm=tn, compute_dtype="bf16").cuda()
            res[f"ca_{tag}_fwd_us"], res[f"ca_{tag}_fwd_bwd_us"] = fwd_and_both(m, lambda: m(x, side, side), dout)
            c = ComposedBlock(D, heads, tokens_norm=tn).cuda().to(torch.bfloat16)
            xb, db = x.to(torch.bfloat16), dout.to(torch.bfloat16)
            res[f"ca_{tag}_composed_fwd_us"], res[f"ca_{tag}_composed_fwd_bwd_us"] = fwd_and_both(c, lambda: c(xb), db)
            del m, c, xb, db
        res["kernels"] = glue_kernels(B, N1, D)
        print(json.dumps(res), flush=True)
        del x, dout
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
