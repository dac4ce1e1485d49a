"""XCiT's XCABlock on one MI355X: the library's module in bf16, forward (no_grad) and forward + backward, beside a plain
PyTorch composition of the reference's models/xcit.py:264-292 written here (bf16 parameters and activations, autograd
backward) on the same device; and the block's junction kernel alone (ops.ls_residual_ln_fwd, csrc/layernorm.hip: y = x +
gamma * b, l = LayerNorm(y), 12 bytes per element with a bf16 branch) beside the two passes it replaces, a residual pass
(ops.ca_merge_fwd, which moves the same 10 bytes per element: fp32 x and bf16 branch in, fp32 out) followed by
ops.layernorm_fwd (6 bytes per element), with the bytes each must move and the largest difference between the two forms'
outputs.  Shape: the trunk of xcit_small_12_p16 (B 64, 14 x 14 tokens, dim 384, 8 heads).  20 timed calls after 3, device
events around the loop.  No pass / fail threshold.

    python tools/xcablock_bench.py        # one JSON line

Run under a time limit (timeout -k 10 <s> python tools/xcablock_bench.py)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

SHAPES = [("xcit_small_12_p16", 64, 14, 384, 8)]      # name, batch, grid side, D, heads


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


class ComposedBlock(nn.Module):
    def __init__(self, dim, heads, eta=1.0, mlp_ratio=4.0):
        super().__init__()
        self.norm1, self.norm2, self.norm3 = (nn.LayerNorm(dim, eps=1e-6) for _ in range(3))
        self.temperature = nn.Parameter(torch.ones(heads, 1, 1))
        self.qkv, self.proj = nn.Linear(dim, 3 * dim), nn.Linear(dim, dim)
        self.fc1, self.fc2 = nn.Linear(dim, int(mlp_ratio * dim)), nn.Linear(int(mlp_ratio * dim), dim)
        self.conv1 = nn.Conv2d(dim, dim, 3, padding=1, groups=dim)
        self.bn = nn.BatchNorm2d(dim)
        self.conv2 = nn.Conv2d(dim, dim, 3, padding=1, groups=dim)
        self.gamma1, self.gamma2, self.gamma3 = (nn.Parameter(eta * torch.ones(dim)) for _ in range(3))
        self.heads = heads

    def forward(self, x, H, W):
        B, N, C = x.shape
        qkv = self.qkv(self.norm1(x)).reshape(B, N, 3, self.heads, C // self.heads).permute(2, 0, 3, 1, 4)
        q, k, v = (t.transpose(-2, -1) for t in (qkv[0], qkv[1], qkv[2]))
        attn = ((F.normalize(q, dim=-1) @ F.normalize(k, dim=-1).transpose(-2, -1)) * self.temperature).softmax(dim=-1)
        x = x + self.gamma1 * self.proj((attn @ v).permute(0, 3, 1, 2).reshape(B, N, C))
        g = self.norm3(x).permute(0, 2, 1).reshape(B, C, H, W)
        g = self.conv2(self.bn(F.gelu(self.conv1(g))))
        x = x + self.gamma3 * g.reshape(B, C, N).permute(0, 2, 1)
        return x + self.gamma2 * self.fc2(F.gelu(self.fc1(self.norm2(x))))


def fwd_and_both(m, call, dout):
    with torch.no_grad():
        fwd = _time(call)

    def both():
        for p in m.parameters():
            p.grad = None
        call().backward(dout)
    return round(fwd, 1), round(_time(both), 1)


def junction(B, N, D):
    """us and GB/s of the junction kernel and of the two passes it replaces (bf16 branch, fp32 residual stream)"""
    from vit_torch_amd import ops
    bf, f32 = torch.bfloat16, torch.float32
    r = lambda *s, dtype=f32: torch.randn(s, device="cuda").to(dtype)      # noqa: E731
    M = B * N
    x, b, gamma, w, bias = r(M, D), r(M, D, dtype=bf), r(D), r(D), r(D)
    a = b.view(B, N, D)[:, 0].contiguous()                # the residual pass reads row 0 of every image from here: the same values
    y1, l1, y2, l2 = (torch.empty((M, D), dtype=dt, device="cuda") for dt in (f32, bf, f32, bf))
    mean1, rstd1, mean2, rstd2 = (torch.empty(M, device="cuda") for _ in range(4))
    fused = lambda: ops.ls_residual_ln_fwd(x, b, gamma, w, bias, y1, l1, mean1, rstd1, 1e-6, M=M, D=D)      # noqa: E731
    residual = lambda: ops.ca_merge_fwd(x, a, b, gamma, y2, B, N, D)      # noqa: E731
    norm = lambda: ops.layernorm_fwd(y2, w, bias, l2, mean2, rstd2, 1e-6, M=M, D=D)      # noqa: E731

    def two():
        residual()
        norm()
    n = M * D
    out = {}
    for k, fn, nbytes in (("ls_residual_ln_fwd", fused, 12 * n), ("residual_pass", residual, 10 * n), ("layernorm_fwd", norm, 6 * n),
                          ("residual_pass+layernorm_fwd", two, 16 * n)):
        us = _time(fn)
        out[k] = {"us": round(us, 1), "GBps": round(nbytes / us / 1e3, 0)}
    torch.cuda.synchronize()
    out["max_abs_diff"] = {"y": float((y1 - y2).abs().max()), "l": float((l1.float() - l2.float()).abs().max()),
                           "mean": float((mean1 - mean2).abs().max()), "rstd": float((rstd1 - rstd2).abs().max())}
    return out


def main():
    from vit_torch_amd import XCABlock
    for name, B, side, D, heads in SHAPES:
        N = side * side
        g = torch.Generator("cuda").manual_seed(0)
        res = dict(shape=name, B=B, N=N, D=D, heads=heads)
        x, dout = torch.randn((B, N, D), device="cuda", generator=g), torch.randn((B, N, D), device="cuda", generator=g)
        m = XCABlock(D, heads, qkv_bias=True, eta=1.0, compute_dtype="bf16").cuda()
        res["block_fwd_us"], res["block_fwd_bwd_us"] = fwd_and_both(m, lambda: m(x, side, side), dout)
        c = ComposedBlock(D, heads).cuda().to(torch.bfloat16)
        xb, db = x.to(torch.bfloat16), dout.to(torch.bfloat16)
        res["composed_fwd_us"], res["composed_fwd_bwd_us"] = fwd_and_both(c, lambda: c(xb, side, side), db)
        del m, c, xb, db, x, dout
        res["junction"] = junction(B, N, D)
        print(json.dumps(res), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
