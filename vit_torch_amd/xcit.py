"""XCiT's cross-covariance attention (XCA) and local patch interaction (LPI) on libvitmi kernels.

`XCA` is the attention module of the reference's `models/xcit.py:221-261`: a qkv Linear, attention over CHANNELS
(q and k L2-normalised along the token axis, a learnable per-head temperature, a softmax over an hd x hd map per head)
and a proj Linear.  It keeps the reference's parameter names and state-dict keys (`temperature [H,1,1]`, `qkv.weight`,
`qkv.bias`, `proj.weight`, `proj.bias`), so its checkpoints load unchanged.

`LPI` is the reference's `models/xcit.py:111-141`: depthwise 3x3 conv, GELU, BatchNorm2d (`SyncBatchNorm` there), depthwise
3x3 conv on the token grid, as one fused op each way on the token-major `[B, H*W, C]` tensor (`ops.lpi_fwd` / `ops.lpi_bwd`,
`lpi.hip`): no NCHW permute.  State-dict keys and shapes are the reference's (`conv1.*`, `bn.*` with the three running
buffers, `conv2.*`), so a checkpoint's `local_mp.*` entries load unchanged.  The batch statistics are per process, which is
what `SyncBatchNorm` does in a single process; exchanging them across ranks is not built.

The rest of XCiT (ConvPatchEmbed, the Fourier positional encoding, XCiT's class-attention blocks, an engine) is not built.

Stand-alone modules on `engine.PackedModule`, as `ClassifierHead` is: the parameters live in a `ParamPack` (the fused
optimizers update them), forward and backward run through the mixin's one `torch.autograd.Function`; each class here
keeps its constructor, its input checks and its `_forward` / `_backward`.  XCA: `ops.gemm`, `ops.xca_fwd` /
`ops.xca_bwd` and `ops.colsum`.  compute_dtype "bf16": bf16 activations between the stages, GEMMs on the pack's bf16 weight
shadows; "fp32": everything in fp32.  LPI: bf16 or fp32 activations, every parameter and parameter gradient in fp32.  CPU
tensors raise: there is no fallback.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import ops
from ._lib import VitmiError
from .engine import PackedModule


class XCA(PackedModule, nn.Module):
    def __init__(self, dim, num_heads=8, qkv_bias=False, qk_scale=None, attn_drop=0., proj_drop=0., compute_dtype="bf16"):
        super().__init__()
        if attn_drop != 0. or proj_drop != 0.:
            raise VitmiError("XCA: dropout is not built (the reference's XCiT factories use attn_drop = proj_drop = 0)")
        if compute_dtype not in ("bf16", "fp32"):
            raise VitmiError(f"XCA: compute_dtype must be 'bf16' or 'fp32', got {compute_dtype!r}")
        if dim % num_heads or dim // num_heads not in (32, 48, 64):
            raise VitmiError(f"XCA: head dim {dim}/{num_heads} not in {{32, 48, 64}}")
        self.dim, self.num_heads, self.compute_dtype = dim, num_heads, compute_dtype
        self.temperature = nn.Parameter(torch.ones(num_heads, 1, 1))
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)
        self.pack_shadow = compute_dtype == "bf16"        # the GEMMs read the bf16 weight shadows

    def no_weight_decay(self):
        return {"temperature"}

    def forward(self, x):
        self._refuse_cpu(x)
        if x.dim() != 3 or x.shape[-1] != self.dim:
            raise VitmiError(f"XCA: input must be [B, N, {self.dim}], got {tuple(x.shape)}")
        return self._run(x)

    # ---- kernels
    def _forward(self, x, save):
        B, N, C = x.shape
        H, hd, pk = self.num_heads, C // self.num_heads, self._pack
        dt = torch.bfloat16 if self.compute_dtype == "bf16" else torch.float32
        pk.refresh_shadow()
        xa = x.reshape(B * N, C).to(dt).contiguous()
        qkv = torch.empty((B * N, 3 * C), dtype=dt, device=x.device)
        ops.gemm(xa, pk.w(self.qkv.weight), qkv, bias=pk.f32(self.qkv.bias) if self.qkv.bias is not None else None)
        att = torch.empty((B * N, C), dtype=dt, device=x.device)
        stat = torch.empty((B, H, hd + 2, hd), dtype=torch.float32, device=x.device)
        ops.xca_fwd(qkv, pk.f32(self.temperature).view(H), att, stat, B, N, H, hd)
        y = torch.empty((B * N, C), dtype=torch.float32, device=x.device)
        ops.gemm(att, pk.w(self.proj.weight), y, bias=pk.f32(self.proj.bias))
        if save:
            self._saved = (xa, qkv, att, stat, (B, N))
        return y.view(B, N, C)

    def _backward(self, dout, need_dx):
        xa, qkv, att, stat, (B, N) = self._take_saved()
        C, H, pk = self.dim, self.num_heads, self._pack
        hd, dt = C // H, xa.dtype
        dy = dout.reshape(B * N, C).to(dt).contiguous()
        ops.gemm(dy, att, pk.g(self.proj.weight), a_kmajor=False, b_kmajor=False)
        ops.colsum(dy, pk.g(self.proj.bias))
        datt = torch.empty((B * N, C), dtype=dt, device=dy.device)
        ops.gemm(dy, pk.w(self.proj.weight), datt, b_kmajor=False)
        dqkv = torch.empty_like(qkv)
        ops.xca_bwd(qkv, datt, pk.f32(self.temperature).view(H), stat, dqkv, pk.g(self.temperature).view(H), B, N, H, hd)
        ops.gemm(dqkv, xa, pk.g(self.qkv.weight), a_kmajor=False, b_kmajor=False)
        if self.qkv.bias is not None:
            ops.colsum(dqkv, pk.g(self.qkv.bias))
        if not need_dx:
            return None
        dx = torch.empty((B * N, C), dtype=torch.float32, device=dy.device)
        ops.gemm(dqkv, pk.w(self.qkv.weight), dx, b_kmajor=False)
        return dx.view(B, N, C)


class LPI(PackedModule, nn.Module):
    """Local patch interaction, `forward(x, H, W)` with x [B, H*W, C].  `.train()` / `.eval()` select batch or running
    statistics; in training the running buffers are updated on the device by the forward (graph-capturable).  The
    statistics are those of this process: cross-rank exchange (the reference's SyncBatchNorm under DDP) is not built.
    `conv1`, `bn`, `conv2` only hold the parameters and buffers under the reference's names; they are never called."""

    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0., kernel_size=3,
                 compute_dtype="bf16"):
        super().__init__()
        out_features = out_features or in_features
        if out_features != in_features:
            raise VitmiError(f"LPI: out_features {out_features} != in_features {in_features} (depthwise: they must be equal)")
        if kernel_size != 3:
            raise VitmiError(f"LPI: kernel_size {kernel_size} is not built (the reference uses 3)")
        if act_layer is not nn.GELU:
            raise VitmiError("LPI: only nn.GELU (erf form) is built as the activation")
        if drop != 0.:
            raise VitmiError("LPI: dropout is not built (the reference's LPI ignores drop)")
        if compute_dtype not in ("bf16", "fp32"):
            raise VitmiError(f"LPI: compute_dtype must be 'bf16' or 'fp32', got {compute_dtype!r}")
        if in_features < 8 or in_features % 8:
            raise VitmiError(f"LPI: C = {in_features} must be a multiple of 8")
        self.dim, self.compute_dtype = in_features, compute_dtype
        self.conv1 = nn.Conv2d(in_features, out_features, kernel_size=3, padding=1, groups=out_features)
        self.act = act_layer()
        self.bn = nn.BatchNorm2d(in_features)
        self.conv2 = nn.Conv2d(in_features, out_features, kernel_size=3, padding=1, groups=out_features)

    def forward(self, x, H, W):
        self._refuse_cpu(x)
        if x.dim() != 3 or x.shape[-1] != self.dim:
            raise VitmiError(f"LPI: input must be [B, H*W, {self.dim}], got {tuple(x.shape)}")
        if x.shape[1] != H * W:
            raise VitmiError(f"LPI: {x.shape[1]} tokens are not an H x W = {H} x {W} grid")
        return self._run(x, H, W)

    # ---- kernels
    def _forward(self, x, H, W, save):
        B, N, C = x.shape
        pk, bn = self._pack, self.bn
        dt = torch.bfloat16 if self.compute_dtype == "bf16" else torch.float32
        xa = x.to(dt).contiguous()
        u = torch.empty_like(xa)
        out = torch.empty_like(xa)
        stat = torch.empty((2, C), dtype=torch.float32, device=x.device)
        ops.lpi_fwd(xa, pk.f32(self.conv1.weight), pk.f32(self.conv1.bias), pk.f32(bn.weight), pk.f32(bn.bias),
                    pk.f32(self.conv2.weight), pk.f32(self.conv2.bias), bn.running_mean, bn.running_var,
                    bn.num_batches_tracked, u, stat, out, B, H, W, C, training=self.training,
                    momentum=bn.momentum, eps=bn.eps)
        if save:
            self._saved = (xa, u, stat, self.training, (B, H, W), x.dtype)
        return out.to(x.dtype)

    def _backward(self, dout, need_dx):
        xa, u, stat, training, (B, H, W), xdt = self._take_saved()
        C, pk, bn = self.dim, self._pack, self.bn
        dy = dout.to(xa.dtype).contiguous()
        dx = torch.empty_like(xa)
        ops.lpi_bwd(xa, u, dy, stat, pk.f32(self.conv1.weight), pk.f32(self.conv1.bias), pk.f32(bn.weight), pk.f32(bn.bias),
                    pk.f32(self.conv2.weight), dx, pk.g(self.conv1.weight), pk.g(self.conv1.bias), pk.g(bn.weight),
                    pk.g(bn.bias), pk.g(self.conv2.weight), pk.g(self.conv2.bias), B, H, W, C, training=training)
        return dx.to(xdt) if need_dx else None
