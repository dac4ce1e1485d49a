"""XCiT's cross-covariance attention (XCA), local patch interaction (LPI) and convolutional patch embedding (ConvPatchEmbed)
on libvitmi kernels.

`XCA` is the attention module of the reference's `models/xcit.py:221-261`: a qkv Linear, attention over CHANNELS
(q and k L2-normalised along the token axis, a learnable per-head temperature, a softmax over an hd x hd map per head)
and a proj Linear.  It keeps the reference's parameter names and state-dict keys (`temperature [H,1,1]`, `qkv.weight`,
`qkv.bias`, `proj.weight`, `proj.bias`), so its checkpoints load unchanged.

`LPI` is the reference's `models/xcit.py:111-141`: depthwise 3x3 conv, GELU, BatchNorm2d (`SyncBatchNorm` there), depthwise
3x3 conv on the token grid, as one fused op each way on the token-major `[B, H*W, C]` tensor (`ops.lpi_fwd` / `ops.lpi_bwd`,
`lpi.hip`): no NCHW permute.  State-dict keys and shapes are the reference's (`conv1.*`, `bn.*` with the three running
buffers, `conv2.*`), so a checkpoint's `local_mp.*` entries load unchanged.  The batch statistics are per process, which is
what `SyncBatchNorm` does in a single process; exchanging them across ranks is not built.

`ConvPatchEmbed` is the reference's `models/xcit.py:58-108`: three (patch 8) or four (patch 16) stages of Conv2d(3x3, stride
2, padding 1, no bias) + BatchNorm2d (`SyncBatchNorm` there) with GELU between them.  Each convolution is a gather
(`ops.conv3s2_im2col`, `convstem.hip`) and a product on the library's GEMM with the weight's own memory as the operand;
BatchNorm + GELU is `ops.bn_act_fwd` / `ops.bn_act_bwd`.  Activations are token-major `[B, H*W, C]` in the compute dtype from
the first stage on: no NCHW tensor exists after the image.  State-dict keys are the reference's (`proj.{0,2,4,6}.0.weight`,
`proj.{0,2,4,6}.1.*`).  Batch statistics are per process, as LPI's.  The gradient with respect to the image is not built.

The rest of XCiT (the Fourier positional encoding, XCiT's class-attention blocks, an engine) is not built.

Stand-alone modules on `engine.PackedModule`, as `ClassifierHead` is: the parameters live in a `ParamPack` (the fused
optimizers update them), forward and backward run through the mixin's one `torch.autograd.Function`; each class here
keeps its constructor, its input checks and its `_forward` / `_backward`.  XCA: `ops.gemm`, `ops.xca_fwd` /
`ops.xca_bwd` and `ops.colsum`.  compute_dtype "bf16": bf16 activations between the stages, GEMMs on the pack's bf16 weight
shadows; "fp32": everything in fp32.  LPI: bf16 or fp32 activations, every parameter and parameter gradient in fp32.
ConvPatchEmbed: bf16 or fp32 activations, the GEMMs on the bf16 weight shadows in "bf16", the norm parameters and every
gradient in fp32.  CPU tensors raise: there is no fallback.
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


class ConvPatchEmbed(PackedModule, nn.Module):
    """Image to patch embedding through stride-2 3x3 convolutions: `forward(x)` with the fp32 image x [B, 3, H, W]
    (contiguous or channels_last) returns `(tokens [B, Hp*Wp, embed_dim] fp32, (Hp, Wp))`; every stage halves the grid,
    rounding up, and `img_size` is not checked (as in the reference).  `.train()` / `.eval()` select batch or running
    statistics; in training the running buffers are updated on the device by the forward (graph-capturable).  The
    statistics are those of this process: cross-rank exchange (the reference's SyncBatchNorm under DDP) is not built.  The
    image gets no gradient: an image that requires grad is refused.  `proj` only holds the parameters and buffers under
    the reference's names; its submodules are never called.

    Kept for the backward, per stage: the stage's input (the image for the first), the conv output y as stored and stat;
    the im2col matrix is rebuilt from the input (it is 2.25x the input)."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, embed_dim=768, compute_dtype="bf16"):
        super().__init__()
        img_size = tuple(img_size) if isinstance(img_size, (tuple, list)) else (img_size, img_size)
        patch = patch_size[0] if isinstance(patch_size, (tuple, list)) else patch_size
        if compute_dtype not in ("bf16", "fp32"):
            raise VitmiError(f"ConvPatchEmbed: compute_dtype must be 'bf16' or 'fp32', got {compute_dtype!r}")
        if in_chans != 3:
            raise VitmiError(f"ConvPatchEmbed: in_chans {in_chans} is not built (the reference's stem takes 3 channels)")
        if patch not in (8, 16):
            raise VitmiError(f"ConvPatchEmbed: patch size {patch} is not built: it has to be 8 or 16")
        div = 64 if patch == 16 else 32
        if embed_dim < div or embed_dim % div:
            raise VitmiError(f"ConvPatchEmbed: embed_dim {embed_dim} must be a multiple of {div} for patch size {patch} "
                             "(every stage's channel count a multiple of 8)")
        self.img_size, self.patch_size = img_size, (patch, patch)
        self.num_patches = (img_size[1] // patch) * (img_size[0] // patch)
        self.embed_dim, self.compute_dtype = embed_dim, compute_dtype
        chans = [3] + [embed_dim // f for f in ((8, 4, 2, 1) if patch == 16 else (4, 2, 1))]
        layers = []
        for k, (ci, co) in enumerate(zip(chans[:-1], chans[1:])):
            if k:
                layers.append(nn.GELU())
            layers.append(nn.Sequential(nn.Conv2d(ci, co, kernel_size=3, stride=2, padding=1, bias=False), nn.BatchNorm2d(co)))
        self.proj = nn.Sequential(*layers)
        self.pack_shadow = compute_dtype == "bf16"        # the GEMMs read the bf16 weight shadows

    def _stages(self):
        return [(m[0], m[1]) for m in self.proj if isinstance(m, nn.Sequential)]

    def forward(self, x):
        self._refuse_cpu(x)
        if x.dim() != 4 or x.shape[1] != 3 or x.dtype != torch.float32:
            raise VitmiError(f"ConvPatchEmbed: input must be an fp32 image [B, 3, H, W], got {x.dtype} {tuple(x.shape)}")
        if x.requires_grad:
            raise VitmiError("ConvPatchEmbed: the gradient with respect to the image is not built (x.requires_grad)")
        B, _, H, W = x.shape
        for _ in self._stages():
            H, W = (H + 1) // 2, (W + 1) // 2
        if self.training and B * H * W < 2:
            raise VitmiError("ConvPatchEmbed: training needs at least two output positions (B*Hp*Wp): the batch variance "
                             "of the last stage is undefined")
        return self._run(x), (H, W)

    # ---- kernels
    def _weight(self, conv, s):
        """The k-major GEMM operand [Cout, K]: the weight's own memory, or for the first stage (K = 27) its [Cout, 32] image."""
        co, ci = conv.weight.shape[:2]
        w = self._pack.w(conv.weight).view(co, 9 * ci)
        if s:
            return w
        return ops.conv3s2_wcopy(w, torch.empty((co, 32), dtype=w.dtype, device=w.device), 27)

    ROW_CHUNK = 65535 * 64      # rows of one product: the generic GEMM kernel's grid limit (the first stage at a large batch)

    def _gemm_rows(self, A, Bm, C, **k):
        """C = A @ op(Bm), in row chunks of A and C where there are more rows than one launch takes (rows are independent)"""
        for r in range(0, A.shape[0], self.ROW_CHUNK):
            ops.gemm(A[r:r + self.ROW_CHUNK], Bm, C[r:r + self.ROW_CHUNK], **k)

    def _gemm_dw(self, dy, col, gw):
        """gw [Cout, K] = dy^T col, a sum over the M rows.  In "fp32" the sum is taken in two levels, at most 64 row chunks
        of at least 1024 rows accumulated into gw: a single fp32 accumulation over the 10^5 .. 10^6 rows of the early stages
        carries an error that grows with sqrt(M), which the two levels cut to about sqrt(M / 64) + 8.  "bf16" keeps one
        product: its operands' rounding dominates."""
        M = dy.shape[0]
        if dy.dtype != torch.float32 or M <= 1024:
            return ops.gemm(dy, col, gw, a_kmajor=False, b_kmajor=False)
        R = max(1024, (-(-M // 64) + 63) // 64 * 64)
        for r in range(0, M, R):
            ops.gemm(dy[r:r + R], col[r:r + R], gw, a_kmajor=False, b_kmajor=False, accumulate=r > 0)
        return gw

    def _forward(self, x, save):
        pk = self._pack
        dt = torch.bfloat16 if self.compute_dtype == "bf16" else torch.float32
        pk.refresh_shadow()
        B, _, h, w = x.shape
        stages = self._stages()
        cur, saved = x, []
        for s, (conv, bn) in enumerate(stages):
            co, ci = conv.weight.shape[:2]
            ho, wo = (h + 1) // 2, (w + 1) // 2
            M = B * ho * wo
            col = torch.empty((M, 9 * ci if s else 32), dtype=dt, device=x.device)
            ops.conv3s2_im2col(cur, col, B, h, w, ci)
            y = torch.empty((M, co), dtype=dt, device=x.device)
            self._gemm_rows(col, self._weight(conv, s), y)
            del col
            stat = torch.empty((2, co), dtype=torch.float32, device=x.device)
            out = torch.empty((B, ho * wo, co), dtype=dt, device=x.device)
            ops.bn_act_fwd(y, pk.f32(bn.weight), pk.f32(bn.bias), bn.running_mean, bn.running_var, bn.num_batches_tracked,
                           stat, out, M, co, gelu=s + 1 < len(stages), training=self.training, momentum=bn.momentum,
                           eps=bn.eps)
            saved.append((cur, y, stat, (h, w)))
            cur, h, w = out, ho, wo
        if save:
            self._saved = (saved, self.training, B)
        if dt == torch.float32:
            return cur
        return ops.cast(cur, torch.empty(cur.shape, dtype=torch.float32, device=x.device))

    def _backward(self, dout, need_dx):
        saved, training, B = self._take_saved()
        pk, stages = self._pack, self._stages()
        dt = saved[0][1].dtype
        d = dout.reshape(-1, self.embed_dim).to(dt).contiguous()
        for s in range(len(stages) - 1, -1, -1):
            conv, bn = stages[s]
            inp, y, stat, (h, w) = saved[s]
            co, ci = conv.weight.shape[:2]
            M = y.shape[0]
            dy = torch.empty_like(y)
            ops.bn_act_bwd(d.view(M, co), y, stat, pk.f32(bn.weight), pk.f32(bn.bias), dy, pk.g(bn.weight), pk.g(bn.bias), M, co,
                           gelu=s + 1 < len(stages), training=training)
            col = torch.empty((M, 9 * ci if s else 32), dtype=dt, device=y.device)
            ops.conv3s2_im2col(inp, col, B, h, w, ci)
            if s == 0:
                gimg = torch.empty((co, 32), dtype=torch.float32, device=y.device)
                self._gemm_dw(dy, col, gimg)
                ops.conv3s2_wcopy(gimg, pk.g(conv.weight).view(co, 27), 27)
                break
            self._gemm_dw(dy, col, pk.g(conv.weight).view(co, 9 * ci))
            self._gemm_rows(dy, pk.w(conv.weight).view(co, 9 * ci), col, b_kmajor=False)    # dcol, over col: it is done with
            d = torch.empty((B * h * w, ci), dtype=dt, device=y.device)
            ops.conv3s2_col2im(col, d, B, h, w, ci)
        return None
