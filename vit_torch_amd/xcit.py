"""XCiT's cross-covariance attention (XCA), local patch interaction (LPI), convolutional patch embedding (ConvPatchEmbed),
Fourier positional encoding (PositionalEncodingFourier), class-attention block (ClassAttentionBlock) and trunk block (XCABlock)
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

`PositionalEncodingFourier` is the reference's `models/xcit.py:20-55` as `XCiT.forward_features` uses it: `x + pos` on the
token-major tensor.  A sin / cos feature table for one image (`ops.posfourier_features`, `xcit_glue.hip`; cached, it depends
on no parameter), its 1x1-conv projection as a product on the library's GEMM with the conv weight's own memory as the operand,
and an add that broadcasts over the batch (`ops.add_rows_bcast`).  State-dict keys are the reference's
(`token_projection.weight [dim, 64, 1, 1]`, `token_projection.bias`).

`ClassAttentionBlock` is the reference's `models/xcit.py:144-218` (its `ClassAttention` inside): LayerNorm, class attention
(one query per head over all tokens: `ops.class_attn_fwd` / `class_attn_bwd`, reading k and v in place), LayerScale residual,
LayerNorm on every token or on the CLS token only (`tokens_norm`), an MLP on the CLS token, and the reference's last line,
which doubles the patch rows.  The element-wise steps between the GEMMs are the `ops.ca_*` kernels (`xcit_glue.hip`).
State-dict keys are the reference's (`norm1.*`, `attn.qkv.*`, `attn.proj.*`, `norm2.*`, `mlp.fc1.*`, `mlp.fc2.*`, `gamma1`,
`gamma2`).

`XCABlock` is the reference's `models/xcit.py:264-292`, the block of XCiT's trunk: `x + gamma1 * attn(norm1(x))`, `x + gamma3 *
local_mp(norm3(x), H, W)`, `x + gamma2 * mlp(norm2(x))`.  One module with one pack on the XCA and LPI kernels (it does not nest
the `XCA` and `LPI` modules), LayerNorm and the GEMMs: the attention and MLP branches end in a Linear, so the product's
`EPI_RESIDUAL` epilogue does their LayerScale residual; the LPI branch ends in no product, and its residual and the norm2 that
reads the sum are one kernel (`ops.ls_residual_ln_fwd`, `layernorm.hip`).  The backward uses existing ops only.  State-dict
keys, shapes and order are the reference's (`gamma1`, `gamma2`, `gamma3`, `norm1.*`, `attn.temperature`, `attn.qkv.*`,
`attn.proj.*`, `norm2.*`, `mlp.fc1.*`, `mlp.fc2.*`, `norm3.*`, `local_mp.conv1.*`, `local_mp.bn.*` with the three running
buffers, `local_mp.conv2.*`).

Of XCiT, the model that stacks these modules, its engine and its zoo entries are not built.

Stand-alone modules on `engine.PackedModule`, as `ClassifierHead` is: the parameters live in a `ParamPack` (the fused
optimizers update them), forward and backward run through the mixin's one `torch.autograd.Function`; each class here
keeps its constructor, its input checks and its `_forward` / `_backward`.  XCA: `ops.gemm`, `ops.xca_fwd` /
`ops.xca_bwd` and `ops.colsum`.  compute_dtype "bf16": bf16 activations between the stages, GEMMs on the pack's bf16 weight
shadows; "fp32": everything in fp32.  LPI: bf16 or fp32 activations, every parameter and parameter gradient in fp32.
ConvPatchEmbed: bf16 or fp32 activations, the GEMMs on the bf16 weight shadows in "bf16", the norm parameters and every
gradient in fp32.  PositionalEncodingFourier: the feature table and the GEMM operands in the compute dtype, the encoding,
the sum and every gradient in fp32.  ClassAttentionBlock: the residual stream in fp32, the branch tensors and GEMM operands
in the compute dtype.  XCABlock: the same.  CPU tensors raise: there is no fallback.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import ops
from ._lib import EPI_BIAS_GELU, EPI_DGELU, EPI_RESIDUAL, VitmiError
from .engine import PackedModule


def _gemm_dw(dy, col, gw, min_rows=1024):
    """gw [Cout, K] = dy^T col, a sum over the M rows.  In "fp32" the sum is taken in two levels, at most 64 row chunks
    of at least `min_rows` rows accumulated into gw: a single fp32 accumulation over the 10^4 .. 10^6 rows of the conv stem's
    early stages or of a batch of token rows carries an error that grows with sqrt(M), which the two levels cut to about
    sqrt(M / 64) + 8.  "bf16" keeps one product: its operands' rounding dominates."""
    M = dy.shape[0]
    if dy.dtype != torch.float32 or M <= min_rows:
        return ops.gemm(dy, col, gw, a_kmajor=False, b_kmajor=False)
    R = max(min_rows, (-(-M // 64) + 63) // 64 * 64)
    for r in range(0, M, R):
        ops.gemm(dy[r:r + R], col[r:r + R], gw, a_kmajor=False, b_kmajor=False, accumulate=r > 0)
    return gw


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
                _gemm_dw(dy, col, gimg)
                ops.conv3s2_wcopy(gimg, pk.g(conv.weight).view(co, 27), 27)
                break
            _gemm_dw(dy, col, pk.g(conv.weight).view(co, 9 * ci))
            self._gemm_rows(dy, pk.w(conv.weight).view(co, 9 * ci), col, b_kmajor=False)    # dcol, over col: it is done with
            d = torch.empty((B * h * w, ci), dtype=dt, device=y.device)
            ops.conv3s2_col2im(col, d, B, h, w, ci)
        return None


class PositionalEncodingFourier(PackedModule, nn.Module):
    """`forward(x, H, W)` with x [B, H*W, dim] returns `x + pos` in fp32, pos [H*W, dim] being the reference's encoding of an
    H x W grid: how `XCiT.forward_features` uses it (`x = x + pos_embeder(B, Hp, Wp).reshape(B, -1, N).permute(0, 2, 1)`).
    The reference's own `forward(B, H, W) -> [B, dim, H, W]` would materialise B identical NCHW copies of the encoding and is
    not built.  `table(H, W)` returns the fp32 encoding [H*W, dim] under no_grad.  `token_projection` only holds the
    parameters under the reference's names; it is never called.  x gets `dx = dout` (the same tensor).

    Kept for the backward: nothing but the grid; the feature table is cached per (H, W, dtype, device)."""

    def __init__(self, hidden_dim=32, dim=768, temperature=10000, compute_dtype="bf16"):
        super().__init__()
        if compute_dtype not in ("bf16", "fp32"):
            raise VitmiError(f"PositionalEncodingFourier: compute_dtype must be 'bf16' or 'fp32', got {compute_dtype!r}")
        if hidden_dim != 32:
            raise VitmiError(f"PositionalEncodingFourier: hidden_dim {hidden_dim} is not built (the reference's XCiT uses 32)")
        if dim < 8 or dim % 8:
            raise VitmiError(f"PositionalEncodingFourier: dim = {dim} must be a multiple of 8")
        if not temperature > 0:
            raise VitmiError(f"PositionalEncodingFourier: the temperature must be positive, got {temperature}")
        self.token_projection = nn.Conv2d(hidden_dim * 2, dim, kernel_size=1)
        self.hidden_dim, self.dim, self.temperature, self.compute_dtype = hidden_dim, dim, temperature, compute_dtype
        self.pack_shadow = compute_dtype == "bf16"        # the projection reads the bf16 weight shadow
        self._tables = {}

    def _check(self, x, H, W):
        self._refuse_cpu(x)
        if x.dim() != 3 or x.shape[-1] != self.dim:
            raise VitmiError(f"PositionalEncodingFourier: input must be [B, H*W, {self.dim}], got {tuple(x.shape)}")
        if H < 1 or W < 1 or x.shape[1] != H * W:
            raise VitmiError(f"PositionalEncodingFourier: {x.shape[1]} tokens are not an H x W = {H} x {W} grid")

    def forward(self, x, H, W):
        self._check(x, H, W)
        return self._run(x, H, W)

    def table(self, H, W):
        """the encoding [H*W, dim] in fp32 (no gradient)"""
        self.engine()
        with torch.no_grad():
            return self._pos(H, W, self._pack.params[0].device)

    # ---- kernels
    def _features(self, H, W, dev):
        dt = torch.bfloat16 if self.compute_dtype == "bf16" else torch.float32
        key = (H, W, dt, str(dev))
        f = self._tables.get(key)
        if f is None:
            f = torch.empty((H * W, 2 * self.hidden_dim), dtype=dt, device=dev)
            ops.posfourier_features(f, H, W, self.hidden_dim, self.temperature)
            self._tables[key] = f
        return f

    def _pos(self, H, W, dev):
        pk, tp = self._pack, self.token_projection
        pk.refresh_shadow()
        pos = torch.empty((H * W, self.dim), dtype=torch.float32, device=dev)
        return ops.gemm(self._features(H, W, dev), pk.w(tp.weight).view(self.dim, 2 * self.hidden_dim), pos, bias=pk.f32(tp.bias))

    def _forward(self, x, H, W, save):
        B, N, C = x.shape
        xa = x.float().contiguous()
        out = ops.add_rows_bcast(xa, self._pos(H, W, x.device), torch.empty_like(xa), B, N, C)
        if save:
            self._saved = (H, W)
        return out

    def _backward(self, dout, need_dx):
        H, W = self._take_saved()
        pk, tp, C = self._pack, self.token_projection, self.dim
        d = dout.float().contiguous()
        B, N = d.shape[0], H * W
        dpos = torch.empty((N, C), dtype=torch.float32, device=d.device)
        ops.colsum(d, dpos, M=B, N=N * C)
        ops.colsum(dpos, pk.g(tp.bias), M=N, N=C)
        feat = self._features(H, W, d.device)
        dp = dpos if feat.dtype == torch.float32 else ops.cast(dpos, torch.empty_like(dpos, dtype=feat.dtype))
        ops.gemm(dp, feat, pk.g(tp.weight).view(C, 2 * self.hidden_dim), a_kmajor=False, b_kmajor=False)
        return dout if need_dx else None


class _ParamHolder(nn.Module):
    """holds parameters, buffers and layers under the reference's names; never called"""

    def forward(self, *a, **k):
        raise VitmiError("this submodule only holds parameters; call the block that owns it")


class ClassAttentionBlock(PackedModule, nn.Module):
    """XCiT's class-attention block: `forward(x, H, W, mask=None)` with x [B, 1 + Np, dim], CLS first, returns the fp32
    [B, 1 + Np, dim] tensor of the reference's block; H, W and mask are accepted and unused, as there.  The patch rows do
    change: they receive `x + gamma1 * norm1(x)`, are normed by norm2 if `tokens_norm`, and are doubled by the block's last
    line.  `attn` (`qkv`, `proj`) and `mlp` (`fc1`, `fc2`) only hold parameters under the reference's names.  The reference
    computes q for every token and uses the CLS row's only, so q is computed for the CLS rows alone; the patch rows' share of
    the q weight gradient is exactly zero.

    Kept for the backward: x (fp32), l = norm1(x) and [k v] (compute dtype, all rows), both norms' statistics, x1 (fp32),
    and per image: q, the attention output, its softmax, the projected CLS token a, the normed CLS row, the MLP's
    pre-activation (its gelu' in "bf16") and hidden row, and m = mlp(cls)."""

    def __init__(self, dim, num_heads, mlp_ratio=4., qkv_bias=False, qk_scale=None, drop=0., attn_drop=0., drop_path=0.,
                 act_layer=nn.GELU, norm_layer=nn.LayerNorm, eta=None, tokens_norm=False, compute_dtype="bf16"):
        super().__init__()
        if compute_dtype not in ("bf16", "fp32"):
            raise VitmiError(f"ClassAttentionBlock: compute_dtype must be 'bf16' or 'fp32', got {compute_dtype!r}")
        if drop != 0. or attn_drop != 0. or drop_path != 0.:
            raise VitmiError("ClassAttentionBlock: dropout and drop_path are not built")
        if act_layer is not nn.GELU:
            raise VitmiError("ClassAttentionBlock: only nn.GELU (erf form) is built as the activation")
        if eta is None:
            raise VitmiError("ClassAttentionBlock: eta=None (no LayerScale) is not built: every XCiT factory of the reference "
                             "passes an eta")
        if dim % num_heads or dim // num_heads > 64 or (dim // num_heads) % 8:
            raise VitmiError(f"ClassAttentionBlock: head dim {dim}/{num_heads} must be a multiple of 8, at most 64")
        self.dim, self.num_heads, self.compute_dtype, self.tokens_norm = dim, num_heads, compute_dtype, tokens_norm
        self.scale = qk_scale or (dim // num_heads) ** -0.5
        self.norm1 = norm_layer(dim)
        self.attn = _ParamHolder()
        self.attn.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.attn.proj = nn.Linear(dim, dim)
        self.norm2 = norm_layer(dim)
        self.mlp = _ParamHolder()
        self.mlp.fc1 = nn.Linear(dim, int(dim * mlp_ratio))
        self.mlp.fc2 = nn.Linear(int(dim * mlp_ratio), dim)
        for n in (self.norm1, self.norm2):
            if not isinstance(n, nn.LayerNorm) or not n.elementwise_affine or tuple(n.normalized_shape) != (dim,):
                raise VitmiError("ClassAttentionBlock: norm_layer must build an affine nn.LayerNorm over dim")
        if int(dim * mlp_ratio) < 8 or int(dim * mlp_ratio) % 8:
            raise VitmiError(f"ClassAttentionBlock: the MLP's hidden width {int(dim * mlp_ratio)} must be a multiple of 8")
        self.gamma1 = nn.Parameter(eta * torch.ones(dim))
        self.gamma2 = nn.Parameter(eta * torch.ones(dim))
        self.pack_shadow = compute_dtype == "bf16"        # the GEMMs read the bf16 weight shadows

    MAX_TOKENS = 1025       # ops.class_attn_fwd / class_attn_bwd

    def forward(self, x, H, W, mask=None):
        self._refuse_cpu(x)
        if x.dim() != 3 or x.shape[-1] != self.dim or x.shape[1] < 2:
            raise VitmiError(f"ClassAttentionBlock: input must be [B, 1 + Np, {self.dim}] with at least one patch, got "
                             f"{tuple(x.shape)}")
        if x.shape[1] > self.MAX_TOKENS:
            raise VitmiError(f"ClassAttentionBlock: {x.shape[1]} tokens: the class-attention kernels take at most {self.MAX_TOKENS}")
        return self._run(x)

    # ---- kernels
    def _forward(self, x, save):
        B, N1, D = x.shape
        H, hd, pk, M = self.num_heads, D // self.num_heads, self._pack, B * N1
        a_, mlp, dev, f32 = self.attn, self.mlp, x.device, torch.float32
        T = torch.bfloat16 if self.compute_dtype == "bf16" else f32
        new = lambda *shape, dtype=T: torch.empty(shape, dtype=dtype, device=dev)      # noqa: E731
        pk.refresh_shadow()
        xa = x.float().contiguous()
        l, mean1, rstd1 = new(M, D), new(M, dtype=f32), new(M, dtype=f32)
        ops.layernorm_fwd(xa, pk.f32(self.norm1.weight), pk.f32(self.norm1.bias), l, mean1, rstd1, self.norm1.eps, M=M, D=D)
        Wqkv, bqkv = pk.w(a_.qkv.weight), (pk.f32(a_.qkv.bias) if a_.qkv.bias is not None else None)
        kv = new(M, 2 * D)
        ops.gemm(l, Wqkv[D:], kv, bias=bqkv[D:] if bqkv is not None else None)
        q = new(B, D)
        ops.gemm(l.view(B, N1 * D)[:, :D], Wqkv[:D], q, bias=bqkv[:D] if bqkv is not None else None)
        o, psave = new(B, D), new(B * H * N1, dtype=f32)
        ops.class_attn_fwd(q, kv, kv[:, D:], 2 * D, o, psave, B, H, N1, hd, self.scale)
        a = new(B, D)
        ops.gemm(o, pk.w(a_.proj.weight), a, bias=pk.f32(a_.proj.bias))
        x1 = ops.ca_merge_fwd(xa, a, l, pk.f32(self.gamma1), new(B, N1, D, dtype=f32), B, N1, D)
        g2, b2 = pk.f32(self.norm2.weight), pk.f32(self.norm2.bias)
        if self.tokens_norm:
            x2, mean2, rstd2 = new(B, N1, D, dtype=f32), new(M, dtype=f32), new(M, dtype=f32)
            ops.layernorm_fwd(x1, g2, b2, x2, mean2, rstd2, self.norm2.eps, M=M, D=D)
            xc, xp = x2.view(B, N1 * D)[:, :D], x2
        else:
            xc, mean2, rstd2 = new(B, D, dtype=f32), new(B, dtype=f32), new(B, dtype=f32)
            ops.layernorm_fwd(x1, g2, b2, xc, mean2, rstd2, self.norm2.eps, M=B, D=D, x_stride=N1 * D)
            xp = x1
        # the MLP's operand: the normed CLS rows, compact, in the compute dtype (kept for the fc1 weight gradient)
        xcT = xc if T == f32 and not self.tokens_norm else ops.scale_cast(xc, new(B, D), M=B, N=D, ldx=N1 * D if self.tokens_norm else D)
        Dh = mlp.fc1.out_features
        pre = new(B, Dh) if save else None
        hid = new(B, Dh)
        ops.gemm(xcT, pk.w(mlp.fc1.weight), hid, epilogue=EPI_BIAS_GELU, bias=pk.f32(mlp.fc1.bias), C2=pre,
                 aux_deriv=T == torch.bfloat16)
        m = new(B, D)
        ops.gemm(hid, pk.w(mlp.fc2.weight), m, bias=pk.f32(mlp.fc2.bias))
        out = ops.ca_out_fwd(xc, xp, m, pk.f32(self.gamma2), new(B, N1, D, dtype=f32), B, N1, D)
        if save:
            self._saved = (xa, l, mean1, rstd1, kv, q, o, psave, a, x1, mean2, rstd2, xcT, pre, hid, m)
        return out

    def _backward(self, dout, need_dx):
        xa, l, mean1, rstd1, kv, q, o, psave, a, x1, mean2, rstd2, xcT, pre, hid, m = self._take_saved()
        B, N1, D = xa.shape
        H, hd, pk, M = self.num_heads, D // self.num_heads, self._pack, B * N1
        a_, mlp, dev, f32, T = self.attn, self.mlp, xa.device, torch.float32, l.dtype
        new = lambda *shape, dtype=T: torch.empty(shape, dtype=dtype, device=dev)      # noqa: E731
        G = dout.float().contiguous()
        Gc = G.view(B, N1 * D)[:, :D]                       # the CLS rows, strided
        # the last line and the MLP on B rows
        dx2, gm = new(B, N1, D, dtype=f32), new(B, D)
        ops.ca_out_bwd(G, pk.f32(self.gamma2), dx2, gm, B, N1, D)
        ops.colsum_mul(Gc, m, pk.g(self.gamma2), M=B, N=D, ldx=N1 * D, ldy=D)
        Dh = mlp.fc1.out_features
        dH = new(B, Dh)
        ops.gemm(gm, pk.w(mlp.fc2.weight), dH, b_kmajor=False, epilogue=EPI_DGELU, aux=pre, aux_deriv=T == torch.bfloat16)
        ops.gemm(gm, hid, pk.g(mlp.fc2.weight), a_kmajor=False, b_kmajor=False)
        ops.colsum(gm, pk.g(mlp.fc2.bias))
        ops.gemm(dH, xcT, pk.g(mlp.fc1.weight), a_kmajor=False, b_kmajor=False)
        ops.colsum(dH, pk.g(mlp.fc1.bias))
        dx2c = dx2.view(B, N1 * D)[:, :D]
        ops.gemm(dH, pk.w(mlp.fc1.weight), dx2c, b_kmajor=False, accumulate=True)          # dx2_c = G_c + the MLP's gradient
        # norm2
        g2w, gg2, gb2 = pk.f32(self.norm2.weight), pk.g(self.norm2.weight), pk.g(self.norm2.bias)
        if self.tokens_norm:
            dx1 = new(B, N1, D, dtype=f32)
            ops.layernorm_bwd(dx2, x1, mean2, rstd2, g2w, None, dx1, None, gg2, gb2, M=M, D=D)
        else:
            dyc = ops.scale_cast(dx2c, new(B, D, dtype=f32), M=B, N=D, ldx=N1 * D)
            ops.layernorm_bwd(dyc, x1, mean2, rstd2, g2w, None, dx2, None, gg2, gb2, M=B, D=D, x_stride=N1 * D,
                              g_stride=N1 * D)                                            # over the CLS rows of dx2; dx1_p = dx2_p
            dx1 = dx2
        # the first residual's branch
        da, dl = new(B, D), new(B, N1, D, dtype=f32)
        ops.ca_merge_bwd(dx1, l, a, pk.f32(self.gamma1), da, dl, pk.g(self.gamma1), B, N1, D)
        ops.gemm(da, o, pk.g(a_.proj.weight), a_kmajor=False, b_kmajor=False)
        ops.colsum(da, pk.g(a_.proj.bias))
        do = new(B, D)
        ops.gemm(da, pk.w(a_.proj.weight), do, b_kmajor=False)
        dq, dkv = new(B, D), new(M, 2 * D)
        ops.class_attn_bwd(q, kv, kv[:, D:], 2 * D, do, psave, dq, dkv, dkv[:, D:], 2 * D, B, H, N1, hd, self.scale)
        Wqkv, gW = pk.w(a_.qkv.weight), pk.g(a_.qkv.weight)
        lc = l.view(B, N1 * D)[:, :D]
        _gemm_dw(dkv, l, gW[D:], min_rows=256)                       # over all B*N1 rows: two levels in "fp32"
        ops.gemm(dq, lc, gW[:D], a_kmajor=False, b_kmajor=False)
        if a_.qkv.bias is not None:
            gb = pk.g(a_.qkv.bias)
            ops.colsum(dkv, gb[D:])
            ops.colsum(dq, gb[:D])
        dlm = dl.view(M, D)
        ops.gemm(dkv, Wqkv[D:], dlm, b_kmajor=False, accumulate=True)
        ops.gemm(dq, Wqkv[:D], dl.view(B, N1 * D)[:, :D], b_kmajor=False, accumulate=True)
        # norm1 (its parameter gradients are needed whether or not dx is): dx = dx1 + LN1bwd(dl), in place over dx1
        ops.layernorm_bwd(dlm, xa, mean1, rstd1, pk.f32(self.norm1.weight), dx1, dx1, None, pk.g(self.norm1.weight),
                          pk.g(self.norm1.bias), M=M, D=D)
        return dx1 if need_dx else None


class XCABlock(PackedModule, nn.Module):
    """XCiT's trunk block: `forward(x, H, W)` with x [B, H*W, dim] returns the fp32 [B, H*W, dim] tensor of the reference's
    block, three LayerScale residual branches: cross-covariance attention, local patch interaction on the H x W grid, MLP.
    `num_tokens` and `qk_scale` are accepted and unused, as there.  `attn` (`temperature`, `qkv`, `proj`), `mlp` (`fc1`,
    `fc2`) and `local_mp` (`conv1`, `bn`, `conv2`) only hold the parameters and buffers under the reference's names.
    `.train()` / `.eval()` select batch or running statistics for the LPI's batch norm; in training the forward updates
    the running buffers on the device, as `LPI` does (per process: no cross-rank exchange).

    Kept for the backward: x, x1, x2 (fp32), the three norms' statistics, and in the compute dtype l1 = norm1(x), qkv, the
    attention output and its stat, f1 = proj(...), l3 = norm3(x1), the LPI's u and stat, p = lpi(l3), l2 = norm2(x2), the
    MLP's pre-activation (its gelu' in "bf16"), the hidden rows and f2 = fc2(...)."""

    def __init__(self, dim, num_heads, mlp_ratio=4., qkv_bias=False, qk_scale=None, drop=0., attn_drop=0., drop_path=0.,
                 act_layer=nn.GELU, norm_layer=nn.LayerNorm, num_tokens=196, eta=None, compute_dtype="bf16"):
        super().__init__()
        if compute_dtype not in ("bf16", "fp32"):
            raise VitmiError(f"XCABlock: compute_dtype must be 'bf16' or 'fp32', got {compute_dtype!r}")
        for name, v in (("drop", drop), ("attn_drop", attn_drop), ("drop_path", drop_path)):
            if v != 0.:
                raise VitmiError(f"XCABlock: {name} = {v} is not built (dropout and drop_path: the kernels have no mask)")
        if act_layer is not nn.GELU:
            raise VitmiError("XCABlock: only nn.GELU (erf form) is built as the activation")
        if eta is None:
            raise VitmiError("XCABlock: eta=None is not built: the reference's own constructor fails on it (eta * ones)")
        if dim % num_heads or dim // num_heads not in (32, 48, 64):
            raise VitmiError(f"XCABlock: head dim {dim}/{num_heads} not in {{32, 48, 64}} (the XCA kernels' limit)")
        hidden = int(dim * mlp_ratio)
        if dim % 8 or hidden < 8 or hidden % 8:
            raise VitmiError(f"XCABlock: dim {dim} and the MLP's hidden width {hidden} must be multiples of 8")
        self.dim, self.num_heads, self.compute_dtype = dim, num_heads, compute_dtype
        self.norm1 = norm_layer(dim)
        self.attn = _ParamHolder()
        self.attn.temperature = nn.Parameter(torch.ones(num_heads, 1, 1))
        self.attn.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.attn.proj = nn.Linear(dim, dim)
        self.norm2 = norm_layer(dim)
        self.mlp = _ParamHolder()
        self.mlp.fc1 = nn.Linear(dim, hidden)
        self.mlp.fc2 = nn.Linear(hidden, dim)
        self.norm3 = norm_layer(dim)
        self.local_mp = _ParamHolder()
        self.local_mp.conv1 = nn.Conv2d(dim, dim, kernel_size=3, padding=1, groups=dim)
        self.local_mp.bn = nn.BatchNorm2d(dim)
        self.local_mp.conv2 = nn.Conv2d(dim, dim, kernel_size=3, padding=1, groups=dim)
        for n in (self.norm1, self.norm2, self.norm3):
            if not isinstance(n, nn.LayerNorm) or not n.elementwise_affine or tuple(n.normalized_shape) != (dim,):
                raise VitmiError("XCABlock: norm_layer must build an affine nn.LayerNorm over dim")
        self.gamma1 = nn.Parameter(eta * torch.ones(dim))
        self.gamma2 = nn.Parameter(eta * torch.ones(dim))
        self.gamma3 = nn.Parameter(eta * torch.ones(dim))
        self.pack_shadow = compute_dtype == "bf16"        # the GEMMs read the bf16 weight shadows

    def forward(self, x, H, W):
        self._refuse_cpu(x)
        if x.dim() != 3 or x.shape[-1] != self.dim:
            raise VitmiError(f"XCABlock: input must be [B, H*W, {self.dim}], got {tuple(x.shape)}")
        if H < 1 or W < 1 or x.shape[1] != H * W:
            raise VitmiError(f"XCABlock: {x.shape[1]} tokens are not an H x W = {H} x {W} grid")
        return self._run(x, H, W)

    # ---- kernels
    def _forward(self, x, Hg, Wg, save):
        B, N, D = x.shape
        H, hd, pk, M = self.num_heads, D // self.num_heads, self._pack, B * N
        a_, mlp, lp, dev, f32 = self.attn, self.mlp, self.local_mp, x.device, torch.float32
        T = torch.bfloat16 if self.compute_dtype == "bf16" else f32
        new = lambda *shape, dtype=T: torch.empty(shape, dtype=dtype, device=dev)      # noqa: E731
        pk.refresh_shadow()
        xa = x.float().contiguous().view(M, D)
        # x1 = x + gamma1 * attn(norm1(x))
        l1, mean1, rstd1 = new(M, D), new(M, dtype=f32), new(M, dtype=f32)
        ops.layernorm_fwd(xa, pk.f32(self.norm1.weight), pk.f32(self.norm1.bias), l1, mean1, rstd1, self.norm1.eps, M=M, D=D)
        qkv = new(M, 3 * D)
        ops.gemm(l1, pk.w(a_.qkv.weight), qkv, bias=pk.f32(a_.qkv.bias) if a_.qkv.bias is not None else None)
        att, stat = new(M, D), new(B, H, hd + 2, hd, dtype=f32)
        ops.xca_fwd(qkv, pk.f32(a_.temperature).view(H), att, stat, B, N, H, hd)
        x1, f1 = new(M, D, dtype=f32), new(M, D)
        ops.gemm(att, pk.w(a_.proj.weight), x1, epilogue=EPI_RESIDUAL, bias=pk.f32(a_.proj.bias), R=xa, gamma=pk.f32(self.gamma1),
                 C2=f1)
        # x2 = x1 + gamma3 * local_mp(norm3(x1)), and l2 = norm2(x2) in the same pass
        l3, mean3, rstd3 = new(M, D), new(M, dtype=f32), new(M, dtype=f32)
        ops.layernorm_fwd(x1, pk.f32(self.norm3.weight), pk.f32(self.norm3.bias), l3, mean3, rstd3, self.norm3.eps, M=M, D=D)
        u, p, lstat, bn = new(M, D), new(M, D), new(2, D, dtype=f32), lp.bn
        ops.lpi_fwd(l3, pk.f32(lp.conv1.weight), pk.f32(lp.conv1.bias), pk.f32(bn.weight), pk.f32(bn.bias),
                    pk.f32(lp.conv2.weight), pk.f32(lp.conv2.bias), bn.running_mean, bn.running_var, bn.num_batches_tracked,
                    u, lstat, p, B, Hg, Wg, D, training=self.training, momentum=bn.momentum, eps=bn.eps)
        x2, l2, mean2, rstd2 = new(M, D, dtype=f32), new(M, D), new(M, dtype=f32), new(M, dtype=f32)
        ops.ls_residual_ln_fwd(x1, p, pk.f32(self.gamma3), pk.f32(self.norm2.weight), pk.f32(self.norm2.bias), x2, l2, mean2,
                               rstd2, self.norm2.eps, M=M, D=D)
        # out = x2 + gamma2 * mlp(l2)
        Dh = mlp.fc1.out_features
        pre = new(M, Dh) if save else None
        hid = new(M, Dh)
        ops.gemm(l2, pk.w(mlp.fc1.weight), hid, epilogue=EPI_BIAS_GELU, bias=pk.f32(mlp.fc1.bias), C2=pre,
                 aux_deriv=T == torch.bfloat16)
        out, f2 = new(M, D, dtype=f32), new(M, D)
        ops.gemm(hid, pk.w(mlp.fc2.weight), out, epilogue=EPI_RESIDUAL, bias=pk.f32(mlp.fc2.bias), R=x2, gamma=pk.f32(self.gamma2),
                 C2=f2)
        if save:
            self._saved = (xa, l1, mean1, rstd1, qkv, att, stat, f1, x1, l3, mean3, rstd3, u, lstat, p, x2, l2, mean2, rstd2,
                           pre, hid, f2, self.training, (B, Hg, Wg))
        return out.view(B, N, D)

    def _backward(self, dout, need_dx):
        (xa, l1, mean1, rstd1, qkv, att, stat, f1, x1, l3, mean3, rstd3, u, lstat, p, x2, l2, mean2, rstd2, pre, hid, f2,
         training, (B, Hg, Wg)) = self._take_saved()
        M, D = xa.shape
        H, hd, pk, N = self.num_heads, D // self.num_heads, self._pack, Hg * Wg
        a_, mlp, lp, dev, f32, T = self.attn, self.mlp, self.local_mp, xa.device, torch.float32, l1.dtype
        new = lambda *shape, dtype=T: torch.empty(shape, dtype=dtype, device=dev)      # noqa: E731
        G = dout.float().contiguous().view(M, D)
        # the MLP branch: out = x2 + gamma2 * f2
        ops.colsum_mul(G, f2, pk.g(self.gamma2), M=M, N=D)
        gm = ops.scale_cast(G, new(M, D), pk.f32(self.gamma2), M=M, N=D)
        ops.colsum(gm, pk.g(mlp.fc2.bias))
        _gemm_dw(gm, hid, pk.g(mlp.fc2.weight), min_rows=256)
        dH = new(M, mlp.fc1.out_features)
        ops.gemm(gm, pk.w(mlp.fc2.weight), dH, b_kmajor=False, epilogue=EPI_DGELU, aux=pre, aux_deriv=T == torch.bfloat16)
        _gemm_dw(dH, l2, pk.g(mlp.fc1.weight), min_rows=256)
        ops.colsum(dH, pk.g(mlp.fc1.bias))
        dl2 = new(M, D)
        ops.gemm(dH, pk.w(mlp.fc1.weight), dl2, b_kmajor=False)
        # norm2: G1 = G + LN2bwd(dl2), the gradient of x2, and gp = gamma3 * G1, the gradient entering the LPI
        G1, gp = new(M, D, dtype=f32), new(M, D)
        ops.layernorm_bwd(dl2, x2, mean2, rstd2, pk.f32(self.norm2.weight), G, G1, gp, pk.g(self.norm2.weight),
                          pk.g(self.norm2.bias), gb_scale=pk.f32(self.gamma3), M=M, D=D)
        ops.colsum_mul(G1, p, pk.g(self.gamma3), M=M, N=D)
        bn, dl3 = lp.bn, new(M, D)
        ops.lpi_bwd(l3, u, gp, lstat, pk.f32(lp.conv1.weight), pk.f32(lp.conv1.bias), pk.f32(bn.weight), pk.f32(bn.bias),
                    pk.f32(lp.conv2.weight), dl3, pk.g(lp.conv1.weight), pk.g(lp.conv1.bias), pk.g(bn.weight), pk.g(bn.bias),
                    pk.g(lp.conv2.weight), pk.g(lp.conv2.bias), B, Hg, Wg, D, training=training)
        # norm3: G1 += LN3bwd(dl3), the gradient of x1, and ga = gamma1 * G1, the gradient entering proj
        ga = new(M, D)
        ops.layernorm_bwd(dl3, x1, mean3, rstd3, pk.f32(self.norm3.weight), G1, G1, ga, pk.g(self.norm3.weight),
                          pk.g(self.norm3.bias), gb_scale=pk.f32(self.gamma1), M=M, D=D)
        ops.colsum_mul(G1, f1, pk.g(self.gamma1), M=M, N=D)
        ops.colsum(ga, pk.g(a_.proj.bias))
        _gemm_dw(ga, att, pk.g(a_.proj.weight), min_rows=256)
        datt = new(M, D)
        ops.gemm(ga, pk.w(a_.proj.weight), datt, b_kmajor=False)
        dqkv = new(M, 3 * D)
        ops.xca_bwd(qkv, datt, pk.f32(a_.temperature).view(H), stat, dqkv, pk.g(a_.temperature).view(H), B, N, H, hd)
        _gemm_dw(dqkv, l1, pk.g(a_.qkv.weight), min_rows=256)
        if a_.qkv.bias is not None:
            ops.colsum(dqkv, pk.g(a_.qkv.bias))
        dl1 = new(M, D)
        ops.gemm(dqkv, pk.w(a_.qkv.weight), dl1, b_kmajor=False)
        # norm1 (its parameter gradients are needed whether or not dx is): dx = G1 + LN1bwd(dl1), in place over G1
        ops.layernorm_bwd(dl1, xa, mean1, rstd1, pk.f32(self.norm1.weight), G1, G1, None, pk.g(self.norm1.weight),
                          pk.g(self.norm1.bias), M=M, D=D)
        return G1.view(B, N, D) if need_dx else None
