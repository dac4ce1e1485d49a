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

Each module's kernel sequence is a pair of plain functions shaped like `head.head_forward` / `head_backward`:
`<name>_forward(pack, m, x, *extra, save=True) -> (out, saved)` and `<name>_backward(pack, m, saved, dout, need_dx=True) -> dx`,
`<name>` one of xca, lpi, conv_patch_embed, posfourier, class_attention_block, xcablock.  `pack` is any `ParamPack` that holds
m's parameters; `m` holds parameters, buffers and configuration (`num_heads`, `compute_dtype`, `training`, the norms' `eps`,
...) under the reference's names; `saved` is a plain tuple the caller keeps (None when not `save`).  The caller, not the
functions, refreshes the pack's bf16 shadow and rebuilds the pack: an engine once per step over one pack for all its blocks;
here each class for itself, a stand-alone module on `engine.PackedModule` as `ClassifierHead` is, with its constructor, its
input checks and `kernels = (forward, backward)`.  What several modules share (the attention branch, the LPI calls, the MLP
branch, a Linear's backward) is a private helper below.  XCA, compute_dtype "bf16": bf16 activations between the stages,
GEMMs on the pack's bf16 weight shadows; "fp32": all in fp32.  LPI: bf16 or fp32 activations, parameters and gradients in fp32.
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


F32 = torch.float32
DW_ONE, DW_ROWS = float("inf"), 256      # weight-gradient rules (`_gemm_dw`'s min_rows): one product, or two levels over token rows


def _dtype(m):
    return torch.bfloat16 if m.compute_dtype == "bf16" else F32


def _allocator(dtype, dev):
    return lambda *shape, dtype=dtype: torch.empty(shape, dtype=dtype, device=dev)


def _check_compute_dtype(cls, compute_dtype):
    if compute_dtype not in ("bf16", "fp32"):
        raise VitmiError(f"{cls}: compute_dtype must be 'bf16' or 'fp32', got {compute_dtype!r}")


def _check_layernorms(cls, dim, *norms):
    for n in norms:
        if not isinstance(n, nn.LayerNorm) or not n.elementwise_affine or tuple(n.normalized_shape) != (dim,):
            raise VitmiError(f"{cls}: norm_layer must build an affine nn.LayerNorm over dim")


def _linear_bwd(pk, lin, dy, x, dx=None, order="wbx", dw=DW_ONE, rows=slice(None), **k):
    """Backward of the rows `rows` of the Linear `lin`, in the order `order`: "w" the weight gradient dy^T x by the rule `dw`,
    "b" the bias's column sum where there is a bias, "x" the data gradient into `dx` where one is given (**k: its epilogue,
    or accumulate).  Returns dx."""
    for step in order:
        if step == "w":
            _gemm_dw(dy, x, pk.g(lin.weight)[rows], min_rows=dw)
        elif step == "b" and lin.bias is not None:
            ops.colsum(dy, pk.g(lin.bias)[rows])
        elif step == "x" and dx is not None:
            ops.gemm(dy, pk.w(lin.weight)[rows], dx, b_kmajor=False, **k)
    return dx


def _attn_fwd(pk, a, xin, new, B, N, H, **proj):
    """The attention branch on xin [B*N, D]: qkv GEMM, `ops.xca_fwd`, proj GEMM into a new fp32 tensor; `a` holds `temperature`,
    `qkv` and `proj`, **proj is proj's epilogue: nothing, or EPI_RESIDUAL with R, gamma, C2.  Returns (out, qkv, att, stat)."""
    M, D = xin.shape
    hd = D // H
    qkv = new(M, 3 * D)
    ops.gemm(xin, pk.w(a.qkv.weight), qkv, bias=pk.f32(a.qkv.bias) if a.qkv.bias is not None else None)
    att, stat = new(M, D), new(B, H, hd + 2, hd, dtype=F32)
    ops.xca_fwd(qkv, pk.f32(a.temperature).view(H), att, stat, B, N, H, hd)
    out = new(M, D, dtype=F32)
    ops.gemm(att, pk.w(a.proj.weight), out, bias=pk.f32(a.proj.bias), **proj)
    return out, qkv, att, stat


def _attn_bwd(pk, a, dy, xin, qkv, att, stat, new, B, N, H, proj_order, dw, dx_dtype):
    """Backward of `_attn_fwd` from dy, the gradient of proj's own output: proj's Linear backward in `proj_order`, `ops.xca_bwd`,
    qkv's Linear backward.  Returns the gradient of xin in `dx_dtype`, or None where that is None."""
    M, D = xin.shape
    datt = _linear_bwd(pk, a.proj, dy, att, new(M, D), proj_order, dw)
    dqkv = new(M, 3 * D)
    ops.xca_bwd(qkv, datt, pk.f32(a.temperature).view(H), stat, dqkv, pk.g(a.temperature).view(H), B, N, H, D // H)
    return _linear_bwd(pk, a.qkv, dqkv, xin, new(M, D, dtype=dx_dtype) if dx_dtype is not None else None, "wbx", dw)


def _lpi_fwd(pk, lp, xa, u, stat, out, B, H, W, training):
    """`ops.lpi_fwd` on xa [B, H*W, C] or [B*H*W, C]; `lp` holds `conv1`, `bn` and `conv2`"""
    bn = lp.bn
    ops.lpi_fwd(xa, pk.f32(lp.conv1.weight), pk.f32(lp.conv1.bias), pk.f32(bn.weight), pk.f32(bn.bias),
                pk.f32(lp.conv2.weight), pk.f32(lp.conv2.bias), bn.running_mean, bn.running_var, bn.num_batches_tracked,
                u, stat, out, B, H, W, xa.shape[-1], training=training, momentum=bn.momentum, eps=bn.eps)


def _lpi_bwd(pk, lp, xa, u, dy, stat, dx, B, H, W, training):
    bn = lp.bn
    ops.lpi_bwd(xa, u, dy, stat, pk.f32(lp.conv1.weight), pk.f32(lp.conv1.bias), pk.f32(bn.weight), pk.f32(bn.bias),
                pk.f32(lp.conv2.weight), dx, pk.g(lp.conv1.weight), pk.g(lp.conv1.bias), pk.g(bn.weight), pk.g(bn.bias),
                pk.g(lp.conv2.weight), pk.g(lp.conv2.bias), B, H, W, xa.shape[-1], training=training)
    return dx


def _mlp_fwd(pk, mlp, xin, new, save, **fc2):
    """The MLP branch on the rows xin: fc1 with bias + GELU in the epilogue (the pre-activation, its gelu' in "bf16", kept when
    `save`), then fc2: plain into the compute dtype, or with **fc2 (EPI_RESIDUAL, R, gamma, C2) into fp32.  -> (out, pre, hid)"""
    M, Dh = xin.shape[0], mlp.fc1.out_features
    pre = new(M, Dh) if save else None
    hid = new(M, Dh)
    ops.gemm(xin, pk.w(mlp.fc1.weight), hid, epilogue=EPI_BIAS_GELU, bias=pk.f32(mlp.fc1.bias), C2=pre,
             aux_deriv=hid.dtype == torch.bfloat16)
    out = new(M, mlp.fc2.out_features, dtype=F32) if fc2 else new(M, mlp.fc2.out_features)
    ops.gemm(hid, pk.w(mlp.fc2.weight), out, bias=pk.f32(mlp.fc2.bias), **fc2)
    return out, pre, hid


def _mlp_bwd(pk, mlp, gm, xin, pre, hid, new, dx, fc2_order, dw, **k):
    """Backward of `_mlp_fwd` from gm, the gradient of fc2's own output: fc2's Linear backward in `fc2_order` (its data gradient
    takes gelu' in the epilogue), then fc1's, whose data gradient goes into `dx` (**k: accumulate)."""
    dH = _linear_bwd(pk, mlp.fc2, gm, hid, new(gm.shape[0], mlp.fc1.out_features), fc2_order, dw, epilogue=EPI_DGELU, aux=pre,
                     aux_deriv=hid.dtype == torch.bfloat16)
    return _linear_bwd(pk, mlp.fc1, dH, xin, dx, "wbx", dw, **k)


def xca_forward(pack, m, x, save=True):
    B, N, C = x.shape
    dt = _dtype(m)
    xa = x.reshape(B * N, C).to(dt).contiguous()
    y, qkv, att, stat = _attn_fwd(pack, m, xa, _allocator(dt, x.device), B, N, m.num_heads)
    return y.view(B, N, C), ((xa, qkv, att, stat, (B, N)) if save else None)


def xca_backward(pack, m, saved, dout, need_dx=True):
    xa, qkv, att, stat, (B, N) = saved
    C, dt = xa.shape[1], xa.dtype
    dy = dout.reshape(B * N, C).to(dt).contiguous()
    dx = _attn_bwd(pack, m, dy, xa, qkv, att, stat, _allocator(dt, dy.device), B, N, m.num_heads, "wbx", DW_ONE,
                   F32 if need_dx else None)
    return dx.view(B, N, C) if need_dx else None


class XCA(PackedModule, nn.Module):
    kernels = (xca_forward, xca_backward)

    def __init__(self, dim, num_heads=8, qkv_bias=False, qk_scale=None, attn_drop=0., proj_drop=0., compute_dtype="bf16"):
        super().__init__()
        if attn_drop != 0. or proj_drop != 0.:
            raise VitmiError("XCA: dropout is not built (the reference's XCiT factories use attn_drop = proj_drop = 0)")
        _check_compute_dtype("XCA", compute_dtype)
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


def lpi_forward(pack, m, x, H, W, save=True):
    B, N, C = x.shape
    xa = x.to(_dtype(m)).contiguous()
    u, out, stat = torch.empty_like(xa), torch.empty_like(xa), torch.empty((2, C), dtype=F32, device=x.device)
    _lpi_fwd(pack, m, xa, u, stat, out, B, H, W, m.training)
    return out.to(x.dtype), ((xa, u, stat, m.training, (B, H, W), x.dtype) if save else None)


def lpi_backward(pack, m, saved, dout, need_dx=True):
    xa, u, stat, training, (B, H, W), xdt = saved
    dx = _lpi_bwd(pack, m, xa, u, dout.to(xa.dtype).contiguous(), stat, torch.empty_like(xa), B, H, W, training)
    return dx.to(xdt) if need_dx else None


class LPI(PackedModule, nn.Module):
    """Local patch interaction, `forward(x, H, W)` with x [B, H*W, C].  `.train()` / `.eval()` select batch or running
    statistics; in training the running buffers are updated on the device by the forward (graph-capturable).  The
    statistics are those of this process: cross-rank exchange (the reference's SyncBatchNorm under DDP) is not built.
    `conv1`, `bn`, `conv2` only hold the parameters and buffers under the reference's names; they are never called."""
    kernels = (lpi_forward, lpi_backward)

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
        _check_compute_dtype("LPI", compute_dtype)
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


ROW_CHUNK = 65535 * 64      # rows of one product: the generic GEMM kernel's grid limit (the first stage at a large batch)


def _gemm_rows(A, Bm, C, **k):
    """C = A @ op(Bm), in row chunks of A and C where there are more rows than one launch takes (rows are independent)"""
    for r in range(0, A.shape[0], ROW_CHUNK):
        ops.gemm(A[r:r + ROW_CHUNK], Bm, C[r:r + ROW_CHUNK], **k)


def _conv_stages(m):
    return [(s[0], s[1]) for s in m.proj if isinstance(s, nn.Sequential)]


def _conv_weight(pack, conv, s):
    """The k-major GEMM operand [Cout, K]: the weight's own memory, or for the first stage (K = 27) its [Cout, 32] image."""
    co, ci = conv.weight.shape[:2]
    w = pack.w(conv.weight).view(co, 9 * ci)
    if s:
        return w
    return ops.conv3s2_wcopy(w, torch.empty((co, 32), dtype=w.dtype, device=w.device), 27)


def conv_patch_embed_forward(pack, m, x, save=True):
    (B, _, h, w), dt, stages = x.shape, _dtype(m), _conv_stages(m)
    cur, saved = x, []
    for s, (conv, bn) in enumerate(stages):
        co, ci = conv.weight.shape[:2]
        ho, wo = (h + 1) // 2, (w + 1) // 2
        M = B * ho * wo
        col = torch.empty((M, 9 * ci if s else 32), dtype=dt, device=x.device)
        ops.conv3s2_im2col(cur, col, B, h, w, ci)
        y = torch.empty((M, co), dtype=dt, device=x.device)
        _gemm_rows(col, _conv_weight(pack, conv, s), y)
        del col
        stat = torch.empty((2, co), dtype=F32, device=x.device)
        out = torch.empty((B, ho * wo, co), dtype=dt, device=x.device)
        ops.bn_act_fwd(y, pack.f32(bn.weight), pack.f32(bn.bias), bn.running_mean, bn.running_var, bn.num_batches_tracked,
                       stat, out, M, co, gelu=s + 1 < len(stages), training=m.training, momentum=bn.momentum,
                       eps=bn.eps)
        saved.append((cur, y, stat, (h, w)))
        cur, h, w = out, ho, wo
    if dt != F32:
        cur = ops.cast(cur, torch.empty(cur.shape, dtype=F32, device=x.device))
    return cur, ((saved, m.training, B) if save else None)


def conv_patch_embed_backward(pack, m, saved, dout, need_dx=True):
    """the image gets no gradient: returns None"""
    saved, training, B = saved
    stages, dt = _conv_stages(m), saved[0][1].dtype
    d = dout.reshape(-1, dout.shape[-1]).to(dt).contiguous()
    for s in range(len(stages) - 1, -1, -1):
        conv, bn = stages[s]
        inp, y, stat, (h, w) = saved[s]
        co, ci = conv.weight.shape[:2]
        M = y.shape[0]
        dy = torch.empty_like(y)
        ops.bn_act_bwd(d.view(M, co), y, stat, pack.f32(bn.weight), pack.f32(bn.bias), dy, pack.g(bn.weight), pack.g(bn.bias),
                       M, co, gelu=s + 1 < len(stages), training=training)
        col = torch.empty((M, 9 * ci if s else 32), dtype=dt, device=y.device)
        ops.conv3s2_im2col(inp, col, B, h, w, ci)
        if s == 0:
            gimg = torch.empty((co, 32), dtype=F32, device=y.device)
            _gemm_dw(dy, col, gimg)
            ops.conv3s2_wcopy(gimg, pack.g(conv.weight).view(co, 27), 27)
            break
        _gemm_dw(dy, col, pack.g(conv.weight).view(co, 9 * ci))
        _gemm_rows(dy, pack.w(conv.weight).view(co, 9 * ci), col, b_kmajor=False)    # dcol, over col: it is done with
        d = torch.empty((B * h * w, ci), dtype=dt, device=y.device)
        ops.conv3s2_col2im(col, d, B, h, w, ci)
    return None


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
    kernels = (conv_patch_embed_forward, conv_patch_embed_backward)

    def __init__(self, img_size=224, patch_size=16, in_chans=3, embed_dim=768, compute_dtype="bf16"):
        super().__init__()
        img_size = tuple(img_size) if isinstance(img_size, (tuple, list)) else (img_size, img_size)
        patch = patch_size[0] if isinstance(patch_size, (tuple, list)) else patch_size
        _check_compute_dtype("ConvPatchEmbed", compute_dtype)
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

    def forward(self, x):
        self._refuse_cpu(x)
        if x.dim() != 4 or x.shape[1] != 3 or x.dtype != torch.float32:
            raise VitmiError(f"ConvPatchEmbed: input must be an fp32 image [B, 3, H, W], got {x.dtype} {tuple(x.shape)}")
        if x.requires_grad:
            raise VitmiError("ConvPatchEmbed: the gradient with respect to the image is not built (x.requires_grad)")
        B, _, H, W = x.shape
        for _ in _conv_stages(self):
            H, W = (H + 1) // 2, (W + 1) // 2
        if self.training and B * H * W < 2:
            raise VitmiError("ConvPatchEmbed: training needs at least two output positions (B*Hp*Wp): the batch variance "
                             "of the last stage is undefined")
        return self._run(x), (H, W)


def _posfourier_features(m, H, W, dev):
    """the sin / cos table [H*W, 2 hidden_dim] in the compute dtype, cached on m per (H, W, dtype, device)"""
    dt = _dtype(m)
    key = (H, W, dt, str(dev))
    f = m._tables.get(key)
    if f is None:
        f = torch.empty((H * W, 2 * m.hidden_dim), dtype=dt, device=dev)
        ops.posfourier_features(f, H, W, m.hidden_dim, m.temperature)
        m._tables[key] = f
    return f


def _posfourier_pos(pack, m, H, W, dev):
    tp = m.token_projection
    pos = torch.empty((H * W, m.dim), dtype=F32, device=dev)
    return ops.gemm(_posfourier_features(m, H, W, dev), pack.w(tp.weight).view(m.dim, 2 * m.hidden_dim), pos,
                    bias=pack.f32(tp.bias))


def posfourier_forward(pack, m, x, H, W, save=True):
    B, N, C = x.shape
    xa = x.float().contiguous()
    out = ops.add_rows_bcast(xa, _posfourier_pos(pack, m, H, W, x.device), torch.empty_like(xa), B, N, C)
    return out, ((H, W) if save else None)


def posfourier_backward(pack, m, saved, dout, need_dx=True):
    H, W = saved
    tp, C = m.token_projection, m.dim
    d = dout.float().contiguous()
    B, N = d.shape[0], H * W
    dpos = torch.empty((N, C), dtype=F32, device=d.device)
    ops.colsum(d, dpos, M=B, N=N * C)
    ops.colsum(dpos, pack.g(tp.bias), M=N, N=C)
    feat = _posfourier_features(m, H, W, d.device)
    dp = dpos if feat.dtype == F32 else ops.cast(dpos, torch.empty_like(dpos, dtype=feat.dtype))
    ops.gemm(dp, feat, pack.g(tp.weight).view(C, 2 * m.hidden_dim), a_kmajor=False, b_kmajor=False)
    return dout if need_dx else None


class PositionalEncodingFourier(PackedModule, nn.Module):
    """`forward(x, H, W)` with x [B, H*W, dim] returns `x + pos` in fp32, pos [H*W, dim] being the reference's encoding of an
    H x W grid: how `XCiT.forward_features` uses it (`x = x + pos_embeder(B, Hp, Wp).reshape(B, -1, N).permute(0, 2, 1)`).
    The reference's own `forward(B, H, W) -> [B, dim, H, W]` would materialise B identical NCHW copies of the encoding and is
    not built.  `table(H, W)` returns the fp32 encoding [H*W, dim] under no_grad.  `token_projection` only holds the
    parameters under the reference's names; it is never called.  x gets `dx = dout` (the same tensor).

    Kept for the backward: nothing but the grid; the feature table is cached per (H, W, dtype, device)."""
    kernels = (posfourier_forward, posfourier_backward)

    def __init__(self, hidden_dim=32, dim=768, temperature=10000, compute_dtype="bf16"):
        super().__init__()
        _check_compute_dtype("PositionalEncodingFourier", compute_dtype)
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

    def forward(self, x, H, W):
        self._refuse_cpu(x)
        if x.dim() != 3 or x.shape[-1] != self.dim:
            raise VitmiError(f"PositionalEncodingFourier: input must be [B, H*W, {self.dim}], got {tuple(x.shape)}")
        if H < 1 or W < 1 or x.shape[1] != H * W:
            raise VitmiError(f"PositionalEncodingFourier: {x.shape[1]} tokens are not an H x W = {H} x {W} grid")
        return self._run(x, H, W)

    def table(self, H, W):
        """the encoding [H*W, dim] in fp32 (no gradient)"""
        pack = self.pack
        pack.refresh_shadow()
        with torch.no_grad():
            return _posfourier_pos(pack, self, H, W, pack.params[0].device)


class _ParamHolder(nn.Module):
    """holds parameters, buffers and layers under the reference's names; never called"""

    def __init__(self, **members):
        super().__init__()
        for name, member in members.items():
            setattr(self, name, member)

    def forward(self, *a, **k):
        raise VitmiError("this submodule only holds parameters; call the block that owns it")


def class_attention_block_forward(pack, m, x, save=True):
    B, N1, D = x.shape
    H, hd, pk, M = m.num_heads, D // m.num_heads, pack, B * N1
    a_, T = m.attn, _dtype(m)
    new, xa = _allocator(T, x.device), x.float().contiguous()
    l, mean1, rstd1 = new(M, D), new(M, dtype=F32), new(M, dtype=F32)
    ops.layernorm_fwd(xa, pk.f32(m.norm1.weight), pk.f32(m.norm1.bias), l, mean1, rstd1, m.norm1.eps, M=M, D=D)
    Wqkv, bqkv = pk.w(a_.qkv.weight), (pk.f32(a_.qkv.bias) if a_.qkv.bias is not None else None)
    kv, q = new(M, 2 * D), new(B, D)
    ops.gemm(l, Wqkv[D:], kv, bias=bqkv[D:] if bqkv is not None else None)
    ops.gemm(l.view(B, N1 * D)[:, :D], Wqkv[:D], q, bias=bqkv[:D] if bqkv is not None else None)
    o, psave, a = new(B, D), new(B * H * N1, dtype=F32), new(B, D)
    ops.class_attn_fwd(q, kv, kv[:, D:], 2 * D, o, psave, B, H, N1, hd, m.scale)
    ops.gemm(o, pk.w(a_.proj.weight), a, bias=pk.f32(a_.proj.bias))
    x1 = ops.ca_merge_fwd(xa, a, l, pk.f32(m.gamma1), new(B, N1, D, dtype=F32), B, N1, D)
    g2, b2 = pk.f32(m.norm2.weight), pk.f32(m.norm2.bias)
    if m.tokens_norm:
        x2, mean2, rstd2 = new(B, N1, D, dtype=F32), new(M, dtype=F32), new(M, dtype=F32)
        ops.layernorm_fwd(x1, g2, b2, x2, mean2, rstd2, m.norm2.eps, M=M, D=D)
        xc, xp = x2.view(B, N1 * D)[:, :D], x2
    else:
        xc, mean2, rstd2 = new(B, D, dtype=F32), new(B, dtype=F32), new(B, dtype=F32)
        ops.layernorm_fwd(x1, g2, b2, xc, mean2, rstd2, m.norm2.eps, M=B, D=D, x_stride=N1 * D)
        xp = x1
    # the MLP's operand: the normed CLS rows, compact, in the compute dtype (kept for the fc1 weight gradient)
    xcT = xc if T == F32 and not m.tokens_norm else ops.scale_cast(xc, new(B, D), M=B, N=D,
                                                                   ldx=N1 * D if m.tokens_norm else D)
    mo, pre, hid = _mlp_fwd(pk, m.mlp, xcT, new, save)
    out = ops.ca_out_fwd(xc, xp, mo, pk.f32(m.gamma2), new(B, N1, D, dtype=F32), B, N1, D)
    return out, ((xa, l, mean1, rstd1, kv, q, o, psave, a, x1, mean2, rstd2, xcT, pre, hid, mo) if save else None)


def class_attention_block_backward(pack, m, saved, dout, need_dx=True):
    xa, l, mean1, rstd1, kv, q, o, psave, a, x1, mean2, rstd2, xcT, pre, hid, mo = saved
    B, N1, D = xa.shape
    H, hd, pk, M = m.num_heads, D // m.num_heads, pack, B * N1
    a_, new = m.attn, _allocator(l.dtype, xa.device)
    G = dout.float().contiguous()
    # the last line and the MLP on B rows
    dx2, gm = new(B, N1, D, dtype=F32), new(B, D)
    ops.ca_out_bwd(G, pk.f32(m.gamma2), dx2, gm, B, N1, D)
    ops.colsum_mul(G.view(B, N1 * D)[:, :D], mo, pk.g(m.gamma2), M=B, N=D, ldx=N1 * D, ldy=D)      # the CLS rows, strided
    dx2c = dx2.view(B, N1 * D)[:, :D]
    _mlp_bwd(pk, m.mlp, gm, xcT, pre, hid, new, dx2c, "xwb", DW_ONE, accumulate=True)      # dx2_c = G_c + the MLP's gradient
    # norm2
    g2w, gg2, gb2 = pk.f32(m.norm2.weight), pk.g(m.norm2.weight), pk.g(m.norm2.bias)
    if m.tokens_norm:
        dx1 = new(B, N1, D, dtype=F32)
        ops.layernorm_bwd(dx2, x1, mean2, rstd2, g2w, None, dx1, None, gg2, gb2, M=M, D=D)
    else:
        dyc = ops.scale_cast(dx2c, new(B, D, dtype=F32), M=B, N=D, ldx=N1 * D)
        ops.layernorm_bwd(dyc, x1, mean2, rstd2, g2w, None, dx2, None, gg2, gb2, M=B, D=D, x_stride=N1 * D,
                          g_stride=N1 * D)                                        # over the CLS rows of dx2; dx1_p = dx2_p
        dx1 = dx2
    # the first residual's branch
    da, dl = new(B, D), new(B, N1, D, dtype=F32)
    ops.ca_merge_bwd(dx1, l, a, pk.f32(m.gamma1), da, dl, pk.g(m.gamma1), B, N1, D)
    do = _linear_bwd(pk, a_.proj, da, o, new(B, D))
    dq, dkv = new(B, D), new(M, 2 * D)
    ops.class_attn_bwd(q, kv, kv[:, D:], 2 * D, do, psave, dq, dkv, dkv[:, D:], 2 * D, B, H, N1, hd, m.scale)
    # qkv: its k / v rows over all B*N1 token rows, its q rows over the B CLS rows; the data gradients add into dl
    dlm = dl.view(M, D)
    lc, dlc = l.view(B, N1 * D)[:, :D], dl.view(B, N1 * D)[:, :D]
    halves = ((dkv, l, dlm, DW_ROWS, slice(D, None)), (dq, lc, dlc, DW_ONE, slice(D)))
    for step in "wbx":
        for dy, xin, dx, dw, rows in halves:
            _linear_bwd(pk, a_.qkv, dy, xin, dx, step, dw, rows, accumulate=True)
    # norm1 (its parameter gradients are needed whether or not dx is): dx = dx1 + LN1bwd(dl), in place over dx1
    ops.layernorm_bwd(dlm, xa, mean1, rstd1, pk.f32(m.norm1.weight), dx1, dx1, None, pk.g(m.norm1.weight),
                      pk.g(m.norm1.bias), M=M, D=D)
    return dx1 if need_dx else None


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
    kernels = (class_attention_block_forward, class_attention_block_backward)

    def __init__(self, dim, num_heads, mlp_ratio=4., qkv_bias=False, qk_scale=None, drop=0., attn_drop=0., drop_path=0.,
                 act_layer=nn.GELU, norm_layer=nn.LayerNorm, eta=None, tokens_norm=False, compute_dtype="bf16"):
        super().__init__()
        _check_compute_dtype("ClassAttentionBlock", compute_dtype)
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
        self.attn = _ParamHolder(qkv=nn.Linear(dim, dim * 3, bias=qkv_bias), proj=nn.Linear(dim, dim))
        self.norm2 = norm_layer(dim)
        self.mlp = _ParamHolder(fc1=nn.Linear(dim, int(dim * mlp_ratio)), fc2=nn.Linear(int(dim * mlp_ratio), dim))
        _check_layernorms("ClassAttentionBlock", dim, self.norm1, self.norm2)
        if int(dim * mlp_ratio) < 8 or int(dim * mlp_ratio) % 8:
            raise VitmiError(f"ClassAttentionBlock: the MLP's hidden width {int(dim * mlp_ratio)} must be a multiple of 8")
        self.gamma1, self.gamma2 = (nn.Parameter(eta * torch.ones(dim)) for _ in range(2))
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


def xcablock_forward(pack, m, x, Hg, Wg, save=True):
    B, N, D = x.shape
    pk, M, new = pack, B * N, _allocator(_dtype(m), x.device)
    xa = x.float().contiguous().view(M, D)
    # x1 = x + gamma1 * attn(norm1(x))
    l1, mean1, rstd1 = new(M, D), new(M, dtype=F32), new(M, dtype=F32)
    ops.layernorm_fwd(xa, pk.f32(m.norm1.weight), pk.f32(m.norm1.bias), l1, mean1, rstd1, m.norm1.eps, M=M, D=D)
    f1 = new(M, D)
    x1, qkv, att, stat = _attn_fwd(pk, m.attn, l1, new, B, N, m.num_heads, epilogue=EPI_RESIDUAL, R=xa, gamma=pk.f32(m.gamma1),
                                   C2=f1)
    # x2 = x1 + gamma3 * local_mp(norm3(x1)), and l2 = norm2(x2) in the same pass
    l3, mean3, rstd3 = new(M, D), new(M, dtype=F32), new(M, dtype=F32)
    ops.layernorm_fwd(x1, pk.f32(m.norm3.weight), pk.f32(m.norm3.bias), l3, mean3, rstd3, m.norm3.eps, M=M, D=D)
    u, p, lstat = new(M, D), new(M, D), new(2, D, dtype=F32)
    _lpi_fwd(pk, m.local_mp, l3, u, lstat, p, B, Hg, Wg, m.training)
    x2, l2, mean2, rstd2 = new(M, D, dtype=F32), new(M, D), new(M, dtype=F32), new(M, dtype=F32)
    ops.ls_residual_ln_fwd(x1, p, pk.f32(m.gamma3), pk.f32(m.norm2.weight), pk.f32(m.norm2.bias), x2, l2, mean2, rstd2,
                           m.norm2.eps, M=M, D=D)
    # out = x2 + gamma2 * mlp(l2)
    f2 = new(M, D)
    out, pre, hid = _mlp_fwd(pk, m.mlp, l2, new, save, epilogue=EPI_RESIDUAL, R=x2, gamma=pk.f32(m.gamma2), C2=f2)
    return out.view(B, N, D), ((xa, l1, mean1, rstd1, qkv, att, stat, f1, x1, l3, mean3, rstd3, u, lstat, p, x2, l2, mean2, rstd2,
                                pre, hid, f2, m.training, (B, Hg, Wg)) if save else None)


def xcablock_backward(pack, m, saved, dout, need_dx=True):
    (xa, l1, mean1, rstd1, qkv, att, stat, f1, x1, l3, mean3, rstd3, u, lstat, p, x2, l2, mean2, rstd2, pre, hid, f2,
     training, (B, Hg, Wg)) = saved
    M, D = xa.shape
    pk, N, new = pack, Hg * Wg, _allocator(l1.dtype, xa.device)
    G = dout.float().contiguous().view(M, D)
    # the MLP branch: out = x2 + gamma2 * f2
    ops.colsum_mul(G, f2, pk.g(m.gamma2), M=M, N=D)
    gm = ops.scale_cast(G, new(M, D), pk.f32(m.gamma2), M=M, N=D)
    dl2 = _mlp_bwd(pk, m.mlp, gm, l2, pre, hid, new, new(M, D), "bwx", DW_ROWS)
    # norm2: G1 = G + LN2bwd(dl2), the gradient of x2, and gp = gamma3 * G1, the gradient entering the LPI
    G1, gp = new(M, D, dtype=F32), new(M, D)
    ops.layernorm_bwd(dl2, x2, mean2, rstd2, pk.f32(m.norm2.weight), G, G1, gp, pk.g(m.norm2.weight),
                      pk.g(m.norm2.bias), gb_scale=pk.f32(m.gamma3), M=M, D=D)
    ops.colsum_mul(G1, p, pk.g(m.gamma3), M=M, N=D)
    dl3 = _lpi_bwd(pk, m.local_mp, l3, u, gp, lstat, new(M, D), B, Hg, Wg, training)
    # norm3: G1 += LN3bwd(dl3), the gradient of x1, and ga = gamma1 * G1, the gradient entering proj
    ga = new(M, D)
    ops.layernorm_bwd(dl3, x1, mean3, rstd3, pk.f32(m.norm3.weight), G1, G1, ga, pk.g(m.norm3.weight),
                      pk.g(m.norm3.bias), gb_scale=pk.f32(m.gamma1), M=M, D=D)
    ops.colsum_mul(G1, f1, pk.g(m.gamma1), M=M, N=D)
    dl1 = _attn_bwd(pk, m.attn, ga, l1, qkv, att, stat, new, B, N, m.num_heads, "bwx", DW_ROWS, l1.dtype)
    # norm1 (its parameter gradients are needed whether or not dx is): dx = G1 + LN1bwd(dl1), in place over G1
    ops.layernorm_bwd(dl1, xa, mean1, rstd1, pk.f32(m.norm1.weight), G1, G1, None, pk.g(m.norm1.weight),
                      pk.g(m.norm1.bias), M=M, D=D)
    return G1.view(B, N, D) if need_dx else None


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
    kernels = (xcablock_forward, xcablock_backward)

    def __init__(self, dim, num_heads, mlp_ratio=4., qkv_bias=False, qk_scale=None, drop=0., attn_drop=0., drop_path=0.,
                 act_layer=nn.GELU, norm_layer=nn.LayerNorm, num_tokens=196, eta=None, compute_dtype="bf16"):
        super().__init__()
        _check_compute_dtype("XCABlock", compute_dtype)
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
        self.attn = _ParamHolder(temperature=nn.Parameter(torch.ones(num_heads, 1, 1)),
                                 qkv=nn.Linear(dim, dim * 3, bias=qkv_bias), proj=nn.Linear(dim, dim))
        self.norm2 = norm_layer(dim)
        self.mlp = _ParamHolder(fc1=nn.Linear(dim, hidden), fc2=nn.Linear(hidden, dim))
        self.norm3 = norm_layer(dim)
        self.local_mp = _ParamHolder(conv1=nn.Conv2d(dim, dim, kernel_size=3, padding=1, groups=dim), bn=nn.BatchNorm2d(dim),
                                     conv2=nn.Conv2d(dim, dim, kernel_size=3, padding=1, groups=dim))
        _check_layernorms("XCABlock", dim, self.norm1, self.norm2, self.norm3)
        self.gamma1, self.gamma2, self.gamma3 = (nn.Parameter(eta * torch.ones(dim)) for _ in range(3))
        self.pack_shadow = compute_dtype == "bf16"        # the GEMMs read the bf16 weight shadows

    def forward(self, x, H, W):
        self._refuse_cpu(x)
        if x.dim() != 3 or x.shape[-1] != self.dim:
            raise VitmiError(f"XCABlock: input must be [B, H*W, {self.dim}], got {tuple(x.shape)}")
        if H < 1 or W < 1 or x.shape[1] != H * W:
            raise VitmiError(f"XCABlock: {x.shape[1]} tokens are not an H x W = {H} x {W} grid")
        return self._run(x, H, W)
