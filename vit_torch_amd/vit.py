"""DINO-style VisionTransformer whose forward/backward run on libvitmi HIP kernels.

Drop-in for the module the reference obtains from
`torch.hub.load('facebookresearch/dino:main', arch)`
(/root/reference/models/vision_all.py:156): same constructor arguments,
attribute surface (`.patch_embed.proj` Conv2d, `.norm`, `.head`, `.blocks[i]`),
parameter names/shapes (state-dict compatible) and call contract
`model(x[B,C,H,W] fp32) -> [B, K or D] fp32` (utils_network.py:418).

The nn.Linear / nn.LayerNorm / nn.Conv2d sub-modules are parameter holders
only; `forward` hands the whole network to `VitEngine`, which sequences the
hand-written kernels (GEMM+epilogues, LayerNorm, fused attention, ...) through
the C ABI and implements the backward pass explicitly (the reference relies on
autograd, utils_network.py:441).  There is no PyTorch fallback.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from . import ops
from ._lib import EPI_BIAS_GELU, EPI_DGELU, EPI_PATCH_POS, EPI_RESIDUAL, VitmiError
from .engine import Engine, EngineModel, engine_wgrad_pair, mlp_backward, mlp_forward, reducer_flags
from .head import head_backward, head_forward
from .posembed import tables_for
from .data import PatchRows

# compute_dtype: "bf16" (bf16 operands, fp32 accumulate: the benchmarked mode), "fp32" (fp32 MFMA / VALU: the exact parity
# mode) or "bf16x3" (round 5: fp32 activations and weights, every GEMM as three bf16 products of hi / lo operand halves on
# the tile kernel — ops.gemm_split3, csrc/split3.hip: fp32-grade products at a third of the bf16 rate instead of 1/80)
_DT = {"bf16": torch.bfloat16, "fp32": torch.float32, "bf16x3": torch.float32, torch.bfloat16: torch.bfloat16,
       torch.float32: torch.float32}


# ----------------------------------------------------------------- modules --
class Mlp(nn.Module):
    def __init__(self, in_features, hidden_features):
        super().__init__()
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.act = nn.GELU()
        self.fc2 = nn.Linear(hidden_features, in_features)


class Attention(nn.Module):
    def __init__(self, dim, num_heads, qkv_bias):
        super().__init__()
        self.num_heads = num_heads
        self.scale = (dim // num_heads) ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)


class Block(nn.Module):
    def __init__(self, dim, num_heads, mlp_ratio, qkv_bias, eps):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=eps)
        self.attn = Attention(dim, num_heads, qkv_bias)
        self.norm2 = nn.LayerNorm(dim, eps=eps)
        self.mlp = Mlp(dim, int(dim * mlp_ratio))


class PatchEmbed(nn.Module):
    def __init__(self, img_size, patch_size, in_chans, embed_dim):
        super().__init__()
        self.img_size = img_size
        self.patch_size = patch_size
        self.num_patches = (img_size // patch_size) ** 2
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=patch_size, stride=patch_size)


def _trunc_normal_(t, std=0.02):
    return nn.init.trunc_normal_(t, std=std)


class VisionTransformer(EngineModel, nn.Module):
    """`apply_head=False` reproduces upstream DINO, whose forward returns
    norm(x)[:, 0] and never calls `.head` ([recall]); the factory
    passes `apply_head=True` when it installs a classifier."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, num_classes=0, embed_dim=768,
                 depth=12, num_heads=12, mlp_ratio=4.0, qkv_bias=True, eps=1e-6, apply_head=False,
                 compute_dtype="bf16", residual_dtype="fp32", cls_only_last_block=False, **_ignored):
        super().__init__()
        self.num_features = self.embed_dim = embed_dim
        self.apply_head = apply_head
        # Opt-in (default off; bench.py reports it as a separate extra, never as `value`): the model's output is
        # norm(x)[:, 0], so in the LAST block only the CLS row of the attention output, of proj and of the MLP reaches it —
        # and only the CLS row carries a gradient back.  With the flag the last block computes exactly that row (k, v
        # still come from all tokens): the same logits, loss and gradients as the full computation (the reference
        # computes the other 196 rows and discards them), ~6 % fewer FLOPs per step.  tests/test_vit_gpu.py compares.
        self.cls_only_last_block = bool(cls_only_last_block)
        self.compute_dtype = _DT[compute_dtype]
        self.split3 = compute_dtype == "bf16x3"
        # the residual stream between the blocks: "fp32" (default: the reference trains in fp32, and the fp32 stream ends a
        # 50-step run within 0.06-0.08 % of the oracle loss, tests/test_training_curve_gpu.py), "bf16" (what bench.py times:
        # 1.1-2.2 % on the same test), or "auto" = follow the compute dtype
        self.residual_dtype = self.compute_dtype if residual_dtype == "auto" else _DT[residual_dtype]
        self.patch_embed = PatchEmbed(img_size, patch_size, in_chans, embed_dim)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, self.patch_embed.num_patches + 1, embed_dim))
        self.blocks = nn.ModuleList([Block(embed_dim, num_heads, mlp_ratio, qkv_bias, eps)
                                     for _ in range(depth)])
        self.norm = nn.LayerNorm(embed_dim, eps=eps)
        self.head = nn.Linear(embed_dim, num_classes) if num_classes > 0 else nn.Identity()
        _trunc_normal_(self.pos_embed)
        _trunc_normal_(self.cls_token)
        for m in self.modules():
            if isinstance(m, nn.Linear):
                _trunc_normal_(m.weight)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)
            elif isinstance(m, nn.LayerNorm):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)
        self._engine: Optional[VitEngine] = None

    def _new_engine(self) -> "VitEngine":
        return VitEngine(self)

    # upstream DINO's two other public methods (facebookresearch/dino vision_transformer.py).  Forward only: they refuse
    # to run where autograd would want a graph (call them under torch.no_grad() or with the backbone frozen); there is no
    # backward through their outputs.  Both run every block in full, also with cls_only_last_block (and so also at
    # N > 256 tokens, which that option's forward refuses).
    def _introspection_engine(self, x, what):
        if not x.is_cuda:
            raise VitmiError("vit_torch_amd models run on an MI355X (HIP) device; got a CPU tensor "
                             "and there is no CPU fallback")
        eng = self.engine()
        if torch.is_grad_enabled() and any(p.requires_grad for p in eng.pack.params):
            raise VitmiError(f"{what} is forward-only (no backward through it): call it under torch.no_grad() or "
                             "freeze the backbone (requires_grad_(False))")
        return eng

    def get_last_selfattention(self, x):
        """The last block's attention probabilities softmax((q k^T) * scale), fp32 [B, num_heads, N, N], N = 1 + patches
        (upstream: DINO's attention-map visualisation).  Accepts what forward accepts.  Forward only."""
        return self._introspection_engine(x, "get_last_selfattention").last_selfattention(x)

    def get_intermediate_layers(self, x, n=1):
        """[self.norm(x) after each of the last n blocks], oldest first, each a fresh fp32 [B, N, embed_dim] over all
        tokens (upstream: DINO's linear evaluation and dense features).  n = 0 gives [], n >= depth every block.
        Accepts what forward accepts.  Forward only."""
        return self._introspection_engine(x, "get_intermediate_layers").intermediate_layers(x, n)


# ------------------------------------------------------------------ engine --
class VitEngine(Engine):
    """Executes VisionTransformer forward / backward as a fixed kernel sequence.

    Activations of type T (compute dtype: bf16, or fp32 in parity mode), residual
    stream of type R; every residual update writes a NEW buffer, so the inputs of
    every LayerNorm are kept for backward without an extra copy.
    """

    def __init__(self, model: VisionTransformer):
        super().__init__(model)
        # Row padding (round 4): M = B * N is a multiple of the 256-row GEMM tile only for special batch sizes (197 B: B % 256
        # == 0).  Every [M, .] activation is allocated to the next multiple of 256 rows and used through its [:M] view; the
        # GEMM calls carry VITMI_LAUNCH_ROWS_PADDED, so a ragged M runs on the 256x256 tile kernel (last row tile: A's last row
        # repeated, surplus output rows into the padding) instead of the slower 256x128 ragged form.
        self.pad_rows = self.T == torch.bfloat16
        self.cls_last = bool(model.cls_only_last_block)
        if self.cls_last and model.embed_dim // model.blocks[0].attn.num_heads > 64:
            # the one-query form runs on the class-attention kernels (cait_ops.hip): hd <= 64 (and N <= 256, checked per input)
            raise VitmiError("cls_only_last_block needs head_dim <= 64 (the class-attention kernels' limit); got "
                             f"{model.embed_dim // model.blocks[0].attn.num_heads}: build the model without the option")

    def is_current(self) -> bool:
        return super().is_current() and bool(self.model.cls_only_last_block) == self.cls_last

    def _pos_for(self, gh, gw):
        """pos_embed at the input's patch grid: as stored, or the bicubic resize upstream DINO
        applies ([recall]; oracle/vit_ref.py:110-127) through the tap-table kernel
        (posembed.py, vitmi_pos_resample); returns (pos [N,D] fp32, tables or None)."""
        m = self.model
        pos = self.pack.f32(m.pos_embed)
        n_stored = pos.shape[1] - 1
        if gh * gw == n_stored and gh == gw:
            return pos.reshape(-1, pos.shape[-1]), None
        tabs = tables_for(n_stored, gh, gw, pos.device)
        return ops.pos_resample(pos.reshape(-1, pos.shape[-1]), tabs.fwd), tabs

    # -- forward -------------------------------------------------------------
    def _shape(self, x):
        """Host-only: (B, N, M, D, H, hd, Kp, gh, gw) of an NCHW image tensor or PatchRows input."""
        m = self.model
        if isinstance(x, PatchRows):
            B, Cin, Himg, Wimg = x.B, x.C, x.H, x.W
        else:
            B, Cin, Himg, Wimg = x.shape
        p = m.patch_embed.patch_size
        conv = m.patch_embed.proj
        if Cin != conv.in_channels:
            raise VitmiError(f"input has {Cin} channels, patch_embed.proj expects {conv.in_channels}")
        gh, gw = Himg // p, Wimg // p
        N = 1 + gh * gw
        D = m.embed_dim
        H = m.blocks[0].attn.num_heads
        return B, N, B * N, D, H, D // H, Cin * p * p, gh, gw

    def _embed(self, x, shape, new):
        """Patch rows, then X = patch_embed(x) + pos_embed with the CLS row in front: the residual stream [M, D] (dtype R)
        that enters block 0.  Returns (X, patches, pos_tabs)."""
        m, T = self.model, self.T
        B, N, M, D, H, hd, Kp, gh, gw = shape
        p = m.patch_embed.patch_size
        conv = m.patch_embed.proj
        pre = x if isinstance(x, PatchRows) else None          # device input pipeline: rows already gathered
        if pre is None:
            x = x.float() if x.dtype != torch.float32 else x
        self.pack.refresh_shadow()
        if pre is None:
            patches = new(M, Kp, T)
            ops.patchify(x, patches, p, cls_rows=1)
        else:
            if pre.p != p or pre.cls_rows != 1 or pre.rows.dtype != T or tuple(pre.rows.shape) != (M, Kp):
                raise VitmiError(f"PatchRows (p={pre.p}, cls_rows={pre.cls_rows}, {pre.rows.dtype}, {tuple(pre.rows.shape)}) "
                                 f"does not fit this model (p={p}, cls_rows=1, {T}, {(M, Kp)})")
            patches = pre.rows
        pos, pos_tabs = self._pos_for(gh, gw)
        X = new(M, D, self.R)
        self._gemm(patches, self._w(conv.weight).view(D, Kp), X, epilogue=EPI_PATCH_POS,
                   bias=self.pack.f32(conv.bias) if conv.bias is not None else None,
                   pos=pos, n_tok=N, cls=self.pack.f32(m.cls_token).view(-1))
        return X, patches, pos_tabs

    def _ln1_qkv(self, blk, X, M, D, new, dev):
        """norm1 and the qkv Linear of a block: (ln1, mean1, rstd1, qkv [M, 3D] dtype T)."""
        a = blk.attn
        ln1 = new(M, D, self.T)
        mean1 = torch.empty(M, dtype=torch.float32, device=dev)
        rstd1 = torch.empty(M, dtype=torch.float32, device=dev)
        ops.layernorm_fwd(X, self.pack.f32(blk.norm1.weight), self.pack.f32(blk.norm1.bias), ln1,
                          mean1, rstd1, blk.norm1.eps, M=M, D=D)
        qkv = new(M, 3 * D, self.T)
        self._gemm(ln1, self._w(a.qkv.weight), qkv,
                   bias=self.pack.f32(a.qkv.bias) if a.qkv.bias is not None else None)
        return ln1, mean1, rstd1, qkv

    def _block_fwd(self, blk, X, B, N, M, D, H, hd, save, new, dev):
        """One full block: X2 = X + attn(norm1(X)), then + mlp(norm2(.)), into new buffers.  Returns (X2, what the
        backward needs or None)."""
        T, R = self.T, self.R
        a, mlp = blk.attn, blk.mlp
        ln1, mean1, rstd1, qkv = self._ln1_qkv(blk, X, M, D, new, dev)
        O = new(M, D, T)
        lse = torch.empty(B * H * N, dtype=torch.float32, device=dev)
        ops.attn_fwd(qkv, O, lse, B, N, H, hd, a.scale)
        X1 = new(M, D, R)
        self._gemm(O, self._w(a.proj.weight), X1, epilogue=EPI_RESIDUAL,
                   bias=self.pack.f32(a.proj.bias), R=X)
        ln2 = new(M, D, T)
        mean2 = torch.empty(M, dtype=torch.float32, device=dev)
        rstd2 = torch.empty(M, dtype=torch.float32, device=dev)
        ops.layernorm_fwd(X1, self.pack.f32(blk.norm2.weight), self.pack.f32(blk.norm2.bias), ln2,
                          mean2, rstd2, blk.norm2.eps, M=M, D=D)
        X2, pre, hid = mlp_forward(self, mlp, ln2, X1, save)
        saved = (X, ln1, mean1, rstd1, qkv, O, lse, X1, ln2, mean2, rstd2, pre, hid) if save else None
        return X2, saved

    def forward(self, x, save: bool):
        m = self.model
        dev = x.device
        shape = self._shape(x)
        B, N, M, D, H, hd, Kp, gh, gw = shape
        if self.cls_last and N > 256:
            raise VitmiError(f"cls_only_last_block needs at most 256 tokens per image (the class-attention kernels' limit); this "
                             f"input has {N}: build the model without the option")

        def new(rows, cols, dt):
            return self._alloc(rows, cols, dt, dev)

        X, patches, pos_tabs = self._embed(x, shape, new)
        blocks = []
        last_cls = None
        for bi_, blk in enumerate(m.blocks):
            if self.cls_last and bi_ == len(m.blocks) - 1:
                X, last_cls = self._last_block_cls_fwd(blk, X, B, N, M, D, H, hd, save, new, dev)
                break
            X, sv = self._block_fwd(blk, X, B, N, M, D, H, hd, save, new, dev)
            if save:
                blocks.append(sv)
        feat = torch.empty((B, D), dtype=torch.float32, device=dev)
        meanf = torch.empty(B, dtype=torch.float32, device=dev)
        rstdf = torch.empty(B, dtype=torch.float32, device=dev)
        xf_stride = D if last_cls is not None else N * D       # the CLS-only last block leaves a [B, D] stream
        ops.layernorm_fwd(X, self.pack.f32(m.norm.weight), self.pack.f32(m.norm.bias), feat, meanf,
                          rstdf, m.norm.eps, M=B, D=D, x_stride=xf_stride, y_stride=D)
        out, head_saved = head_forward(self.pack, self.head, feat)
        if save:
            self.saved = dict(B=B, N=N, M=M, D=D, H=H, hd=hd, Kp=Kp, patches=patches, blocks=blocks,
                              Xf=X, meanf=meanf, rstdf=rstdf, head=head_saved,
                              pos_tabs=pos_tabs, last_cls=last_cls)
        return out

    # -- upstream DINO's introspection methods (forward only, every block computed in full) -----------------------
    def intermediate_layers(self, x, n: int):
        """[norm(x) after block i for the last n blocks], oldest first, each a fresh fp32 [B, N, D] tensor."""
        m = self.model
        L = len(m.blocks)
        n = max(0, min(int(n), L))
        if n == 0:
            return []
        dev = x.device
        shape = self._shape(x)
        B, N, M, D, H, hd = shape[:6]

        def new(rows, cols, dt):
            return self._alloc(rows, cols, dt, dev)

        X, _, _ = self._embed(x, shape, new)
        outs = []
        for bi_, blk in enumerate(m.blocks):
            X, _ = self._block_fwd(blk, X, B, N, M, D, H, hd, False, new, dev)
            if L - bi_ <= n:
                y = torch.empty((M, D), dtype=torch.float32, device=dev)
                ops.layernorm_fwd(X, self.pack.f32(m.norm.weight), self.pack.f32(m.norm.bias), y,
                                  torch.empty(M, dtype=torch.float32, device=dev),
                                  torch.empty(M, dtype=torch.float32, device=dev), m.norm.eps, M=M, D=D)
                outs.append(y.view(B, N, D))
        return outs

    def last_selfattention(self, x):
        """softmax((q k^T) * scale) of the last block, fp32 [B, H, N, N]: blocks 0 .. L-2 in full, then only the last
        block's norm1, qkv Linear and the probabilities (vitmi_attn_probs)."""
        m = self.model
        dev = x.device
        shape = self._shape(x)
        B, N, M, D, H, hd = shape[:6]

        def new(rows, cols, dt):
            return self._alloc(rows, cols, dt, dev)

        X, _, _ = self._embed(x, shape, new)
        for blk in list(m.blocks)[:-1]:
            X, _ = self._block_fwd(blk, X, B, N, M, D, H, hd, False, new, dev)
        last = m.blocks[-1]
        qkv = self._ln1_qkv(last, X, M, D, new, dev)[3]
        P = torch.empty((B, H, N, N), dtype=torch.float32, device=dev)
        return ops.attn_probs(qkv, P, B, N, H, hd, last.attn.scale)

    # -- the last block on the CLS row only (cls_only_last_block) ------------------
    def _last_block_cls_fwd(self, blk, X, B, N, M, D, H, hd, save, new, dev):
        """x_cls' = block(x)[:, 0]: LayerNorm and the k / v projections over all tokens, one query per image (the
        class-attention kernels of cait_ops.hip: softmax((q k^T) scale) v with q from token 0), proj / residual / MLP on B rows.
        Returns the new CLS stream [B, D] (dtype R) and what the backward needs."""
        T, R, pk = self.T, self.R, self.pack
        a, mlp = blk.attn, blk.mlp
        f32 = torch.float32
        ln1 = new(M, D, T)
        mean1, rstd1 = torch.empty(M, dtype=f32, device=dev), torch.empty(M, dtype=f32, device=dev)
        ops.layernorm_fwd(X, pk.f32(blk.norm1.weight), pk.f32(blk.norm1.bias), ln1, mean1, rstd1, blk.norm1.eps, M=M, D=D)
        Wqkv, bqkv = self._w(a.qkv.weight), (pk.f32(a.qkv.bias) if a.qkv.bias is not None else None)
        kv = new(M, 2 * D, T)
        self._gemm(ln1, Wqkv[D:], kv, bias=bqkv[D:] if bqkv is not None else None)
        ln1_cls = ln1.view(B, N * D)[:, :D]                     # strided CLS rows
        q = torch.empty((B, D), dtype=T, device=dev)
        ops.gemm(ln1_cls, Wqkv[:D], q, bias=bqkv[:D] if bqkv is not None else None)
        oc = torch.empty((B, D), dtype=T, device=dev)
        psave = torch.empty(B * H * N, dtype=f32, device=dev)
        ops.class_attn_fwd(q, kv, kv[:, D:], 2 * D, oc, psave, B, H, N, hd, a.scale)
        Xc = X.view(B, N * D)[:, :D]                            # the residual stream's CLS rows (strided)
        X1 = torch.empty((B, D), dtype=R, device=dev)
        ops.gemm(oc, self._w(a.proj.weight), X1, epilogue=EPI_RESIDUAL, bias=pk.f32(a.proj.bias), R=Xc)
        ln2 = torch.empty((B, D), dtype=T, device=dev)
        mean2, rstd2 = torch.empty(B, dtype=f32, device=dev), torch.empty(B, dtype=f32, device=dev)
        ops.layernorm_fwd(X1, pk.f32(blk.norm2.weight), pk.f32(blk.norm2.bias), ln2, mean2, rstd2, blk.norm2.eps, M=B, D=D)
        Dh = mlp.fc1.out_features
        pre = torch.empty((B, Dh), dtype=T, device=dev) if save else None
        hid = torch.empty((B, Dh), dtype=T, device=dev)
        ops.gemm(ln2, self._w(mlp.fc1.weight), hid, epilogue=EPI_BIAS_GELU, bias=pk.f32(mlp.fc1.bias), C2=pre,
                 aux_deriv=T == torch.bfloat16)
        X2 = torch.empty((B, D), dtype=R, device=dev)
        ops.gemm(hid, self._w(mlp.fc2.weight), X2, epilogue=EPI_RESIDUAL, bias=pk.f32(mlp.fc2.bias), R=X1)
        saved = (X, ln1, mean1, rstd1, kv, q, oc, psave, X1, ln2, mean2, rstd2, pre, hid) if save else None
        return X2, saved

    def _last_block_cls_bwd(self, blk, sv, Gc, B, N, M, D, H, hd, dev, prev_fc2_bias):
        """Backward of _last_block_cls_fwd.  Gc [B, D] (dtype R): gradient of the block's CLS output.  Returns G [M, D]
        (dtype R, padded rows): the gradient of the residual stream entering the block, and its operand copy Gb."""
        T, R, pk = self.T, self.R, self.pack
        a, mlp = blk.attn, blk.mlp
        f32 = torch.float32
        X, ln1, mean1, rstd1, kv, q, oc, psave, X1, ln2, mean2, rstd2, pre, hid = sv
        Dh = mlp.fc1.out_features

        def cast(t):
            if t.dtype == T:
                return t
            o = torch.empty(t.shape, dtype=T, device=dev)
            ops.cast(t.contiguous(), o)
            return o

        Gcb = cast(Gc)
        # MLP branch on B rows
        dH = torch.empty((B, Dh), dtype=T, device=dev)
        ops.gemm(Gcb, self._w(mlp.fc2.weight), dH, b_kmajor=False, epilogue=EPI_DGELU, aux=pre, aux_deriv=T == torch.bfloat16)
        ops.gemm(Gcb, hid, pk.g(mlp.fc2.weight), a_kmajor=False, b_kmajor=False)
        ops.colsum(Gcb, pk.g(mlp.fc2.bias))
        ops.gemm(dH, ln2, pk.g(mlp.fc1.weight), a_kmajor=False, b_kmajor=False)
        ops.colsum(dH, pk.g(mlp.fc1.bias))
        dln2 = torch.empty((B, D), dtype=T, device=dev)
        ops.gemm(dH, self._w(mlp.fc1.weight), dln2, b_kmajor=False)
        G1 = torch.empty((B, D), dtype=R, device=dev)            # gradient of X1 = Gc + LN2 backward
        G1b = torch.empty((B, D), dtype=T, device=dev) if T != R else None
        ops.layernorm_bwd(dln2, X1, mean2, rstd2, pk.f32(blk.norm2.weight), Gc.contiguous(), G1, G1b,
                          pk.g(blk.norm2.weight), pk.g(blk.norm2.bias), gsum=pk.g(a.proj.bias), M=B, D=D)
        G1o = G1 if G1b is None else G1b
        # attention branch: one query per image
        doc = torch.empty((B, D), dtype=T, device=dev)
        ops.gemm(G1o, self._w(a.proj.weight), doc, b_kmajor=False)
        ops.gemm(G1o, oc, pk.g(a.proj.weight), a_kmajor=False, b_kmajor=False)
        dq = torch.empty((B, D), dtype=T, device=dev)
        dkv = self._alloc(M, 2 * D, T, dev)
        ops.class_attn_bwd(q, kv, kv[:, D:], 2 * D, doc, psave, dq, dkv, dkv[:, D:], 2 * D, B, H, N, hd, a.scale)
        Wqkv = self._w(a.qkv.weight)
        gW = pk.g(a.qkv.weight)
        ln1_cls = ln1.view(B, N * D)[:, :D]
        ops.gemm(dkv, ln1, gW[D:], a_kmajor=False, b_kmajor=False)
        ops.gemm(dq, ln1_cls, gW[:D], a_kmajor=False, b_kmajor=False)
        if a.qkv.bias is not None:
            gb = pk.g(a.qkv.bias)
            ops.colsum(dkv, gb[D:])
            ops.colsum(dq, gb[:D])
        # d ln1 = dkv Wkv (+ dq Wq on the CLS rows), accumulated in fp32
        dln1 = self._alloc(M, D, f32, dev)
        self._gemm(dkv, Wqkv[D:], dln1, b_kmajor=False)
        ops.gemm(dq, Wqkv[:D], dln1.view(B, N * D)[:, :D], b_kmajor=False, accumulate=True)
        # residual gradient entering the block: zero except the CLS rows (= G1), plus LN1 backward
        G = self._alloc(M, D, R, dev, zero=True)
        ops.scale_cast(G1, G.view(B, N * D), M=B, N=D, ldo=N * D)
        Gb = None if T == R else self._alloc(M, D, T, dev)
        ops.layernorm_bwd(dln1, X, mean1, rstd1, pk.f32(blk.norm1.weight), G, G, Gb,
                          pk.g(blk.norm1.weight), pk.g(blk.norm1.bias),
                          gsum=pk.g(prev_fc2_bias) if prev_fc2_bias is not None else None, M=M, D=D, fold=self.folds)
        return G, (G if Gb is None else Gb)

    # -- backward ------------------------------------------------------------
    def _backward(self, dout):
        s = self._take_saved()
        m, T, R, pk = self.model, self.T, self.R, self.pack
        B, N, M, D, H, hd = s["B"], s["N"], s["M"], s["D"], s["H"], s["hd"]
        dev = dout.device

        def new(rows, cols, dt):
            return self._alloc(rows, cols, dt, dev)

        dfeat = head_backward(pk, self.head, s["head"], dout.contiguous().float())

        # ---- final LayerNorm on the CLS rows -> residual-stream gradient G ----
        blocks_list = list(m.blocks)
        if s.get("last_cls") is not None:
            # CLS-only last block: the stream after it is [B, D]; its backward rebuilds the full-width gradient
            Gc = torch.empty((B, D), dtype=R, device=dev)
            ops.layernorm_bwd(dfeat, s["Xf"], s["meanf"], s["rstdf"], pk.f32(m.norm.weight), None, Gc, None,
                              pk.g(m.norm.weight), pk.g(m.norm.bias), M=B, D=D, dy_stride=D, x_stride=D, g_stride=D,
                              fold=self.folds)
            self._ready(m.norm, m.head)
            last = blocks_list.pop()
            prev = blocks_list[-1].mlp.fc2.bias if blocks_list else None
            G, Gb = self._last_block_cls_bwd(last, s["last_cls"], Gc, B, N, M, D, H, hd, dev, prev)
            s["last_cls"] = None
            self._ready(last)
        else:
            G = self._alloc(M, D, R, dev, zero=True)
            # gsum of an LN backward = column sum of the gradient it leaves in G = the bias
            # gradient of the Linear (fc2 / proj) that wrote that residual position
            last_fc2_bias = m.blocks[-1].mlp.fc2.bias
            ops.layernorm_bwd(dfeat, s["Xf"], s["meanf"], s["rstdf"], pk.f32(m.norm.weight), None, G, None,
                              pk.g(m.norm.weight), pk.g(m.norm.bias), gsum=pk.g(last_fc2_bias), M=B, D=D,
                              dy_stride=D, x_stride=N * D, g_stride=N * D, fold=self.folds)
            self._ready(m.norm, m.head)
            if T == R:
                Gb = G                      # GEMM operand and residual gradient share one buffer
            else:
                Gb = new(M, D, T)
                ops.cast(G, Gb)
        gb_out = None if T == R else Gb

        saved_blocks = s["blocks"]
        for bi in range(len(blocks_list) - 1, -1, -1):
            blk = blocks_list[bi]
            sv = saved_blocks.pop()      # release each block's activations as we go
            X, ln1, mean1, rstd1, qkv, O, lse, X1, ln2, mean2, rstd2, pre, hid = sv
            del sv
            a, mlp = blk.attn, blk.mlp
            # MLP branch
            dln2 = mlp_backward(self, mlp, Gb, ln2, pre, hid)
            ops.layernorm_bwd(dln2, X1, mean2, rstd2, pk.f32(blk.norm2.weight), G, G, gb_out,
                              pk.g(blk.norm2.weight), pk.g(blk.norm2.bias), gsum=pk.g(a.proj.bias),
                              M=M, D=D, fold=self.folds)
            # attention branch
            dO = new(M, D, T)
            self._gemm(Gb, self._w(a.proj.weight), dO, b_kmajor=False)
            dqkv = new(M, 3 * D, T)
            # the qkv bias gradient rides on the attention backward (per-row-block column sums, folded by a tiny colsum)
            dqkv_part = None
            if T == torch.bfloat16 and a.qkv.bias is not None:
                dqkv_part = torch.empty((ops.attn_bwd_dbias_rows(B, N), 3 * D), dtype=torch.float32, device=dev)
            ops.attn_bwd(qkv, O, dO, lse, dqkv, B, N, H, hd, a.scale, dbias_part=dqkv_part, launch_flags=reducer_flags(self))
            # the proj and qkv weight gradients share one split-K launch (Gb still holds this block's G' here: the
            # LayerNorm backward below is what overwrites it)
            engine_wgrad_pair(self, Gb, O, pk.g(a.proj.weight), dqkv, ln1, pk.g(a.qkv.weight))
            if a.qkv.bias is not None:
                ops.colsum(dqkv_part if dqkv_part is not None else dqkv, pk.g(a.qkv.bias), fold=self.folds)
            dln1 = new(M, D, T)
            self._gemm(dqkv, self._w(a.qkv.weight), dln1, b_kmajor=False)
            # the gradient this leaves in G flows into the previous block's fc2 output
            prev_fc2_bias = blocks_list[bi - 1].mlp.fc2.bias if bi > 0 else None
            ops.layernorm_bwd(dln1, X, mean1, rstd1, pk.f32(blk.norm1.weight), G, G, gb_out,
                              pk.g(blk.norm1.weight), pk.g(blk.norm1.bias),
                              gsum=pk.g(prev_fc2_bias) if prev_fc2_bias is not None else None, M=M, D=D,
                              fold=self.folds)
            self._ready(blk)

        # ---- embeddings ----
        conv = m.patch_embed.proj
        Kp = s["Kp"]
        dpos = torch.empty(N * D, dtype=torch.float32, device=dev)
        ops.colsum(G, dpos, M=B, N=N * D, ld=N * D)          # sum over the batch
        ops.cast(dpos[:D], pk.g(m.cls_token).view(-1))       # d cls = d pos[0]
        if s["pos_tabs"] is None:
            ops.cast(dpos, pk.g(m.pos_embed).view(-1))
        else:   # through the bicubic resize: the transposed tap table
            ops.pos_resample(dpos.view(N, D), s["pos_tabs"].bwd, pk.g(m.pos_embed).view(-1, D))
        self._gemm(Gb, s["patches"], pk.g(conv.weight).view(D, Kp), a_kmajor=False, b_kmajor=False)
        if conv.bias is not None:
            ops.colsum(dpos[D:].view(N - 1, D), pk.g(conv.bias))  # CLS rows carry no conv bias
        self._ready(m.cls_token, m.pos_embed, m.patch_embed)
