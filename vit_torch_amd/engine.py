"""Engine core shared by VitEngine (vit.py), CaitEngine (cait.py) and SwinEngine (swin.py).

Each engine orders the kernel launches of its model and writes the backward pass by hand; what is the same around that
order lives here: the GEMM launch wrapper (`engine_gemm`: bf16x3 mode, row padding, reducer launch flags) over the one
flag lookup (`reducer_flags`) and the one event bracket (`profiled_launch`), the `Engine` base class (construction,
parameter pack, gradient bookkeeping), the MLP half-block of a transformer block (`mlp_forward` / `mlp_backward`), the
autograd bridge (`_EngineFn`) and the `EngineModel` mixin that gives the model classes their `engine()` / `forward()`.

The modules that run without an engine (head.ClassifierHead and xcit's XCA, LPI, ConvPatchEmbed, PositionalEncodingFourier,
ClassAttentionBlock, XCABlock) share the `PackedModule` mixin and its one autograd bridge (`_PackedFn`) at the end of this file.
"""
from __future__ import annotations

import os
from typing import List, Optional

import torch
import torch.nn as nn

from . import ops
from ._lib import EPI_BIAS_GELU, EPI_DGELU, EPI_RESIDUAL, LAUNCH_ROWS_PADDED, VitmiError
from .packing import ParamPack


def _head_layers(head) -> Optional[List[tuple]]:
    """[(Linear, gelu_after)] for Identity / Linear / Sequential(Linear[,GELU]...) heads
    (/root/reference/models/vision_all.py:299-320); None if the head is something else."""
    if isinstance(head, nn.Identity):
        return []
    if isinstance(head, nn.Linear):
        return [(head, False)]
    if isinstance(head, nn.Sequential):
        out = []
        mods = list(head)
        i = 0
        while i < len(mods):
            if not isinstance(mods[i], nn.Linear):
                return None
            gelu = i + 1 < len(mods) and isinstance(mods[i + 1], nn.GELU)
            out.append((mods[i], gelu))
            i += 2 if gelu else 1
        return out
    return None


def _rows_padded(*tensors) -> bool:
    """True when every given [M, .] tensor's storage reaches ceil256(M) rows at its row stride."""
    for t in tensors:
        if t is None or t.dim() != 2:
            continue
        rows = (t.shape[0] + 255) // 256 * 256
        need = (t.storage_offset() + (rows - 1) * t.stride(0) + t.shape[1]) * t.element_size()
        if t.untyped_storage().nbytes() < need:
            return False
    return True


def reducer_flags(eng, passed=None) -> int:
    """The `launch_flags` of one launch: what the caller passed, else the reducer's (gradient buckets in flight: share
    the device with RCCL's kernels), else 0.  GradReducer.launch_flags() spends a credit, so it is asked only for a
    launch that will carry its answer."""
    if passed is not None:
        return passed
    return eng.reducer.launch_flags() if eng.reducer is not None else 0


def profiled_launch(eng, name, shape, flops, launch):
    """Run launch(); when eng.profile is a list, bracket it by two HIP events on the launch stream and append
    (name, shape, flops, start_event, end_event) (bench.py's roofline leg)."""
    if eng.profile is None:
        return launch()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = launch()
    e1.record()
    eng.profile.append((name, shape, flops, e0, e1))
    return out


def _profiled_gemm(eng, fn, prefix, A, B, C, k):
    """fn(A, B, C, **k) (ops.gemm / ops.gemm_split3) as a profiled launch of the algorithmic 2 M N K FLOPs."""
    if eng.profile is None:                 # the timed step: the launch is not even described
        return fn(A, B, C, **k)
    akm, bkm = k.get("a_kmajor", True), k.get("b_kmajor", True)
    Kdim = A.shape[1] if akm else A.shape[0]
    return profiled_launch(eng, prefix + ("n" if akm else "t") + ("t" if bkm else "n"), (C.shape[0], C.shape[1], Kdim),
                           2.0 * C.shape[0] * C.shape[1] * Kdim, lambda: fn(A, B, C, **k))


def _engine_gemm_split3(eng, A, B, C, **k):
    """engine_gemm in the "bf16x3" mode: fp32 operands -> three-part bf16 images -> ONE bf16 product over 3K on the tile
    kernels, fp32 epilogue (ops.gemm_split3).  Profiled launches count the algorithmic 2 M N K FLOPs (the mode's own
    roofline is a third of the bf16 peak)."""
    k["launch_flags"] = reducer_flags(eng, k.get("launch_flags"))
    if k.get("C2") is not None and k.get("epilogue") == EPI_RESIDUAL:
        # CaiT's LayerScale residual x + gamma * f(x) with the branch output f kept for d gamma (models/cait.py:143-150): the
        # tile kernel writes that second output in the OPERAND dtype (bf16 here), so the mode takes three steps, each the
        # reference's own rounding: f = A W^T + b (three-product GEMM, fp32; it carries the flags taken above), out = gamma * f,
        # out += x
        if k.get("rowscale") is not None or not (C.is_contiguous() and k["R"].is_contiguous()):
            raise VitmiError("compute_dtype='bf16x3': LayerScale residual with a DropPath row scale / strided rows is not built")
        f, R_, gamma = k.pop("C2"), k.pop("R"), k.pop("gamma", None)
        k.pop("epilogue")
        _engine_gemm_split3(eng, A, B, f, **k)
        ops.scale_cast(f, C, gamma, M=C.shape[0], N=C.shape[1])
        ops.axpy(R_.reshape(-1), C.reshape(-1), 1.0)
        return C
    return _profiled_gemm(eng, ops.gemm_split3, "gemm3_", A, B, C, k)


def engine_gemm(eng, A, B, C, **k):
    """ops.gemm for an engine: the bf16x3 mode, the GELU epilogues' derivative form, the reducer's launch flags, the
    row-padding flag, and profiling (profiled_launch)."""
    # the block MLPs keep gelu'(pre) instead of pre in bf16 mode: the GELU epilogue has the exp
    # at hand, and the backward epilogue becomes a multiply (vitmi_gemm_desc.aux_is_derivative).
    # fp32 (parity) mode keeps the pre-activation, as the reference's autograd does.
    if eng.split3 and A.dtype == torch.float32:
        return _engine_gemm_split3(eng, A, B, C, **k)
    if k.get("epilogue") in (EPI_BIAS_GELU, EPI_DGELU):
        k.setdefault("aux_deriv", eng.T == torch.bfloat16)
    k["launch_flags"] = reducer_flags(eng, k.get("launch_flags"))
    if eng.pad_rows and _rows_padded(C, k.get("C2"), k.get("R"), k.get("aux")):
        # every [M, .] activation of this engine comes from _alloc (rows rounded up to 256); the flag is only passed when the
        # storage behind each row-indexed output / side input really covers the padding (a future torch.empty
        # output would otherwise be a silent out-of-bounds write of up to 255 rows)
        k["launch_flags"] |= LAUNCH_ROWS_PADDED
    return _profiled_gemm(eng, ops.gemm, "gemm_", A, B, C, k)


def engine_wgrad_pair(eng, dY0, X0, dW0, dY1, X1, dW1):
    """dW0 = dY0^T X0 and dW1 = dY1^T X1 (the proj and qkv weight gradients of an attention block) in one launch where
    the library pairs them (ops.gemm_pair / vitmi_gemm_pair), else as two GEMMs."""
    paired = (dY0.dtype == torch.bfloat16 and dW0.dtype == torch.float32
              and ops.gemm_pair_shares_a_launch(dW0.shape[0], dW0.shape[1], dW1.shape[0], dW1.shape[1], dY0.shape[0]))
    if not paired:
        eng._gemm(dY0, X0, dW0, a_kmajor=False, b_kmajor=False)
        eng._gemm(dY1, X1, dW1, a_kmajor=False, b_kmajor=False)
        return
    flags = reducer_flags(eng)
    if eng.profile is None:                 # as in _profiled_gemm
        return ops.gemm_pair(dY0, X0, dW0, dY1, X1, dW1, launch_flags=flags)
    K = dY0.shape[0]
    profiled_launch(eng, "gemm_tn_pair", (dW0.shape[0] + dW1.shape[0], dW0.shape[1], K),
                    2.0 * K * (dW0.shape[0] * dW0.shape[1] + dW1.shape[0] * dW1.shape[1]),
                    lambda: ops.gemm_pair(dY0, X0, dW0, dY1, X1, dW1, launch_flags=flags))


# ------------------------------------------------------------ MLP half-block --
def mlp_forward(eng, mlp, ln2, X1, save, **residual):
    """X2 = X1 + fc2(gelu(fc1(ln2))) into a new residual-stream buffer; `residual`: the model's extra arguments of the
    fc2 residual epilogue (CaiT's LayerScale gamma / branch output C2, Swin's DropPath rowscale).  Returns X2 and what
    mlp_backward needs of fc1's output (pre: None unless save)."""
    M, D = X1.shape
    Dh = mlp.fc1.out_features
    dev = X1.device
    pre = eng._alloc(M, Dh, eng.T, dev) if save else None     # what the backward needs of fc1's output (engine_gemm)
    hid = eng._alloc(M, Dh, eng.T, dev)
    eng._gemm(ln2, eng._w(mlp.fc1.weight), hid, epilogue=EPI_BIAS_GELU, bias=eng.pack.f32(mlp.fc1.bias), C2=pre)
    X2 = eng._alloc(M, D, eng.R, dev)
    eng._gemm(hid, eng._w(mlp.fc2.weight), X2, epilogue=EPI_RESIDUAL, bias=eng.pack.f32(mlp.fc2.bias), R=X1, **residual)
    return X2, pre, hid


def mlp_backward(eng, mlp, Gb, ln2, pre, hid):
    """Backward of mlp_forward's branch given Gb = its output gradient (operand dtype, [M, D]): the fc1 / fc2 weight
    gradients and the fc1 bias gradient (the fc2 bias gradient is the caller's).  Returns dln2."""
    pk = eng.pack
    M, D = Gb.shape
    Dh = mlp.fc1.out_features
    dev = Gb.device
    dH = eng._alloc(M, Dh, eng.T, dev)
    # the fc1 bias gradient rides on the kernel that produces dH (per-128-row column sums, folded by a tiny colsum)
    # whenever that kernel is the bf16 fast one; otherwise dH itself is summed
    part = None
    if eng.T == torch.bfloat16 and ops.gemm_uses_fast(M, Dh, D, b_kmajor=False, epilogue=EPI_DGELU, colsum_part=True):
        part = torch.empty(((M + 127) // 128, Dh), dtype=torch.float32, device=dev)
    eng._gemm(Gb, eng._w(mlp.fc2.weight), dH, b_kmajor=False, epilogue=EPI_DGELU, aux=pre, colsum_part=part)
    eng._gemm(Gb, hid, pk.g(mlp.fc2.weight), a_kmajor=False, b_kmajor=False)
    eng._gemm(dH, ln2, pk.g(mlp.fc1.weight), a_kmajor=False, b_kmajor=False)
    ops.colsum(dH if part is None else part, pk.g(mlp.fc1.bias), fold=eng.folds)
    dln2 = eng._alloc(M, D, eng.T, dev)
    eng._gemm(dH, eng._w(mlp.fc1.weight), dln2, b_kmajor=False)
    return dln2


# ------------------------------------------------------------------ engine --
class Engine:
    """What every engine holds: the model, its compute dtype T (bf16, or fp32 in the parity and bf16x3 modes) and
    residual-stream dtype R, the classifier head's layers, the flat parameter buffers (ParamPack) and the backward's
    bookkeeping.  Subclasses write forward(x, save) and _backward(dout)."""

    def __init__(self, model):
        self.model = model
        dev = model.norm.weight.device
        if dev.type != "cuda":
            raise VitmiError("move the model to the GPU before the first forward")
        self.T, self.R = model.compute_dtype, model.residual_dtype
        self.split3 = bool(model.split3)
        if self.T == torch.float32 and self.R != torch.float32:
            raise VitmiError("fp32 compute needs an fp32 residual stream")
        self.head = _head_layers(model.head) if model.apply_head else []
        if self.head is None:
            raise VitmiError("head must be Identity, Linear or Sequential(Linear[, GELU], ...)")
        self.pack = ParamPack(list(model.named_parameters()), dev, shadow=self.T == torch.bfloat16)
        self.saved = None
        self.reducer = None          # ddp.GradReducer: told when a section's grads are final
        self.profile = None          # list of (name, shape, flops, start_event, end_event) when profiling (profiled_launch)
        # (round 1 ran the weight-gradient GEMMs on a second HIP stream; A/B on one box,
        # profiles/r02_ab_overlap*: 38.47-38.67 ms/step without it, 38.55-39.26 with it — a
        # 256x256-tile GEMM workgroup owns its CU's whole register file and 128 KiB of LDS, so
        # two GEMM kernels only take CUs from each other.  Removed.)
        # the ~50 small folds of a backward pass (LayerNorm dgamma | dbeta | bias sums, fc1 / qkv bias partials) run as
        # ONE launch per flush instead of one each (ops.FoldQueue; VITMI_DEFER_FOLDS=0: fold at once, for A/B)
        self.folds = ops.FoldQueue() if os.environ.get("VITMI_DEFER_FOLDS", "1") != "0" else None
        # rows of every [M, .] activation from _alloc rounded up to the 256-row GEMM tile (VitEngine, bf16)
        self.pad_rows = False

    def is_current(self) -> bool:
        m = self.model
        return (self.pack.is_current() and m.compute_dtype == self.T and m.residual_dtype == self.R
                and bool(m.split3) == self.split3
                and len(self.pack.params) == sum(1 for _ in m.parameters()))

    # -- helpers -------------------------------------------------------------
    def _alloc(self, rows, cols, dt, dev, zero=False):
        r = (rows + 255) // 256 * 256 if self.pad_rows else rows
        t = (torch.zeros if zero else torch.empty)((r, cols), dtype=dt, device=dev)
        return t[:rows]

    def _w(self, p):
        return self.pack.w(p)

    def _gemm(self, A, B, C, **k):
        return engine_gemm(self, A, B, C, **k)

    def _ready(self, *mods_or_params):
        """The gradients of these modules / parameters are final: their section of the flat buffer may leave.  Over one
        backward the sections tile the whole pack: a parameter the engine never writes (the head of a model built with
        `apply_head=False`) is announced with its neighbours, zeros included, so every rank steps on the same buffer."""
        if self.reducer is None:
            return
        if self.folds is not None:
            self.folds.flush()              # the section's bias / LayerNorm gradients must be final before its bucket leaves
        ps = []
        for o in mods_or_params:
            ps.extend(o.parameters() if isinstance(o, nn.Module) else [o])
        self.reducer.section_ready(ps)

    # -- backward ------------------------------------------------------------
    def backward(self, dout):
        try:
            self._backward(dout)
            if self.folds is not None:
                self.folds.flush()
            if self.reducer is not None:
                self.reducer.finish()
        except BaseException:
            if self.folds is not None:
                self.folds.clear()
            if self.reducer is not None:
                self.reducer.abort()
            raise

    def _take_saved(self):
        return take_saved(self, "saved")


def take_saved(owner, attr):
    """The saved forward kept in owner.<attr>, handed out once."""
    s = getattr(owner, attr)
    if s is None:
        raise VitmiError("backward called without a saved forward (or called twice)")
    setattr(owner, attr, None)
    return s


def param_grads(pack):
    """The parameter gradients a backward returns to autograd: the pack's fresh gradient views, None for a parameter
    that needs none or whose .grad already IS this buffer (zero_grad(set_to_none=False))."""
    grads = []
    for p, gv in zip(pack.params, pack.fresh_grad_views()):
        if not p.requires_grad:
            grads.append(None)
        elif p.grad is not None and p.grad.data_ptr() == gv.data_ptr():
            grads.append(None)
        else:
            grads.append(gv)
    return grads


class _EngineFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, eng, x, *params):
        ctx.eng = eng
        return eng.forward(x, save=True)

    @staticmethod
    def backward(ctx, dout):
        eng = ctx.eng
        held = eng.pack.begin_backward()        # .grad tensors that alias the flat buffer: accumulate, do not overwrite
        eng.backward(dout)
        eng.pack.end_backward(held)
        return (None, None, *param_grads(eng.pack))


class EngineModel:
    """engine() / forward() of a model that runs on an Engine.  The model sets `self._engine = None` in __init__ and
    defines `_new_engine()`; resetting `_engine` to None forces a rebuild (checkpoint.py)."""

    def engine(self):
        if self._engine is None or not self._engine.is_current():
            self._engine = self._new_engine()
        return self._engine

    def forward(self, x):
        if not x.is_cuda:
            raise VitmiError("vit_torch_amd models run on an MI355X (HIP) device; got a CPU tensor "
                             "and there is no CPU fallback")
        eng = self.engine()
        if torch.is_grad_enabled() and any(p.requires_grad for p in eng.pack.params):
            return _EngineFn.apply(eng, x, *eng.pack.params)
        return eng.forward(x, save=False)


# ------------------------------------------------------- stand-alone modules --
class _PackedFn(torch.autograd.Function):
    """The autograd bridge of every PackedModule; `extra`: the forward's non-tensor arguments as a plain tuple."""

    @staticmethod
    def forward(ctx, mod, x, extra, *params):
        ctx.mod = mod
        ctx.need_dx = x.requires_grad
        return mod._forward(x, *extra, save=True)

    @staticmethod
    def backward(ctx, dout):
        mod = ctx.mod
        held = mod._pack.begin_backward()       # torch's accumulation contract (packing.ParamPack.begin_backward)
        dx = mod._backward(dout, ctx.need_dx)
        mod._pack.end_backward(held)
        return (None, dx, None, *param_grads(mod._pack))


class PackedModule:
    """Mixin of an nn.Module that runs on libvitmi kernels by itself (ClassifierHead, xcit's modules), not inside a model's
    Engine: its parameters live in a ParamPack (the fused optimizers update them) and one autograd.Function carries
    its forward and backward.  It holds plain attributes only: nothing enters a state_dict, and parameter names, order
    and pack layout are the module's own.  A subclass lists it BEFORE its nn.Module base, sets `pack_shadow` where its
    GEMMs read the pack's bf16 weight shadows, checks its input in `forward` (`_refuse_cpu`, its shapes) and ends it with
    `self._run(x, *extra)`, and names its kernels, plain functions over any pack: `kernels = (forward, backward)` with
    `forward(pack, m, x, *extra, save) -> (out, saved)` and `backward(pack, m, saved, dout, need_dx) -> dL/dx or None`, which
    writes the parameter gradients into the pack (`pack.g(p)`).  The mixin refreshes the shadow before the forward and keeps
    `saved` in `self._saved` between the two; a subclass with more to do overrides `_forward` / `_backward`."""
    _pack = None
    _saved = None
    pack_shadow = False
    kernels = None

    def engine(self):
        """(Re)build the flat parameter buffers (after .to(device) / load_state_dict)."""
        dev = next(self.parameters()).device
        if dev.type != "cuda":
            raise VitmiError(f"move the {type(self).__name__} to the GPU before the first forward")
        if self._pack is None or not self._pack.is_current() or len(self._pack.params) != sum(1 for _ in self.parameters()):
            self._pack = ParamPack(list(self.named_parameters()), dev, shadow=self.pack_shadow)
        return self

    @property
    def pack(self):
        return self.engine()._pack

    def _refuse_cpu(self, x):
        if not x.is_cuda:
            raise VitmiError(f"vit_torch_amd.{type(self).__name__} runs on an MI355X (HIP) device; got a CPU tensor "
                             "and there is no CPU fallback")

    def _run(self, x, *extra):
        self.engine()
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self._pack.params)):
            return _PackedFn.apply(self, x, extra, *self._pack.params)
        return self._forward(x, *extra, save=False)

    def _forward(self, x, *extra, save):
        self._pack.refresh_shadow()
        out, saved = self.kernels[0](self._pack, self, x, *extra, save=save)
        if save:
            self._saved = saved
        return out

    def _backward(self, dout, need_dx):
        return self.kernels[1](self._pack, self, self._take_saved(), dout, need_dx)

    def _take_saved(self):
        return take_saved(self, "_saved")
