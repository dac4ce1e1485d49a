"""Stand-alone classifier head on libvitmi kernels (linear evaluation: SURVEY §8f rank 2).

`VisionModelZoo.get_classifier_head` (/root/reference/models/vision_all.py:299-320) returns
`Sequential(Linear(bias=True), GELU, ..., Linear(out, bias=False))`.  When that head is part of a
model, the model's engine runs it; in the reference's linear-evaluation mode
(`main.py:184-201`) it is a module of its own, trained on the features of a frozen backbone
(`utils_network.py:143,202-206,413-415`).  `ClassifierHead` is that module: the same
`nn.Sequential` structure and state-dict keys ("0.weight", "0.bias", "2.weight", ...), but
`forward` / `backward` run the fp32 MFMA GEMM with fused bias+GELU / gelu' epilogues, and its
parameters live in a `ParamPack`, so `FusedSGD` updates them.  CPU tensors raise: no fallback.  The pack, the autograd
bridge and the dispatch are `engine.PackedModule`'s; here are the head's kernels, its reducer hand-off and the early
return of an empty head.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import ops
from ._lib import EPI_BIAS_GELU, EPI_DGELU, VitmiError
from .engine import PackedModule, _head_layers


def head_forward(pack, layers, x):
    """x [B, in] fp32 through the [(Linear, gelu_after)] layers (engine._head_layers): tiny fp32 GEMMs on the generic MFMA
    kernel, bias and GELU in the epilogue.  Returns the output and what head_backward needs."""
    acts, pres, cur = [x], [], x
    for lin, gelu in layers:
        out = torch.empty((x.shape[0], lin.out_features), dtype=torch.float32, device=x.device)
        bias = pack.f32(lin.bias) if lin.bias is not None else None
        if gelu:
            pre = torch.empty_like(out)
            ops.gemm(cur, pack.f32(lin.weight), out, epilogue=EPI_BIAS_GELU, bias=bias, C2=pre)
        else:
            pre = None
            ops.gemm(cur, pack.f32(lin.weight), out, bias=bias)
        pres.append(pre)
        acts.append(out)
        cur = out
    return cur, (acts, pres)


def head_backward(pack, layers, saved, d, need_dx=True):
    """Backward of head_forward: d = dL/d output (fp32, contiguous).  Writes the layers' gradients into the pack and
    returns dL/dx (None when not need_dx)."""
    # z_i = a_i W_i^T + b_i ; a_{i+1} = gelu(z_i) or z_i.  `d` is dL/dz_i on entry;
    # the inner layer's gelu' is applied by the DGELU epilogue of this layer's dX GEMM.
    acts, pres = saved
    if layers and layers[-1][1]:
        raise VitmiError("a head ending in GELU is not supported")
    for li in range(len(layers) - 1, -1, -1):
        lin, _ = layers[li]
        ops.gemm(d, acts[li], pack.g(lin.weight), a_kmajor=False, b_kmajor=False)
        if lin.bias is not None:
            ops.colsum(d, pack.g(lin.bias))
        if li == 0 and not need_dx:
            return None
        dx = torch.empty((d.shape[0], lin.in_features), dtype=torch.float32, device=d.device)
        if li > 0 and layers[li - 1][1]:
            ops.gemm(d, pack.f32(lin.weight), dx, b_kmajor=False, epilogue=EPI_DGELU, aux=pres[li - 1])
        else:
            ops.gemm(d, pack.f32(lin.weight), dx, b_kmajor=False)
        d = dx
    return d


class ClassifierHead(PackedModule, nn.Sequential):
    kernels = (lambda pack, m, x, save: head_forward(pack, m._layers, x), None)      # the backward: _backward, with the reducer

    def __init__(self, *layers):
        super().__init__(*layers)
        self._layers = _head_layers(self)
        if self._layers is None:
            raise VitmiError("ClassifierHead: layers must be Linear[, GELU], ..., Linear")
        self.reducer = None          # ddp.GradReducer (Network(ddp=...)): the head's gradients leave as one bucket after its backward

    def forward(self, x):
        self._refuse_cpu(x)
        if not self._layers:
            return x
        return self._run(x.float().contiguous())

    def _backward(self, dout, need_dx):
        try:
            dx = head_backward(self._pack, self._layers, self._take_saved(), dout.contiguous().float(), need_dx)
        except BaseException:
            if self.reducer is not None:
                self.reducer.abort()
            raise
        if self.reducer is not None:         # data-parallel linear evaluation: all of the head's gradients are final here
            self.reducer.section_ready([p for p in self._pack.params if p.requires_grad])
            self.reducer.finish()
        return dx
