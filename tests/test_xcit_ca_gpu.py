"""The class-attention block's glue kernels (csrc/xcit_glue.hip: ops.ca_merge_fwd / ca_merge_bwd / ca_out_fwd / ca_out_bwd) and
the ClassAttentionBlock module on the GPU.

Metric: max |got - want| / max |want| (xcit_ca_util.rel).  Every check prints its error beside its bound (-s).
References are float64 (xcit_ca_util), pinned to the reference's class by tests/golden/xcit_ca.npz (test_xcit_ca_cpu.py);
the fixture cases run the module on the fixture's inputs and state.

Bounds, measured on the CPU by test_xcit_ca_cpu.py and frozen here, rounded up (rules of test_convembed_gpu.py /
test_lpi_gpu.py):
  * fp32: 4x the error of the float32 closed form (xcit_ca_util.closed_block / glue_reference in float32) against float64 on
    the same inputs (F32_*).
  * bf16: 2x the error of the float64 emulation that carries exactly the declared roundings (the weight shadows; the stored
    activations l, [k v], q, o, a, the MLP's operand, gelu'(pre), the hidden row, m; the stored gradients gm, dH, da, do, dq,
    dk, dv) plus 4x the float32 figure of the same tensor (EMU_*): the emulation runs in float64 and carries nothing of the
    fp32 accumulation the bf16 path also has.
  * the glue kernels' branch tensors (l, a, m) are bf16-representable, so both dtypes see the same operands; only da and gm
    are rounded on store.  dx2 (G or 2 G) is exact.
  * exact: a zero dout gives exactly zero gradients and a zero dx.
Measured on an MI355X (one run; DESIGN.md 4.8 has the list).
"""
import os

import pytest
import torch

import fixture_codec as FC
import xcit_ca_util as U
from vit_torch_amd import ClassAttentionBlock, FusedSGD, VitmiError, ops

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])

F32_MODULE = {
    "fixture-tn": {"out": 1.53e-07, "dx": 1.12e-07, "grad/gamma1": 1.16e-07, "grad/gamma2": 1.46e-07, 
        "grad/norm1.weight": 7.30e-08, "grad/norm1.bias": 1.01e-07, "grad/attn.qkv.weight": 1.58e-07, 
        "grad/attn.qkv.bias": 1.79e-07, "grad/attn.proj.weight": 2.77e-07, "grad/attn.proj.bias": 1.90e-07, 
        "grad/norm2.weight": 1.18e-07, "grad/norm2.bias": 4.10e-08, "grad/mlp.fc1.weight": 2.24e-07, 
        "grad/mlp.fc1.bias": 1.84e-07, "grad/mlp.fc2.weight": 1.56e-07, "grad/mlp.fc2.bias": 0.0},
    "fixture-cls": {"out": 8.79e-08, "dx": 8.13e-08, "grad/gamma1": 4.81e-08, "grad/gamma2": 2.12e-07, 
        "grad/norm1.weight": 1.02e-07, "grad/norm1.bias": 1.13e-07, "grad/attn.qkv.weight": 2.75e-07, 
        "grad/attn.qkv.bias": 1.19e-07, "grad/attn.proj.weight": 2.91e-07, "grad/attn.proj.bias": 1.11e-07, 
        "grad/norm2.weight": 1.36e-07, "grad/norm2.bias": 8.73e-08, "grad/mlp.fc1.weight": 1.63e-07, 
        "grad/mlp.fc1.bias": 1.27e-07, "grad/mlp.fc2.weight": 2.07e-07, "grad/mlp.fc2.bias": 0.0},
    "single-patch-tn": {"out": 1.21e-07, "dx": 8.67e-08, "grad/gamma1": 1.76e-07, "grad/gamma2": 2.82e-07, 
        "grad/norm1.weight": 2.26e-07, "grad/norm1.bias": 1.21e-07, "grad/attn.qkv.weight": 1.42e-07, 
        "grad/attn.qkv.bias": 2.31e-07, "grad/attn.proj.weight": 2.54e-07, "grad/attn.proj.bias": 1.40e-07, 
        "grad/norm2.weight": 6.06e-08, "grad/norm2.bias": 1.03e-07, "grad/mlp.fc1.weight": 2.21e-07, 
        "grad/mlp.fc1.bias": 2.56e-07, "grad/mlp.fc2.weight": 1.65e-07, "grad/mlp.fc2.bias": 3.58e-08},
    "single-patch-cls": {"out": 5.25e-08, "dx": 7.83e-08, "grad/gamma1": 1.06e-07, "grad/gamma2": 2.82e-07, 
        "grad/norm1.weight": 2.30e-07, "grad/norm1.bias": 7.47e-08, "grad/attn.qkv.weight": 1.42e-07, 
        "grad/attn.qkv.bias": 2.31e-07, "grad/attn.proj.weight": 2.54e-07, "grad/attn.proj.bias": 1.40e-07, 
        "grad/norm2.weight": 2.33e-07, "grad/norm2.bias": 1.73e-07, "grad/mlp.fc1.weight": 2.21e-07, 
        "grad/mlp.fc1.bias": 2.56e-07, "grad/mlp.fc2.weight": 1.65e-07, "grad/mlp.fc2.bias": 3.58e-08},
    "n197-hd48-tn": {"out": 1.38e-07, "dx": 1.25e-07, "grad/gamma1": 2.22e-07, "grad/gamma2": 1.54e-07, 
        "grad/norm1.weight": 2.95e-07, "grad/norm1.bias": 9.18e-08, "grad/attn.qkv.weight": 5.24e-07, 
        "grad/attn.qkv.bias": 4.79e-07, "grad/attn.proj.weight": 3.94e-07, "grad/attn.proj.bias": 1.93e-07, 
        "grad/norm2.weight": 1.40e-07, "grad/norm2.bias": 5.35e-08, "grad/mlp.fc1.weight": 3.69e-07, 
        "grad/mlp.fc1.bias": 2.45e-07, "grad/mlp.fc2.weight": 1.76e-07, "grad/mlp.fc2.bias": 3.59e-08},
    "n197-hd48-cls": {"out": 9.46e-08, "dx": 1.15e-07, "grad/gamma1": 1.50e-07, "grad/gamma2": 1.54e-07, 
        "grad/norm1.weight": 1.76e-07, "grad/norm1.bias": 1.21e-07, "grad/attn.qkv.weight": 5.24e-07, 
        "grad/attn.qkv.bias": 4.79e-07, "grad/attn.proj.weight": 3.94e-07, "grad/attn.proj.bias": 1.93e-07, 
        "grad/norm2.weight": 1.34e-07, "grad/norm2.bias": 1.52e-07, "grad/mlp.fc1.weight": 3.69e-07, 
        "grad/mlp.fc1.bias": 2.45e-07, "grad/mlp.fc2.weight": 1.76e-07, "grad/mlp.fc2.bias": 3.59e-08},
    "n197-hd64-tn": {"out": 1.30e-07, "dx": 1.46e-07, "grad/gamma1": 1.15e-07, "grad/gamma2": 1.43e-07, 
        "grad/norm1.weight": 1.02e-07, "grad/norm1.bias": 1.28e-07, "grad/attn.qkv.weight": 4.35e-07, 
        "grad/attn.qkv.bias": 2.90e-07, "grad/attn.proj.weight": 4.34e-07, "grad/attn.proj.bias": 2.10e-07, 
        "grad/norm2.weight": 9.10e-08, "grad/norm2.bias": 4.11e-08, "grad/mlp.fc1.weight": 3.61e-07, 
        "grad/mlp.fc1.bias": 2.48e-07, "grad/mlp.fc2.weight": 2.17e-07, "grad/mlp.fc2.bias": 5.03e-08},
    "n197-hd64-cls": {"out": 9.13e-08, "dx": 1.11e-07, "grad/gamma1": 1.12e-07, "grad/gamma2": 1.43e-07, 
        "grad/norm1.weight": 8.51e-08, "grad/norm1.bias": 1.01e-07, "grad/attn.qkv.weight": 4.35e-07, 
        "grad/attn.qkv.bias": 2.90e-07, "grad/attn.proj.weight": 4.34e-07, "grad/attn.proj.bias": 2.10e-07, 
        "grad/norm2.weight": 1.05e-07, "grad/norm2.bias": 1.08e-07, "grad/mlp.fc1.weight": 3.61e-07, 
        "grad/mlp.fc1.bias": 2.48e-07, "grad/mlp.fc2.weight": 2.17e-07, "grad/mlp.fc2.bias": 5.03e-08},
    "n785-hd32-tn": {"out": 1.14e-07, "dx": 1.42e-07, "grad/gamma1": 2.54e-07, "grad/gamma2": 1.17e-07, 
        "grad/norm1.weight": 1.97e-07, "grad/norm1.bias": 1.10e-07, "grad/attn.qkv.weight": 3.08e-07, 
        "grad/attn.qkv.bias": 1.66e-07, "grad/attn.proj.weight": 2.23e-07, "grad/attn.proj.bias": 6.84e-08, 
        "grad/norm2.weight": 1.18e-07, "grad/norm2.bias": 6.03e-08, "grad/mlp.fc1.weight": 2.77e-07, 
        "grad/mlp.fc1.bias": 2.17e-07, "grad/mlp.fc2.weight": 1.94e-07, "grad/mlp.fc2.bias": 4.00e-08},
    "n785-hd32-cls": {"out": 9.94e-08, "dx": 1.18e-07, "grad/gamma1": 1.01e-07, "grad/gamma2": 1.17e-07, 
        "grad/norm1.weight": 1.20e-07, "grad/norm1.bias": 1.02e-07, "grad/attn.qkv.weight": 3.08e-07, 
        "grad/attn.qkv.bias": 1.66e-07, "grad/attn.proj.weight": 2.23e-07, "grad/attn.proj.bias": 6.84e-08, 
        "grad/norm2.weight": 1.06e-07, "grad/norm2.bias": 1.03e-07, "grad/mlp.fc1.weight": 2.77e-07, 
        "grad/mlp.fc1.bias": 2.17e-07, "grad/mlp.fc2.weight": 1.94e-07, "grad/mlp.fc2.bias": 4.00e-08},
    "wide-tn": {"out": 1.57e-07, "dx": 1.77e-07, "grad/gamma1": 1.86e-07, "grad/gamma2": 4.29e-07, 
        "grad/norm1.weight": 1.52e-07, "grad/norm1.bias": 2.34e-07, "grad/attn.qkv.weight": 6.83e-07, 
        "grad/attn.qkv.bias": 2.73e-07, "grad/attn.proj.weight": 4.33e-07, "grad/attn.proj.bias": 2.32e-07, 
        "grad/norm2.weight": 1.63e-07, "grad/norm2.bias": 1.43e-07, "grad/mlp.fc1.weight": 4.07e-07, 
        "grad/mlp.fc1.bias": 2.26e-07, "grad/mlp.fc2.weight": 4.33e-07, "grad/mlp.fc2.bias": 1.24e-07},
    "wide-cls": {"out": 1.29e-07, "dx": 1.33e-07, "grad/gamma1": 1.59e-07, "grad/gamma2": 4.29e-07, 
        "grad/norm1.weight": 1.51e-07, "grad/norm1.bias": 1.85e-07, "grad/attn.qkv.weight": 6.83e-07, 
        "grad/attn.qkv.bias": 2.73e-07, "grad/attn.proj.weight": 4.33e-07, "grad/attn.proj.bias": 2.32e-07, 
        "grad/norm2.weight": 1.95e-07, "grad/norm2.bias": 2.25e-07, "grad/mlp.fc1.weight": 4.07e-07, 
        "grad/mlp.fc1.bias": 2.26e-07, "grad/mlp.fc2.weight": 4.33e-07, "grad/mlp.fc2.bias": 1.24e-07},
}
EMU_MODULE = {
    "fixture-tn": {"out": 1.12e-03, "dx": 5.72e-04, "grad/gamma1": 1.40e-03, "grad/gamma2": 5.29e-03, 
        "grad/norm1.weight": 5.83e-04, "grad/norm1.bias": 9.74e-04, "grad/attn.qkv.weight": 5.63e-03, 
        "grad/attn.qkv.bias": 2.96e-03, "grad/attn.proj.weight": 4.10e-03, "grad/attn.proj.bias": 2.68e-03, 
        "grad/norm2.weight": 6.55e-04, "grad/norm2.bias": 1.73e-04, "grad/mlp.fc1.weight": 4.45e-03, 
        "grad/mlp.fc1.bias": 3.52e-03, "grad/mlp.fc2.weight": 5.50e-03, "grad/mlp.fc2.bias": 2.20e-03},
    "fixture-cls": {"out": 1.06e-03, "dx": 2.95e-04, "grad/gamma1": 1.39e-03, "grad/gamma2": 2.13e-03, 
        "grad/norm1.weight": 5.58e-04, "grad/norm1.bias": 6.17e-04, "grad/attn.qkv.weight": 4.69e-03, 
        "grad/attn.qkv.bias": 2.00e-03, "grad/attn.proj.weight": 5.50e-03, "grad/attn.proj.bias": 1.84e-03, 
        "grad/norm2.weight": 9.76e-04, "grad/norm2.bias": 7.10e-04, "grad/mlp.fc1.weight": 5.80e-03, 
        "grad/mlp.fc1.bias": 3.65e-03, "grad/mlp.fc2.weight": 4.07e-03, "grad/mlp.fc2.bias": 1.98e-03},
    "single-patch-tn": {"out": 2.19e-03, "dx": 1.60e-03, "grad/gamma1": 3.37e-03, "grad/gamma2": 8.38e-03, 
        "grad/norm1.weight": 3.06e-03, "grad/norm1.bias": 2.23e-03, "grad/attn.qkv.weight": 5.16e-03, 
        "grad/attn.qkv.bias": 5.41e-03, "grad/attn.proj.weight": 5.85e-03, "grad/attn.proj.bias": 3.61e-03, 
        "grad/norm2.weight": 1.54e-03, "grad/norm2.bias": 7.32e-04, "grad/mlp.fc1.weight": 6.50e-03, 
        "grad/mlp.fc1.bias": 5.67e-03, "grad/mlp.fc2.weight": 5.50e-03, "grad/mlp.fc2.bias": 1.85e-03},
    "single-patch-cls": {"out": 1.54e-03, "dx": 1.22e-03, "grad/gamma1": 2.20e-03, "grad/gamma2": 8.38e-03, 
        "grad/norm1.weight": 2.37e-03, "grad/norm1.bias": 1.66e-03, "grad/attn.qkv.weight": 5.16e-03, 
        "grad/attn.qkv.bias": 5.41e-03, "grad/attn.proj.weight": 5.85e-03, "grad/attn.proj.bias": 3.61e-03, 
        "grad/norm2.weight": 6.07e-03, "grad/norm2.bias": 2.14e-03, "grad/mlp.fc1.weight": 6.50e-03, 
        "grad/mlp.fc1.bias": 5.67e-03, "grad/mlp.fc2.weight": 5.50e-03, "grad/mlp.fc2.bias": 1.85e-03},
    "n197-hd48-tn": {"out": 1.04e-03, "dx": 4.96e-04, "grad/gamma1": 2.37e-03, "grad/gamma2": 5.52e-03, 
        "grad/norm1.weight": 3.66e-04, "grad/norm1.bias": 1.99e-04, "grad/attn.qkv.weight": 7.60e-03, 
        "grad/attn.qkv.bias": 6.04e-03, "grad/attn.proj.weight": 5.61e-03, "grad/attn.proj.bias": 1.92e-03, 
        "grad/norm2.weight": 1.04e-03, "grad/norm2.bias": 6.76e-05, "grad/mlp.fc1.weight": 5.14e-03, 
        "grad/mlp.fc1.bias": 3.36e-03, "grad/mlp.fc2.weight": 3.42e-03, "grad/mlp.fc2.bias": 1.81e-03},
    "n197-hd48-cls": {"out": 1.72e-03, "dx": 3.23e-04, "grad/gamma1": 2.12e-03, "grad/gamma2": 5.52e-03, 
        "grad/norm1.weight": 9.82e-05, "grad/norm1.bias": 7.81e-05, "grad/attn.qkv.weight": 7.60e-03, 
        "grad/attn.qkv.bias": 6.04e-03, "grad/attn.proj.weight": 5.61e-03, "grad/attn.proj.bias": 1.92e-03, 
        "grad/norm2.weight": 1.66e-03, "grad/norm2.bias": 1.63e-03, "grad/mlp.fc1.weight": 5.14e-03, 
        "grad/mlp.fc1.bias": 3.36e-03, "grad/mlp.fc2.weight": 3.42e-03, "grad/mlp.fc2.bias": 1.81e-03},
    "n197-hd64-tn": {"out": 1.01e-03, "dx": 8.88e-04, "grad/gamma1": 1.47e-03, "grad/gamma2": 3.51e-03, 
        "grad/norm1.weight": 2.62e-04, "grad/norm1.bias": 1.47e-04, "grad/attn.qkv.weight": 8.83e-03, 
        "grad/attn.qkv.bias": 4.33e-03, "grad/attn.proj.weight": 7.26e-03, "grad/attn.proj.bias": 3.75e-03, 
        "grad/norm2.weight": 5.91e-04, "grad/norm2.bias": 4.42e-05, "grad/mlp.fc1.weight": 7.84e-03, 
        "grad/mlp.fc1.bias": 5.54e-03, "grad/mlp.fc2.weight": 6.49e-03, "grad/mlp.fc2.bias": 2.76e-03},
    "n197-hd64-cls": {"out": 1.32e-03, "dx": 6.89e-04, "grad/gamma1": 1.26e-03, "grad/gamma2": 3.51e-03, 
        "grad/norm1.weight": 8.17e-05, "grad/norm1.bias": 1.28e-04, "grad/attn.qkv.weight": 8.83e-03, 
        "grad/attn.qkv.bias": 4.33e-03, "grad/attn.proj.weight": 7.26e-03, "grad/attn.proj.bias": 3.75e-03, 
        "grad/norm2.weight": 8.48e-04, "grad/norm2.bias": 1.22e-03, "grad/mlp.fc1.weight": 7.84e-03, 
        "grad/mlp.fc1.bias": 5.54e-03, "grad/mlp.fc2.weight": 6.49e-03, "grad/mlp.fc2.bias": 2.76e-03},
    "n785-hd32-tn": {"out": 1.02e-03, "dx": 3.48e-04, "grad/gamma1": 2.26e-03, "grad/gamma2": 3.63e-03, 
        "grad/norm1.weight": 2.90e-04, "grad/norm1.bias": 1.04e-04, "grad/attn.qkv.weight": 7.72e-03, 
        "grad/attn.qkv.bias": 3.41e-03, "grad/attn.proj.weight": 2.63e-03, "grad/attn.proj.bias": 2.23e-03, 
        "grad/norm2.weight": 6.61e-04, "grad/norm2.bias": 3.33e-05, "grad/mlp.fc1.weight": 5.14e-03, 
        "grad/mlp.fc1.bias": 3.67e-03, "grad/mlp.fc2.weight": 6.29e-03, "grad/mlp.fc2.bias": 1.75e-03},
    "n785-hd32-cls": {"out": 1.76e-03, "dx": 1.92e-04, "grad/gamma1": 1.08e-03, "grad/gamma2": 3.63e-03, 
        "grad/norm1.weight": 3.24e-05, "grad/norm1.bias": 3.93e-05, "grad/attn.qkv.weight": 7.72e-03, 
        "grad/attn.qkv.bias": 3.41e-03, "grad/attn.proj.weight": 2.63e-03, "grad/attn.proj.bias": 2.23e-03, 
        "grad/norm2.weight": 1.20e-03, "grad/norm2.bias": 1.24e-03, "grad/mlp.fc1.weight": 5.14e-03, 
        "grad/mlp.fc1.bias": 3.67e-03, "grad/mlp.fc2.weight": 6.29e-03, "grad/mlp.fc2.bias": 1.75e-03},
    "wide-tn": {"out": 1.22e-03, "dx": 6.69e-04, "grad/gamma1": 2.10e-03, "grad/gamma2": 5.15e-03, 
        "grad/norm1.weight": 1.67e-04, "grad/norm1.bias": 2.02e-04, "grad/attn.qkv.weight": 4.95e-03, 
        "grad/attn.qkv.bias": 3.44e-03, "grad/attn.proj.weight": 3.68e-03, "grad/attn.proj.bias": 2.14e-03, 
        "grad/norm2.weight": 1.21e-03, "grad/norm2.bias": 6.28e-05, "grad/mlp.fc1.weight": 5.29e-03, 
        "grad/mlp.fc1.bias": 2.54e-03, "grad/mlp.fc2.weight": 4.10e-03, "grad/mlp.fc2.bias": 1.69e-03},
    "wide-cls": {"out": 1.32e-03, "dx": 4.76e-04, "grad/gamma1": 2.22e-03, "grad/gamma2": 5.15e-03, 
        "grad/norm1.weight": 5.24e-05, "grad/norm1.bias": 1.32e-04, "grad/attn.qkv.weight": 4.95e-03, 
        "grad/attn.qkv.bias": 3.44e-03, "grad/attn.proj.weight": 3.68e-03, "grad/attn.proj.bias": 2.14e-03, 
        "grad/norm2.weight": 1.83e-03, "grad/norm2.bias": 1.68e-03, "grad/mlp.fc1.weight": 5.29e-03, 
        "grad/mlp.fc1.bias": 2.54e-03, "grad/mlp.fc2.weight": 4.10e-03, "grad/mlp.fc2.bias": 1.69e-03},
}
F32_GLUE = {"x1": 6.82e-08, "da": 5.05e-08, "dl": 4.24e-08, "dgamma1": 1.77e-07, "out": 3.80e-08, "dx2": 0.0, 
            "gm": 4.55e-08}
EMU_GLUE = {"x1": 0.0, "da": 3.04e-03, "dl": 0.0, "dgamma1": 0.0, "out": 0.0, "dx2": 0.0, "gm": 3.12e-03}


def module_bound(mode, case):
    """"fp32" 4x the float32 figure; "bf16" 2x the float64 emulation's error plus that (docstring)"""
    return {k: 4 * v + (2 * EMU_MODULE[case][k] if mode == "bf16" else 0.0) for k, v in F32_MODULE[case].items()}


def glue_bound(dtype):
    return {k: 4 * v + (2 * EMU_GLUE[k] if dtype == torch.bfloat16 else 0.0) for k, v in F32_GLUE.items()}


def judge(name, e, b):
    print(f"\n  {name}: " + "  ".join(f"{k} {v:.2e} ({b[k]:.1e})" for k, v in e.items()), end="")
    bad = {k: (v, b[k]) for k, v in e.items() if not v <= b[k]}
    assert not bad, f"{name}: over the bound: {bad}"


G = 1024


def guarded(shape, dtype):
    """a NaN tensor of `shape` between two NaN guard bands: (whole buffer, the view)"""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * G,), float("nan"), dtype=dtype, device="cuda")
    return buf, buf[G:G + n].view(shape)


def guards_untouched(buf, n):
    return bool(torch.isnan(buf[:G]).all() and torch.isnan(buf[G + n:]).all())


# ------------------------------------------------------------------------------------------- 1: the glue kernels ---
@DTYPES
@pytest.mark.parametrize("B,N1,D", U.GLUE_SHAPES, ids=[f"B{b}-N{n}-D{d}" for b, n, d in U.GLUE_SHAPES])
def test_glue_kernels_against_float64(B, N1, D, dtype):
    t = U.glue_inputs(B, N1, D)
    ref = U.glue_reference(t)
    f32 = torch.float32
    d = {k: v.cuda() for k, v in t.items()}
    l, a, m = (d[k].to(dtype) for k in ("l", "a", "m"))
    outs = {"x1": guarded((B, N1, D), f32), "da": guarded((B, D), dtype), "dl": guarded((B, N1, D), f32),
            "dgamma1": guarded((D,), f32), "out": guarded((B, N1, D), f32), "dx2": guarded((B, N1, D), f32),
            "gm": guarded((B, D), dtype)}
    o = {k: v[1] for k, v in outs.items()}
    ops.ca_merge_fwd(d["x"], a, l, d["g1"], o["x1"], B, N1, D)
    ops.ca_merge_bwd(d["G"], l, a, d["g1"], o["da"], o["dl"], o["dgamma1"], B, N1, D)
    ops.ca_out_fwd(d["xc"], d["x"], m, d["g2"], o["out"], B, N1, D)
    ops.ca_out_bwd(d["G"], d["g2"], o["dx2"], o["gm"], B, N1, D)
    torch.cuda.synchronize()
    for k, (buf, view) in outs.items():
        assert guards_untouched(buf, view.numel()) and not torch.isnan(view).any(), k
    assert torch.equal(o["dx2"].cpu().double(), ref["dx2"]) and not o["dl"][:, 0].any()
    judge(f"glue B{B} N1 {N1} D{D} {dtype}", {k: U.rel(o[k].float().cpu(), ref[k]) for k in U.GLUE_KEYS}, glue_bound(dtype))


def test_ca_out_fwd_reads_strided_cls_rows():
    """tokens_norm: the normed CLS rows are row 0 of each image of norm2's full output"""
    B, N1, D = 3, 7, 64
    t = U.glue_inputs(B, N1, D)
    x2, m, g2 = t["x"].cuda(), t["m"].cuda(), t["g2"].cuda()
    buf, out = guarded((B, N1, D), torch.float32)
    ops.ca_out_fwd(x2.view(B, N1 * D)[:, :D], x2, m, g2, out, B, N1, D)
    torch.cuda.synchronize()
    want = torch.cat([(t["x"][:, 0].double() + t["g2"].double() * t["m"].double()).unsqueeze(1), 2 * t["x"][:, 1:].double()], dim=1)
    assert guards_untouched(buf, out.numel())
    judge("strided xc", {"out": U.rel(out.cpu(), want)}, glue_bound(torch.float32))


def test_ca_merge_bwd_is_bitwise_repeatable():
    B, N1, D = 3, 197, 192
    t = {k: v.cuda() for k, v in U.glue_inputs(B, N1, D).items()}
    runs = []
    for _ in range(2):
        da, dl, dg = (torch.empty(s, device="cuda") for s in ((B, D), (B, N1, D), (D,)))
        ops.ca_merge_bwd(t["G"], t["l"], t["a"], t["g1"], da, dl, dg, B, N1, D)
        runs.append((da, dl, dg))
    torch.cuda.synchronize()
    assert all(torch.equal(p, q) for p, q in zip(*runs))


# -------------------------------------------------------------------------------------------------- 2: the module ---
@pytest.fixture(scope="module")
def fx():
    return FC.load(os.path.join(HERE, "golden", "xcit_ca.npz"))


def load_module(st, H, tokens_norm, mode):
    D, Dh = st["attn.proj.weight"].shape[0], st["mlp.fc1.weight"].shape[0]
    m = ClassAttentionBlock(D, H, mlp_ratio=Dh / D, qkv_bias=True, eta=0.5, tokens_norm=tokens_norm,
                            norm_layer=lambda d: torch.nn.LayerNorm(d, eps=U.EPS), compute_dtype=mode)
    m.load_state_dict(st)
    return m.cuda()


def run_module(m, x, dy):
    xd = x.cuda().requires_grad_(True)
    out = m(xd, 0, 0)
    out.backward(dy.cuda())
    torch.cuda.synchronize()
    assert out.dtype == torch.float32 and xd.grad.dtype == torch.float32
    return {"out": out.detach().cpu(), "dx": xd.grad.cpu(), **{"grad/" + n: p.grad.cpu() for n, p in m.named_parameters()}}


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["tn", "cls"])
def test_module_against_fixture(fx, name, mode):
    x, dy, st, H, tokens_norm, _ = U.fixture_case(fx, name)
    assert tokens_norm == (name == "tn")
    m = load_module(st, H, tokens_norm, mode)
    got = run_module(m, x, dy)
    judge(f"fixture {name} {mode}", U.errors(got, U.torch_block(x, dy, st, H, tokens_norm)), module_bound(mode, "fixture-" + name))
    first = {n: p.grad.clone() for n, p in m.named_parameters()}
    m(x.cuda(), 2, 3).backward(dy.cuda())                          # a second backward accumulates into .grad
    torch.cuda.synchronize()
    for n, p in m.named_parameters():
        assert torch.allclose(p.grad, 2 * first[n], rtol=1e-5, atol=1e-6), f"{n}: .grad did not accumulate"


CASE_NAMES = [c[0] for c in U.MODULE_CASES]


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("tokens_norm", [True, False], ids=["tn", "cls"])
@pytest.mark.parametrize("case", CASE_NAMES)
def test_module_against_float64(case, tokens_norm, mode):
    x, dy, st, H = U.module_case(case)
    got = run_module(load_module(st, H, tokens_norm, mode), x, dy)
    judge(f"{case} {'tn' if tokens_norm else 'cls'} {mode}", U.errors(got, U.module_reference(case, tokens_norm)),
          module_bound(mode, f"{case}-{'tn' if tokens_norm else 'cls'}"))


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("tokens_norm", [True, False], ids=["tn", "cls"])
def test_need_dx_false_and_zero_dout(fx, tokens_norm, mode):
    x, dy, st, H, _, _ = U.fixture_case(fx, "tn")
    m = load_module(st, H, tokens_norm, mode)
    with_dx = run_module(m, x, dy)
    m.zero_grad()
    m(x.cuda(), 2, 3).backward(dy.cuda())                          # x does not require grad: need_dx is False
    torch.cuda.synchronize()
    for n, p in m.named_parameters():
        assert torch.equal(p.grad.cpu(), with_dx["grad/" + n]), f"{n}: differs without dx"
    m.zero_grad()
    xd = x.cuda().requires_grad_(True)
    m(xd, 2, 3).backward(torch.zeros_like(xd))
    torch.cuda.synchronize()
    assert not xd.grad.any()
    for n, p in m.named_parameters():
        assert p.grad is not None and not p.grad.any(), f"{n}: a zero dout gave a non-zero gradient"


def test_backward_without_forward_raises(fx):
    x, dy, st, H, tn, _ = U.fixture_case(fx, "tn")
    m = load_module(st, H, tn, "bf16")
    m.engine()
    with pytest.raises(VitmiError, match="without a saved forward"):
        m._backward(dy.cuda(), True)
    with torch.no_grad():
        m(x.cuda(), 2, 3)                                           # a forward that keeps nothing
    with pytest.raises(VitmiError, match="without a saved forward"):
        m._backward(dy.cuda(), True)


def test_module_fused_sgd_step(fx):
    x, dy, st, H, tn, _ = U.fixture_case(fx, "cls")
    m = load_module(st, H, tn, "bf16")
    opt = FusedSGD(m.parameters(), lr=0.1, momentum=0.9)
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    m(x.cuda(), 2, 3).backward(dy.cuda())
    torch.cuda.synchronize()
    opt.step()
    torch.cuda.synchronize()
    for n, p in m.named_parameters():
        assert not torch.equal(p.detach(), before[n]), f"{n} did not move"
        assert torch.isfinite(p).all()


def test_module_graph_replay(fx):
    x, dy, st, H, tn, _ = U.fixture_case(fx, "tn")
    m, xd = load_module(st, H, tn, "bf16"), x.cuda()
    with torch.no_grad():
        want = m(xd, 2, 3)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g), torch.no_grad():
        out = m(xd, 2, 3)
    out.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)


def test_refusals():
    B, N1, D = 2, 7, 64
    t = {k: v.cuda() for k, v in U.glue_inputs(1, 7, 64).items()}
    x1 = torch.full((1, 7, 64), float("nan"), device="cuda")
    with pytest.raises(VitmiError, match="bf16 or fp32"):
        ops.ca_merge_fwd(t["x"], t["a"].half(), t["l"].half(), t["g1"], x1, 1, 7, 64)
    with pytest.raises(VitmiError, match="N1 >= 2"):
        ops.ca_merge_fwd(t["x"][:, :1].contiguous(), t["a"], t["l"][:, :1].contiguous(), t["g1"], x1[:, :1].contiguous(), 1, 1, 64)
    with pytest.raises(VitmiError, match="multiple of 8"):
        ops.ca_out_bwd(torch.zeros((1, 7, 12), device="cuda"), torch.zeros(12, device="cuda"), torch.zeros((1, 7, 12), device="cuda"),
                       torch.zeros((1, 12), device="cuda"), 1, 7, 12)
    with pytest.raises(VitmiError, match="l must be"):
        ops.ca_merge_fwd(t["x"], t["a"], t["l"].bfloat16(), t["g1"], x1, 1, 7, 64)
    with pytest.raises(VitmiError, match="xc must be"):
        ops.ca_out_fwd(t["xc"].bfloat16(), t["x"], t["m"], t["g2"], x1, 1, 7, 64)
    torch.cuda.synchronize()
    assert torch.isnan(x1).all()
    assert not ops.ca_glue_supported(torch.float16, 1, 7, 64) and ops.ca_glue_supported(torch.bfloat16, 64, 197, 192)
    m = ClassAttentionBlock(D, 2, eta=1.0).cuda()
    with pytest.raises(VitmiError, match="at most 1025"):
        m(torch.zeros((1, 1026, D), device="cuda"), 25, 41)
    with pytest.raises(VitmiError, match="at least one patch"):
        m(torch.zeros((B, 1, D), device="cuda"), 0, 0)
    with pytest.raises(VitmiError, match="input must be"):
        m(torch.zeros((B, N1, 32), device="cuda"), 2, 3)
