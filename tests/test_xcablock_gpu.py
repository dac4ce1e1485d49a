"""The XCABlock's junction kernel (csrc/layernorm.hip: ops.ls_residual_ln_fwd, y = x + gamma * b and l = LayerNorm(y) in one
pass) and the XCABlock module on the GPU.

Metric: max |got - want| / max |want| (xcab_util.rel).  Every check prints its error beside its bound (-s).
References are float64 (xcab_util), pinned to the reference's class by tests/golden/xcab.npz (test_xcablock_cpu.py); the
fixture case runs the module on the fixture's inputs and state.

Bounds, measured on the CPU by test_xcablock_cpu.py and frozen here, rounded up (rules of test_xcit_ca_gpu.py /
test_lpi_gpu.py / test_convembed_gpu.py), per case and per tensor:
  * fp32: 4x the error of the float32 closed form (xcab_util.closed_block / kernel_reference in float32) against float64 on
    the same inputs (F32_*), and never below FLOOR = 2^-23: one fp32 store alone is off by up to 2^-24 of its own value, so a
    float32 figure that happens to be 0 on a fixture's grid values (sums of few exactly representable products) does not
    ask the GPU's summation order for exactness.
  * bf16: 2x the error of the float64 emulation that carries exactly the declared roundings (xcab_util's docstring lists
    them) plus the fp32 bound of the same tensor (EMU_*): the emulation runs in float64 and carries nothing of the fp32
    accumulation the bf16 path also has.
  * the junction kernel alone: b is bf16-representable, so both dtypes see the same operands; only l is rounded on store.
    Its figures are the worst over the M of xcab_util.KERNEL_M at each D.
  * exact: gamma = 0 gives y bit-equal to x; in place (y is x) gives the bits of out of place; ops.layernorm_fwd on the
    junction's own y gives the junction's l, mean and rstd (the two kernels are neighbours in layernorm.hip and sum a row
    in the same order: the junction stays that LayerNorm); a zero dout gives exactly zero
    gradients and a zero dx; two rounds on one module give the same bits; num_batches_tracked.
  * the optimizer step: |p' - (p - lr g_ref)| <= lr * (the gradient's bound) * max |g_ref| + 2^-23 max |p| (the fp32 store of p').
Measured on an MI355X (one run; DESIGN.md 4.9 has the list).
"""
import os

import pytest
import torch

import fixture_codec as FC
import xcab_util as U
from vit_torch_amd import FusedSGD, VitmiError, XCABlock, ops

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
MODES = pytest.mark.parametrize("mode", ["fp32", "bf16"])
FLOOR = 2.0 ** -23

F32_MODULE = {
    "fixture": {
        "out": 1.74e-07, "dx": 1.95e-07, "grad/gamma1": 4.43e-07, "grad/gamma2": 3.31e-07, "grad/gamma3": 1.49e-07,
        "grad/norm1.weight": 2.09e-07, "grad/norm1.bias": 1.65e-07, "grad/attn.temperature": 1.11e-07,
        "grad/attn.qkv.weight": 3.31e-07, "grad/attn.qkv.bias": 1.56e-07, "grad/attn.proj.weight": 5.19e-07,
        "grad/attn.proj.bias": 8.80e-08, "grad/norm2.weight": 3.65e-07, "grad/norm2.bias": 2.31e-07,
        "grad/mlp.fc1.weight": 2.31e-07, "grad/mlp.fc1.bias": 2.27e-07, "grad/mlp.fc2.weight": 1.88e-07,
        "grad/mlp.fc2.bias": 0.00e+00, "grad/norm3.weight": 9.70e-07, "grad/norm3.bias": 3.85e-07,
        "grad/local_mp.conv1.weight": 2.83e-07, "grad/local_mp.conv1.bias": 1.24e-06, "grad/local_mp.bn.weight": 2.95e-07,
        "grad/local_mp.bn.bias": 9.57e-08, "grad/local_mp.conv2.weight": 2.79e-07, "grad/local_mp.conv2.bias": 2.15e-07,
        "buf/local_mp.bn.running_mean": 3.66e-08, "buf/local_mp.bn.running_var": 7.74e-08, "out_eval": 1.39e-07},
    "B2-1x2-D64-h2": {
        "out": 1.53e-07, "dx": 5.33e-06, "grad/gamma1": 7.83e-07, "grad/gamma2": 3.59e-07, "grad/gamma3": 4.24e-07,
        "grad/norm1.weight": 6.30e-06, "grad/norm1.bias": 1.93e-05, "grad/attn.temperature": 8.04e-06,
        "grad/attn.qkv.weight": 6.46e-06, "grad/attn.qkv.bias": 3.00e-05, "grad/attn.proj.weight": 4.52e-06,
        "grad/attn.proj.bias": 3.95e-07, "grad/norm2.weight": 2.15e-07, "grad/norm2.bias": 2.55e-07,
        "grad/mlp.fc1.weight": 3.58e-07, "grad/mlp.fc1.bias": 1.83e-07, "grad/mlp.fc2.weight": 2.95e-07,
        "grad/mlp.fc2.bias": 6.55e-08, "grad/norm3.weight": 1.17e-06, "grad/norm3.bias": 2.71e-06,
        "grad/local_mp.conv1.weight": 2.84e-07, "grad/local_mp.conv1.bias": 1.28e-05, "grad/local_mp.bn.weight": 5.45e-07,
        "grad/local_mp.bn.bias": 1.37e-07, "grad/local_mp.conv2.weight": 1.17e-06, "grad/local_mp.conv2.bias": 1.99e-07,
        "buf/local_mp.bn.running_mean": 4.06e-08, "buf/local_mp.bn.running_var": 7.74e-08, "out_eval": 1.67e-07},
    "B2-3x5-D96-h2": {
        "out": 2.80e-07, "dx": 1.62e-07, "grad/gamma1": 3.91e-07, "grad/gamma2": 2.48e-07, "grad/gamma3": 2.19e-07,
        "grad/norm1.weight": 3.24e-07, "grad/norm1.bias": 4.98e-07, "grad/attn.temperature": 5.82e-07,
        "grad/attn.qkv.weight": 2.36e-07, "grad/attn.qkv.bias": 3.74e-07, "grad/attn.proj.weight": 3.97e-07,
        "grad/attn.proj.bias": 1.07e-07, "grad/norm2.weight": 4.93e-07, "grad/norm2.bias": 3.08e-07,
        "grad/mlp.fc1.weight": 2.15e-07, "grad/mlp.fc1.bias": 2.10e-07, "grad/mlp.fc2.weight": 2.01e-07,
        "grad/mlp.fc2.bias": 1.25e-07, "grad/norm3.weight": 5.60e-07, "grad/norm3.bias": 4.04e-07,
        "grad/local_mp.conv1.weight": 3.99e-07, "grad/local_mp.conv1.bias": 8.55e-07, "grad/local_mp.bn.weight": 3.36e-07,
        "grad/local_mp.bn.bias": 1.18e-07, "grad/local_mp.conv2.weight": 1.98e-07, "grad/local_mp.conv2.bias": 5.89e-08,
        "buf/local_mp.bn.running_mean": 5.22e-08, "buf/local_mp.bn.running_var": 7.47e-08, "out_eval": 2.21e-07},
    "B3-7x9-D128-h2": {
        "out": 2.65e-07, "dx": 2.59e-07, "grad/gamma1": 2.50e-07, "grad/gamma2": 4.18e-07, "grad/gamma3": 1.88e-07,
        "grad/norm1.weight": 2.07e-07, "grad/norm1.bias": 8.27e-07, "grad/attn.temperature": 2.58e-07,
        "grad/attn.qkv.weight": 7.56e-07, "grad/attn.qkv.bias": 8.44e-07, "grad/attn.proj.weight": 5.78e-07,
        "grad/attn.proj.bias": 1.80e-07, "grad/norm2.weight": 3.69e-07, "grad/norm2.bias": 3.64e-07,
        "grad/mlp.fc1.weight": 5.17e-07, "grad/mlp.fc1.bias": 2.95e-07, "grad/mlp.fc2.weight": 4.07e-07,
        "grad/mlp.fc2.bias": 1.19e-07, "grad/norm3.weight": 1.83e-06, "grad/norm3.bias": 6.61e-07,
        "grad/local_mp.conv1.weight": 2.71e-07, "grad/local_mp.conv1.bias": 7.99e-07, "grad/local_mp.bn.weight": 2.14e-07,
        "grad/local_mp.bn.bias": 1.02e-07, "grad/local_mp.conv2.weight": 2.98e-07, "grad/local_mp.conv2.bias": 1.67e-07,
        "buf/local_mp.bn.running_mean": 8.71e-08, "buf/local_mp.bn.running_var": 8.79e-08, "out_eval": 3.11e-07},
    "B2-14x14-D192-h4": {
        "out": 2.15e-07, "dx": 3.56e-07, "grad/gamma1": 3.27e-07, "grad/gamma2": 4.10e-07, "grad/gamma3": 1.94e-07,
        "grad/norm1.weight": 2.40e-07, "grad/norm1.bias": 8.10e-07, "grad/attn.temperature": 8.74e-07,
        "grad/attn.qkv.weight": 5.47e-07, "grad/attn.qkv.bias": 7.00e-07, "grad/attn.proj.weight": 6.09e-07,
        "grad/attn.proj.bias": 2.51e-07, "grad/norm2.weight": 6.21e-07, "grad/norm2.bias": 4.12e-07,
        "grad/mlp.fc1.weight": 4.93e-07, "grad/mlp.fc1.bias": 3.22e-07, "grad/mlp.fc2.weight": 3.68e-07,
        "grad/mlp.fc2.bias": 1.09e-07, "grad/norm3.weight": 1.82e-06, "grad/norm3.bias": 2.64e-07,
        "grad/local_mp.conv1.weight": 3.69e-07, "grad/local_mp.conv1.bias": 4.42e-07, "grad/local_mp.bn.weight": 2.38e-07,
        "grad/local_mp.bn.bias": 1.30e-07, "grad/local_mp.conv2.weight": 3.80e-07, "grad/local_mp.conv2.bias": 1.04e-07,
        "buf/local_mp.bn.running_mean": 5.48e-08, "buf/local_mp.bn.running_var": 9.50e-08, "out_eval": 2.45e-07},
}
EMU_MODULE = {
    "fixture": {
        "out": 3.10e-03, "dx": 3.69e-03, "grad/gamma1": 4.10e-03, "grad/gamma2": 4.41e-03, "grad/gamma3": 2.38e-03,
        "grad/norm1.weight": 2.59e-03, "grad/norm1.bias": 4.69e-03, "grad/attn.temperature": 6.78e-03,
        "grad/attn.qkv.weight": 4.63e-03, "grad/attn.qkv.bias": 4.37e-03, "grad/attn.proj.weight": 6.90e-03,
        "grad/attn.proj.bias": 2.81e-03, "grad/norm2.weight": 4.47e-03, "grad/norm2.bias": 3.72e-03,
        "grad/mlp.fc1.weight": 3.82e-03, "grad/mlp.fc1.bias": 3.70e-03, "grad/mlp.fc2.weight": 2.39e-03,
        "grad/mlp.fc2.bias": 1.36e-03, "grad/norm3.weight": 8.39e-03, "grad/norm3.bias": 5.35e-03,
        "grad/local_mp.conv1.weight": 2.89e-03, "grad/local_mp.conv1.bias": 6.43e-03, "grad/local_mp.bn.weight": 2.47e-03,
        "grad/local_mp.bn.bias": 3.56e-03, "grad/local_mp.conv2.weight": 3.44e-03, "grad/local_mp.conv2.bias": 2.21e-03,
        "buf/local_mp.bn.running_mean": 1.45e-04, "buf/local_mp.bn.running_var": 1.54e-04, "out_eval": 1.72e-03},
    "B2-1x2-D64-h2": {
        "out": 1.37e-03, "dx": 2.68e-02, "grad/gamma1": 5.09e-03, "grad/gamma2": 4.40e-03, "grad/gamma3": 7.07e-03,
        "grad/norm1.weight": 4.01e-02, "grad/norm1.bias": 8.56e-02, "grad/attn.temperature": 3.74e-02,
        "grad/attn.qkv.weight": 4.28e-02, "grad/attn.qkv.bias": 1.24e-01, "grad/attn.proj.weight": 1.92e-02,
        "grad/attn.proj.bias": 3.11e-03, "grad/norm2.weight": 2.25e-03, "grad/norm2.bias": 3.99e-03,
        "grad/mlp.fc1.weight": 5.52e-03, "grad/mlp.fc1.bias": 3.55e-03, "grad/mlp.fc2.weight": 5.61e-03,
        "grad/mlp.fc2.bias": 1.48e-03, "grad/norm3.weight": 1.02e-02, "grad/norm3.bias": 1.51e-02,
        "grad/local_mp.conv1.weight": 1.34e-02, "grad/local_mp.conv1.bias": 8.10e-02, "grad/local_mp.bn.weight": 4.14e-03,
        "grad/local_mp.bn.bias": 4.60e-03, "grad/local_mp.conv2.weight": 9.81e-03, "grad/local_mp.conv2.bias": 4.53e-03,
        "buf/local_mp.bn.running_mean": 5.10e-04, "buf/local_mp.bn.running_var": 4.90e-04, "out_eval": 1.08e-03},
    "B2-3x5-D96-h2": {
        "out": 2.68e-03, "dx": 3.31e-03, "grad/gamma1": 3.08e-03, "grad/gamma2": 3.25e-03, "grad/gamma3": 4.75e-03,
        "grad/norm1.weight": 5.40e-03, "grad/norm1.bias": 7.78e-03, "grad/attn.temperature": 4.66e-03,
        "grad/attn.qkv.weight": 4.43e-03, "grad/attn.qkv.bias": 5.74e-03, "grad/attn.proj.weight": 5.06e-03,
        "grad/attn.proj.bias": 2.08e-03, "grad/norm2.weight": 7.63e-03, "grad/norm2.bias": 3.95e-03,
        "grad/mlp.fc1.weight": 3.55e-03, "grad/mlp.fc1.bias": 3.27e-03, "grad/mlp.fc2.weight": 2.85e-03,
        "grad/mlp.fc2.bias": 9.48e-04, "grad/norm3.weight": 5.74e-03, "grad/norm3.bias": 4.72e-03,
        "grad/local_mp.conv1.weight": 4.54e-03, "grad/local_mp.conv1.bias": 5.41e-03, "grad/local_mp.bn.weight": 6.60e-03,
        "grad/local_mp.bn.bias": 1.23e-03, "grad/local_mp.conv2.weight": 4.88e-03, "grad/local_mp.conv2.bias": 2.08e-03,
        "buf/local_mp.bn.running_mean": 1.55e-04, "buf/local_mp.bn.running_var": 8.77e-05, "out_eval": 2.03e-03},
    "B3-7x9-D128-h2": {
        "out": 3.96e-03, "dx": 3.91e-03, "grad/gamma1": 2.39e-03, "grad/gamma2": 4.29e-03, "grad/gamma3": 2.78e-03,
        "grad/norm1.weight": 2.64e-03, "grad/norm1.bias": 8.04e-03, "grad/attn.temperature": 2.49e-02,
        "grad/attn.qkv.weight": 5.49e-03, "grad/attn.qkv.bias": 1.13e-02, "grad/attn.proj.weight": 3.71e-03,
        "grad/attn.proj.bias": 2.81e-03, "grad/norm2.weight": 4.63e-03, "grad/norm2.bias": 3.63e-03,
        "grad/mlp.fc1.weight": 4.68e-03, "grad/mlp.fc1.bias": 3.78e-03, "grad/mlp.fc2.weight": 3.27e-03,
        "grad/mlp.fc2.bias": 1.93e-03, "grad/norm3.weight": 1.48e-02, "grad/norm3.bias": 5.69e-03,
        "grad/local_mp.conv1.weight": 2.85e-03, "grad/local_mp.conv1.bias": 3.81e-03, "grad/local_mp.bn.weight": 3.69e-03,
        "grad/local_mp.bn.bias": 1.41e-03, "grad/local_mp.conv2.weight": 3.24e-03, "grad/local_mp.conv2.bias": 2.02e-03,
        "buf/local_mp.bn.running_mean": 1.14e-04, "buf/local_mp.bn.running_var": 3.94e-05, "out_eval": 2.45e-03},
    "B2-14x14-D192-h4": {
        "out": 2.52e-03, "dx": 3.63e-03, "grad/gamma1": 4.22e-03, "grad/gamma2": 3.98e-03, "grad/gamma3": 2.30e-03,
        "grad/norm1.weight": 2.46e-03, "grad/norm1.bias": 1.10e-02, "grad/attn.temperature": 7.37e-03,
        "grad/attn.qkv.weight": 5.05e-03, "grad/attn.qkv.bias": 1.01e-02, "grad/attn.proj.weight": 7.21e-03,
        "grad/attn.proj.bias": 2.74e-03, "grad/norm2.weight": 7.86e-03, "grad/norm2.bias": 4.47e-03,
        "grad/mlp.fc1.weight": 4.23e-03, "grad/mlp.fc1.bias": 3.33e-03, "grad/mlp.fc2.weight": 2.72e-03,
        "grad/mlp.fc2.bias": 1.21e-03, "grad/norm3.weight": 3.60e-02, "grad/norm3.bias": 3.55e-03,
        "grad/local_mp.conv1.weight": 3.74e-03, "grad/local_mp.conv1.bias": 3.42e-03, "grad/local_mp.bn.weight": 2.13e-03,
        "grad/local_mp.bn.bias": 1.42e-03, "grad/local_mp.conv2.weight": 7.83e-03, "grad/local_mp.conv2.bias": 1.30e-03,
        "buf/local_mp.bn.running_mean": 9.96e-05, "buf/local_mp.bn.running_var": 4.41e-05, "out_eval": 2.70e-03},
}
F32_KERNEL = {
    8: {"y": 5.86e-08, "l": 1.34e-07, "mean": 8.11e-08, "rstd": 1.18e-07},
    64: {"y": 5.38e-08, "l": 1.90e-07, "mean": 1.01e-07, "rstd": 8.35e-08},
    72: {"y": 4.50e-08, "l": 1.42e-07, "mean": 9.18e-08, "rstd": 7.17e-08},
    136: {"y": 5.00e-08, "l": 1.58e-07, "mean": 1.23e-07, "rstd": 9.95e-08},
    192: {"y": 5.45e-08, "l": 1.20e-07, "mean": 1.21e-07, "rstd": 9.69e-08},
    384: {"y": 6.25e-08, "l": 1.37e-07, "mean": 8.92e-08, "rstd": 9.30e-08},
    392: {"y": 5.10e-08, "l": 1.91e-07, "mean": 9.46e-08, "rstd": 9.18e-08},
    512: {"y": 4.91e-08, "l": 1.53e-07, "mean": 1.57e-07, "rstd": 1.25e-07},
    768: {"y": 6.29e-08, "l": 2.06e-07, "mean": 1.46e-07, "rstd": 9.42e-08},
    1032: {"y": 5.27e-08, "l": 1.26e-07, "mean": 1.45e-07, "rstd": 1.17e-07},
    2048: {"y": 5.93e-08, "l": 1.77e-07, "mean": 1.18e-07, "rstd": 9.63e-08},
}
EMU_KERNEL = {
    8: {"y": 0.00e+00, "l": 3.08e-03, "mean": 0.00e+00, "rstd": 0.00e+00},
    64: {"y": 0.00e+00, "l": 3.28e-03, "mean": 0.00e+00, "rstd": 0.00e+00},
    72: {"y": 0.00e+00, "l": 2.30e-03, "mean": 0.00e+00, "rstd": 0.00e+00},
    136: {"y": 0.00e+00, "l": 3.11e-03, "mean": 0.00e+00, "rstd": 0.00e+00},
    192: {"y": 0.00e+00, "l": 3.73e-03, "mean": 0.00e+00, "rstd": 0.00e+00},
    384: {"y": 0.00e+00, "l": 3.23e-03, "mean": 0.00e+00, "rstd": 0.00e+00},
    392: {"y": 0.00e+00, "l": 2.60e-03, "mean": 0.00e+00, "rstd": 0.00e+00},
    512: {"y": 0.00e+00, "l": 2.77e-03, "mean": 0.00e+00, "rstd": 0.00e+00},
    768: {"y": 0.00e+00, "l": 2.65e-03, "mean": 0.00e+00, "rstd": 0.00e+00},
    1032: {"y": 0.00e+00, "l": 2.87e-03, "mean": 0.00e+00, "rstd": 0.00e+00},
    2048: {"y": 0.00e+00, "l": 2.57e-03, "mean": 0.00e+00, "rstd": 0.00e+00},
}
F32_KERNEL_MEAN100 = {
    384: {"y": 3.74e-08, "l": 4.53e-06, "mean": 1.31e-07, "rstd": 2.47e-07},
}
EMU_KERNEL_MEAN100 = {
    384: {"y": 0.00e+00, "l": 3.23e-03, "mean": 0.00e+00, "rstd": 0.00e+00},
}


def module_bound(mode, case):
    """"fp32" 4x the float32 figure (at least FLOOR); "bf16" 2x the float64 emulation's error plus that (docstring)"""
    return {k: max(4 * v, FLOOR) + (2 * EMU_MODULE[case][k] if mode == "bf16" else 0.0) for k, v in F32_MODULE[case].items()}


def kernel_bound(dtype, D, mean100=False):
    f32, emu = (F32_KERNEL_MEAN100, EMU_KERNEL_MEAN100) if mean100 else (F32_KERNEL, EMU_KERNEL)
    return {k: max(4 * v, FLOOR) + (2 * emu[D][k] if dtype == torch.bfloat16 else 0.0) for k, v in f32[D].items()}


def judge(name, e, b):
    print(f"\n  {name}: " + "  ".join(f"{k} {v:.2e} ({b[k]:.1e})" for k, v in e.items()), end="")
    bad = {k: (v, b[k]) for k, v in e.items() if not v <= b[k]}
    assert not bad, f"{name}: over the bound: {bad}"


# --------------------------------------------------------------------------------------- 1: the junction kernel ---
def guarded(M, D, dtype):
    """NaN rows [M, D] between a NaN guard row before and after: (whole buffer, the view); D = 1 for the per-row vectors,
    whose guard is four elements so that the view stays 16-byte aligned"""
    g = D if D > 1 else 4
    buf = torch.full((M * D + 2 * g,), float("nan"), dtype=dtype, device="cuda")
    v = buf[g:g + M * D]
    return buf, (v.view(M, D) if D > 1 else v)


def guards_untouched(buf, view):
    g = (buf.numel() - view.numel()) // 2
    return bool(torch.isnan(buf[:g]).all() and torch.isnan(buf[g + view.numel():]).all())


def run_kernel(t, dtype, in_place=False, gamma=None):
    """the kernel on xcab_util.kernel_inputs: {"y", "l", "mean", "rstd"} on the device, guards checked"""
    M, D = t["x"].shape
    f32 = torch.float32
    x, b = t["x"].cuda(), t["b"].cuda().to(dtype)
    bufs = {"y": guarded(M, D, f32), "l": guarded(M, D, dtype), "mean": guarded(M, 1, f32), "rstd": guarded(M, 1, f32)}
    o = {k: v[1] for k, v in bufs.items()}
    if in_place:
        o["y"].copy_(x)
    ops.ls_residual_ln_fwd(o["y"] if in_place else x, b, (t["gamma"] if gamma is None else gamma).cuda(), t["w"].cuda(),
                           t["bias"].cuda(), o["y"], o["l"], o["mean"], o["rstd"], U.EPS, M=M, D=D)
    torch.cuda.synchronize()
    for k, (buf, view) in bufs.items():
        assert guards_untouched(buf, view), f"{k}: a guard row was written (M {M}, D {D})"
        assert not torch.isnan(view).any(), f"{k}: not every element was written (M {M}, D {D})"
    if not in_place:
        assert torch.equal(x.cpu(), t["x"]), "x was modified"
    return o


@DTYPES
@pytest.mark.parametrize("D", U.KERNEL_D)
def test_kernel_against_float64(D, dtype):
    assert ops.ls_residual_ln_supported(dtype, max(U.KERNEL_M), D)
    for M in U.KERNEL_M:
        t = U.kernel_inputs(M, D)
        got, ref = run_kernel(t, dtype), U.kernel_reference(t)
        judge(f"M{M} D{D} {dtype}", {k: U.rel(got[k].float().cpu(), ref[k]) for k in U.KERNEL_KEYS}, kernel_bound(dtype, D))


@DTYPES
def test_kernel_rows_with_a_mean_of_100(dtype):
    """unit spread on a mean of 100: a one-pass variance (E[y^2] - E[y]^2 in fp32) would lose rstd"""
    M, D = 67, 384
    t = U.kernel_inputs(M, D, 100.0)
    got, ref = run_kernel(t, dtype), U.kernel_reference(t)
    judge(f"mean100 {dtype}", {k: U.rel(got[k].float().cpu(), ref[k]) for k in U.KERNEL_KEYS}, kernel_bound(dtype, D, True))


@DTYPES
def test_kernel_gamma_zero_and_in_place(dtype):
    for M, D in ((5, 72), (67, 392), (3, 2048)):
        t = U.kernel_inputs(M, D)
        zero = run_kernel(t, dtype, gamma=torch.zeros(D))
        assert torch.equal(zero["y"].cpu(), t["x"]), "gamma = 0: y is not x, bit for bit"
        out, inp = run_kernel(t, dtype), run_kernel(t, dtype, in_place=True)
        for k in U.KERNEL_KEYS:
            assert torch.equal(out[k], inp[k]), f"{k}: in place differs from out of place (M {M}, D {D})"


@DTYPES
@pytest.mark.parametrize("D", U.KERNEL_D)
def test_kernel_is_the_layernorm_of_its_own_y(D, dtype):
    """ops.layernorm_fwd (ln_fwd8_kernel: y and every vector are 16-byte aligned) on the junction's y, with the same weight,
    bias and eps, gives the junction's l, mean and rstd bit for bit"""
    for M in U.KERNEL_M:
        t = U.kernel_inputs(M, D)
        got = run_kernel(t, dtype)
        l = torch.empty((M, D), dtype=dtype, device="cuda")
        mean, rstd = torch.empty(M, device="cuda"), torch.empty(M, device="cuda")
        ops.layernorm_fwd(got["y"], t["w"].cuda(), t["bias"].cuda(), l, mean, rstd, U.EPS, M=M, D=D)
        for k, v in (("l", l), ("mean", mean), ("rstd", rstd)):
            assert torch.equal(got[k], v), f"{k}: the junction and layernorm_fwd differ (M {M}, D {D})"


def test_kernel_refusals():
    M, D = 3, 64
    t = {k: v.cuda() for k, v in U.kernel_inputs(M, D).items()}
    y, l = torch.full((M, D), float("nan"), device="cuda"), torch.full((M, D), float("nan"), device="cuda")
    mean, rstd = torch.empty(M, device="cuda"), torch.empty(M, device="cuda")
    args = lambda **k: [k.get(n, v) for n, v in (("x", t["x"]), ("b", t["b"]), ("gamma", t["gamma"]), ("w", t["w"]),  # noqa: E731
                                                 ("bias", t["bias"]), ("y", y), ("l", l), ("mean", mean), ("rstd", rstd))]
    with pytest.raises(VitmiError, match="bf16 or fp32"):
        ops.ls_residual_ln_fwd(*args(b=t["b"].half(), l=l.half()), U.EPS)
    with pytest.raises(VitmiError, match="l must be"):
        ops.ls_residual_ln_fwd(*args(l=l.bfloat16()), U.EPS)
    with pytest.raises(VitmiError, match="gamma must be"):
        ops.ls_residual_ln_fwd(*args(gamma=t["gamma"][:32]), U.EPS)
    with pytest.raises(VitmiError, match="mean must be"):
        ops.ls_residual_ln_fwd(*args(mean=torch.empty(M + 1, device="cuda")), U.EPS)
    z = lambda *s: torch.zeros(s, device="cuda")      # noqa: E731
    with pytest.raises(VitmiError, match="multiple of 8"):
        ops.ls_residual_ln_fwd(z(M, 60), z(M, 60), z(60), z(60), z(60), z(M, 60), z(M, 60), mean, rstd, U.EPS)
    with pytest.raises(VitmiError, match="multiple of 8"):
        ops.ls_residual_ln_fwd(z(1, 2056), z(1, 2056), z(2056), z(2056), z(2056), z(1, 2056), z(1, 2056), z(1), z(1), U.EPS)
    with pytest.raises(VitmiError, match="no CPU fallback"):
        ops.ls_residual_ln_fwd(*args(x=t["x"].cpu()), U.EPS)
    torch.cuda.synchronize()
    assert torch.isnan(y).all() and torch.isnan(l).all()
    assert not ops.ls_residual_ln_supported(torch.float16, M, D) and ops.ls_residual_ln_supported(torch.bfloat16, 50176, 384)


# -------------------------------------------------------------------------------------------------- 2: the module ---
@pytest.fixture(scope="module")
def fx():
    return FC.load(os.path.join(HERE, "golden", "xcab.npz"))


def load_module(st, heads, mode):
    D, Dh = st["attn.proj.weight"].shape[0], st["mlp.fc1.weight"].shape[0]
    m = XCABlock(D, heads, mlp_ratio=Dh / D, qkv_bias=True, eta=0.5, norm_layer=lambda d: torch.nn.LayerNorm(d, eps=U.EPS),
                 compute_dtype=mode)
    m.load_state_dict(st)
    return m.cuda()


def buffers(m):
    return {"buf/" + k: v.detach().cpu().clone() for k, v in m.state_dict().items() if k in U.BUF_KEYS}


def run_module(m, x, dy, Hg, Wg, requires_grad=True, eval_too=True):
    """one train-mode forward / backward, then an eval-mode forward on the buffers it left: xcab_util.KEYS"""
    m.train()
    xd = x.cuda().requires_grad_(requires_grad)
    out = m(xd, Hg, Wg)
    out.backward(dy.cuda())
    torch.cuda.synchronize()
    assert out.dtype == torch.float32 and tuple(out.shape) == tuple(x.shape)
    got = {"out": out.detach().cpu(), **{"grad/" + n: p.grad.cpu().clone() for n, p in m.named_parameters()}, **buffers(m)}
    if requires_grad:
        assert xd.grad.dtype == torch.float32
        got["dx"] = xd.grad.cpu()
    if eval_too:
        m.eval()
        with torch.no_grad():
            got["out_eval"] = m(x.cuda(), Hg, Wg).cpu()
        after = buffers(m)
        assert all(torch.equal(after[k], got[k]) for k in after), "an eval forward changed the buffers"
        m.train()
    return got


@MODES
def test_module_against_fixture(fx, mode):
    x, dy, st, heads, Hg, Wg, _ = U.fixture_case(fx)
    m = load_module(st, heads, mode)
    got = run_module(m, x, dy, Hg, Wg)
    ref = U.with_eval(U.torch_block, x, dy, st, heads, Hg, Wg)
    judge(f"fixture {mode}", U.errors(got, ref), module_bound(mode, "fixture"))
    nbt = got["buf/" + U.BUF_KEYS[2]]
    assert nbt.dtype == torch.int64 and int(nbt) == 8
    first = {n: p.grad.clone() for n, p in m.named_parameters()}
    m(x.cuda(), Hg, Wg).backward(dy.cuda())                        # a second backward accumulates into .grad
    torch.cuda.synchronize()
    for n, p in m.named_parameters():
        assert torch.allclose(p.grad, 2 * first[n], rtol=1e-5, atol=1e-6), f"{n}: .grad did not accumulate"


@MODES
@pytest.mark.parametrize("case", U.CASE_NAMES)
def test_module_against_float64(case, mode):
    x, dy, st, heads, Hg, Wg = U.module_case(case)
    got = run_module(load_module(st, heads, mode), x, dy, Hg, Wg)
    judge(f"{case} {mode}", U.errors(got, U.module_reference(case)), module_bound(mode, case))


@MODES
def test_module_exactness(fx, mode):
    x, dy, st, heads, Hg, Wg, _ = U.fixture_case(fx)
    m = load_module(st, heads, mode)
    first = run_module(m, x, dy, Hg, Wg, eval_too=False)
    m.zero_grad()
    second = run_module(m, x, dy, Hg, Wg, eval_too=False)           # batch statistics: the moved buffers change nothing
    for k in ("out", "dx") + tuple("grad/" + n for n in U.PARAM_KEYS):
        assert torch.equal(first[k], second[k]), f"{k}: the second round differs from the first"
    m.zero_grad()
    no_dx = run_module(m, x, dy, Hg, Wg, requires_grad=False, eval_too=False)
    for n in U.PARAM_KEYS:
        assert torch.equal(no_dx["grad/" + n], first["grad/" + n]), f"{n}: differs without dx"
    m.zero_grad()
    zero = run_module(m, x, torch.zeros_like(dy), Hg, Wg, eval_too=False)
    assert not zero["dx"].any()
    for n in U.PARAM_KEYS:
        assert not zero["grad/" + n].any(), f"{n}: a zero dout gave a non-zero gradient"


@MODES
def test_module_fused_sgd_step(fx, mode):
    x, dy, st, heads, Hg, Wg, _ = U.fixture_case(fx)
    m = load_module(st, heads, mode)
    lr, pack = 0.1, m.pack
    opt = FusedSGD(pack.params, lr=lr, momentum=0.9)
    run_module(m, x, dy, Hg, Wg, eval_too=False)
    opt.step()
    torch.cuda.synchronize()
    ref, bound = U.with_eval(U.torch_block, x, dy, st, heads, Hg, Wg), module_bound(mode, "fixture")
    for n, p in m.named_parameters():
        g = ref["grad/" + n]
        want = st[n].double() - lr * g
        err = (p.detach().cpu().double() - want).abs().max().item()
        tol = lr * bound["grad/" + n] * g.abs().max().item() + FLOOR * st[n].abs().max().item()
        print(f"\n  sgd {mode} {n}: {err:.2e} ({tol:.1e})", end="")
        assert err <= tol, f"{n}: {err:.3e} > {tol:.3e}"
        assert not torch.equal(p.detach().cpu(), st[n]), f"{n} did not move"


def test_module_refusals_on_the_device():
    m = XCABlock(64, 2, eta=1.0).cuda()
    with pytest.raises(VitmiError, match="input must be"):
        m(torch.zeros((2, 15, 32), device="cuda"), 3, 5)
    with pytest.raises(VitmiError, match="are not an H x W"):
        m(torch.zeros((2, 15, 64), device="cuda"), 4, 4)
    with pytest.raises(VitmiError, match="without a saved forward"):
        m.engine()._backward(torch.zeros((2, 15, 64), device="cuda"), True)
