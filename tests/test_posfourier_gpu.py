"""The positional-encoding kernels (csrc/xcit_glue.hip: ops.posfourier_features / ops.add_rows_bcast) and the
PositionalEncodingFourier module on the GPU.

Metric: max |got - want| / max |want| (posfourier_util.rel).  Every check prints its error beside its bound (-s).
References are float64 (posfourier_util), pinned to the reference's class by tests/golden/pos_fourier.npz
(test_posfourier_cpu.py); the module is run on the fixture's inputs and state.

Bounds, measured on the CPU by test_posfourier_cpu.py and frozen here (rules of test_convembed_gpu.py / test_lpi_gpu.py):
  * the feature table: fp32 4x F32_TABLE, the worst difference between the table in numpy float32 (every step rounded, the
    reference's order) and float64 over the tested grids: device sinf / cosf / powf may differ from the host's by a few ulp at
    arguments up to 2 pi.  bf16: 2x EMU_TABLE (the float64 table rounded to bf16) plus 4x F32_TABLE.
  * add_rows_bcast: one fp32 add per element.  fp32: EXACT against the float32 sum (IEEE addition).  bf16: the float32 sum
    rounded to bf16, exact as well.
  * the module: "fp32" 4x the float32 closed form's error against float64 on the same inputs (F32_MODULE); "bf16" 2x the
    error of the float64 emulation with the declared roundings (feature table, weight shadow, dpos as the weight gradient's
    operand) plus 4x the float32 figure.  The bias gradient of the fixtures is a sum of multiples of 1/32 that is exact in every
    dtype: its bound is 0.
  * exact: dx is dout, bit for bit; a zero dout gives exactly zero gradients.
Measured on an MI355X (one run; DESIGN.md 4.8 has the list).
"""
import os

import pytest
import torch

import fixture_codec as FC
import posfourier_util as U
from vit_torch_amd import FusedSGD, PositionalEncodingFourier, VitmiError, ops

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])

F32_TABLE, EMU_TABLE = 4.78e-07, 1.94e-03
F32_MODULE = {"g3x5": {"out": 8.60e-08, "pos": 2.02e-07, "grad/weight": 2.04e-07, "grad/bias": 0.0},
              "g4x4": {"out": 1.28e-07, "pos": 2.27e-07, "grad/weight": 1.55e-07, "grad/bias": 0.0}}
EMU_MODULE = {"g3x5": {"out": 4.81e-04, "pos": 1.13e-03, "grad/weight": 1.74e-03, "grad/bias": 0.0},
              "g4x4": {"out": 4.91e-04, "pos": 8.71e-04, "grad/weight": 1.39e-03, "grad/bias": 0.0}}


def module_bound(mode, name):
    """"fp32" 4x the float32 figure; "bf16" 2x the float64 emulation's error plus that (docstring)"""
    return {k: 4 * v + (2 * EMU_MODULE[name][k] if mode == "bf16" else 0.0) for k, v in F32_MODULE[name].items()}


def judge(name, e, b):
    print(f"\n  {name}: " + "  ".join(f"{k} {v:.2e} ({b[k]:.1e})" for k, v in e.items()), end="")
    bad = {k: (v, b[k]) for k, v in e.items() if not v <= b[k]}
    assert not bad, f"{name}: over the bound: {bad}"


G = 1024


def guarded(n, dtype):
    """n NaN elements between two NaN guard bands: (whole buffer, the view)"""
    buf = torch.full((n + 2 * G,), float("nan"), dtype=dtype, device="cuda")
    return buf, buf[G:G + n]


def guards_untouched(buf, n):
    return bool(torch.isnan(buf[:G]).all() and torch.isnan(buf[G + n:]).all())


# ------------------------------------------------------------------------------------------- 1: the feature table ---
@DTYPES
@pytest.mark.parametrize("H,W", U.TABLE_GRIDS, ids=[f"{h}x{w}" for h, w in U.TABLE_GRIDS])
def test_feature_table_against_float64(H, W, dtype):
    buf, out = guarded(H * W * 64, dtype)
    ops.posfourier_features(out.view(H * W, 64), H, W)
    torch.cuda.synchronize()
    assert guards_untouched(buf, out.numel())
    e = U.rel(out.view(H * W, 64).float().cpu(), U.features(H, W), denom=1.0)
    b = 4 * F32_TABLE + (2 * EMU_TABLE if dtype == torch.bfloat16 else 0.0)
    judge(f"table {H}x{W} {dtype}", {"table": e}, {"table": b})


# ---------------------------------------------------------------------------------------------- 2: add_rows_bcast ---
ADD_CASES = [(1, 5, 64), (3, 5, 64), (1, 3, 7), (3, 3, 7), (3, 1, 13), (1, 7, 10), (8, 196, 192)]


@DTYPES
@pytest.mark.parametrize("B,N,C", ADD_CASES, ids=[f"B{b}-N{n}-C{c}" for b, n, c in ADD_CASES])
def test_add_rows_bcast_is_the_rounded_float32_sum(B, N, C, dtype):
    x = U.gen((B, N, C), 10 * B + N + C).to(dtype)
    pos = U.gen((N, C), 77 + N + C)
    buf, out = guarded(B * N * C, dtype)
    ops.add_rows_bcast(x.cuda(), pos.cuda(), out.view(B, N, C), B, N, C)
    torch.cuda.synchronize()
    assert guards_untouched(buf, out.numel())
    assert torch.equal(out.view(B, N, C).cpu(), (x.float() + pos).to(dtype))


# -------------------------------------------------------------------------------------------------- 3: the module ---
@pytest.fixture(scope="module")
def fx():
    return FC.load(os.path.join(HERE, "golden", "pos_fourier.npz"))


def load_module(w, b, mode):
    m = PositionalEncodingFourier(dim=w.shape[0], compute_dtype=mode)
    m.load_state_dict({"token_projection.weight": w, "token_projection.bias": b})
    return m.cuda()


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(U.FIXTURE_GRIDS))
def test_module_against_fixture(fx, name, mode):
    x, dy, w, b, (H, W), _ = U.fixture_case(fx, name)
    ref = U.torch_posenc(x, dy, w, b, H, W)
    m = load_module(w, b, mode)
    xd, dyd = x.cuda().requires_grad_(True), dy.cuda()
    out = m(xd, H, W)
    out.backward(dyd)
    torch.cuda.synchronize()
    assert out.dtype == torch.float32 and torch.equal(xd.grad, dyd)                  # dx == dout exactly
    got = {"out": out.detach().cpu(), "pos": m.table(H, W).cpu(), "grad/weight": m.token_projection.weight.grad.cpu(),
           "grad/bias": m.token_projection.bias.grad.cpu()}
    judge(f"module {name} {mode}", U.errors(got, ref), module_bound(mode, name))
    first = {n: p.grad.clone() for n, p in m.named_parameters()}
    m(xd, H, W).backward(dyd)                                                          # a second backward accumulates
    torch.cuda.synchronize()
    for n, p in m.named_parameters():
        assert torch.allclose(p.grad, 2 * first[n], rtol=1e-5, atol=1e-6), f"{n}: .grad did not accumulate"


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_table_is_forward_on_zeros_and_zero_dout_gives_zero_gradients(fx, mode):
    x, dy, w, b, (H, W), _ = U.fixture_case(fx, "g3x5")
    m = load_module(w, b, mode)
    z = torch.zeros_like(x).cuda()
    with torch.no_grad():
        assert torch.equal(m(z, H, W)[0], m.table(H, W)) and torch.equal(m(z, H, W)[1], m.table(H, W))
    m(x.cuda(), H, W).backward(z)
    torch.cuda.synchronize()
    for n, p in m.named_parameters():
        assert p.grad is not None and not p.grad.any(), n


def test_module_fused_sgd_step(fx):
    x, dy, w, b, (H, W), _ = U.fixture_case(fx, "g4x4")
    m = load_module(w, b, "bf16")
    opt = FusedSGD(m.parameters(), lr=0.1, momentum=0.9)
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    m(x.cuda(), H, W).backward(dy.cuda())
    torch.cuda.synchronize()
    opt.step()
    torch.cuda.synchronize()
    for n, p in m.named_parameters():
        assert not torch.equal(p.detach(), before[n]), f"{n} did not move"
        assert torch.isfinite(p).all()
    old = U.torch_posenc(x, dy, w, b, H, W)["pos"].float()
    assert not torch.equal(m.table(H, W).cpu(), old)             # the projection is recomputed from the moved parameters


def test_module_graph_replay(fx):
    x, dy, w, b, (H, W), _ = U.fixture_case(fx, "g3x5")
    m, xd = load_module(w, b, "bf16"), x.cuda()
    with torch.no_grad():
        want = m(xd, H, W)                                       # also the warm-up: the feature table is cached here
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g), torch.no_grad():
        out = m(xd, H, W)
    out.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)


def test_refusals():
    out = torch.full((15, 64), float("nan"), device="cuda")
    with pytest.raises(VitmiError, match="hidden_dim"):
        ops.posfourier_features(torch.empty((15, 32), device="cuda"), 3, 5, hidden_dim=16)
    with pytest.raises(VitmiError, match="bf16 or fp32"):
        ops.posfourier_features(out.half(), 3, 5)
    with pytest.raises(VitmiError, match="contiguous"):
        ops.posfourier_features(out[:14], 3, 5)
    x = torch.zeros((2, 15, 64), device="cuda")
    with pytest.raises(VitmiError, match="pos"):
        ops.add_rows_bcast(x, torch.zeros((15, 64), dtype=torch.bfloat16, device="cuda"), torch.empty_like(x), 2, 15, 64)
    big = torch.zeros(x.numel() + 8, device="cuda")
    with pytest.raises(VitmiError, match="aligned"):
        ops.add_rows_bcast(big[1:1 + x.numel()].view_as(x), torch.zeros((15, 64), device="cuda"), torch.empty_like(x), 2, 15, 64)
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    assert not ops.posfourier_supported(torch.float32, 3, 5, 16) and ops.posfourier_supported(torch.bfloat16, 3, 5, 32)
    m = PositionalEncodingFourier(dim=64).cuda()
    with pytest.raises(VitmiError, match="grid"):
        m(x, 4, 4)
    with pytest.raises(VitmiError, match="input must be"):
        m(torch.zeros((2, 15, 32), device="cuda"), 3, 5)
