"""ops.xca_fwd / ops.xca_bwd (vitmi_xca_fwd / _bwd, csrc/xca.hip) and the XCA module against float64.

Metric: max |got - want| / max |want| (xca_util.rel), both sides on the same bf16-rounded operands; the reference is
xca_util.torch_xca, float64 autograd over the reference's lines.  Every check prints its error beside its bound (-s).

Bounds, measured on the CPU over each section's own inputs and frozen here (rules of test_vit_attention_gpu.py):
  * bf16 out, dq, dk, dv: 2x the largest error of xca_util.emulated_xca (float64 with exactly the declared roundings).
    The factor covers fp32 accumulation, the hardware exp and a rounding placed one operation earlier or later.
      section 1 maxima: out 4.63e-3 (hd 64, N 4), dq 9.19e-3 (hd 32, N 3), dk 8.35e-3 (hd 64, N 2), dv 4.55e-3 (hd 48, N 255)
      section 2 maxima per pair: out 4.77e-3, dq 4.64e-3, dk 4.74e-3, dv 5.90e-3
  * fp32 everything, and stat (Gh, r_q, r_k rows) and dtemp on both dtypes (no declared rounding): 4x the largest error
    of the closed form evaluated in torch float32 on the CPU.  The factor covers another summation order over up to 2304
    tokens and the division by the norms.
      section 1 maxima: out 4.52e-7, Gh 4.42e-6, r_q 2.41e-6, r_k 2.66e-6, dq 3.82e-6, dk 4.02e-6, dv 5.56e-7,
                        dtemp 2.39e-6 (all but out and dv at N 2304)
      section 2 maxima per pair: out 6.56e-7, Gh 5.96e-7, r_q 3.05e-7, r_k 3.33e-7, dq 9.32e-7, dk 8.85e-7, dv 5.07e-7,
                        dtemp 2.76e-7
  * the module, "fp32": 4x the error of the reference class in float32 (the fixture) against float64 on the fixture's
    inputs: y 1.88e-7, dx 4.33e-7, temperature 1.31e-7, qkv.weight 2.84e-7, qkv.bias 2.80e-7, proj.weight 2.53e-7,
    proj.bias 0 (a sum of 40 grid values: exact in any order).  "bf16": 2x the error of xca_util.module_ref with the
    stage-boundary roundings: y 1.22e-3, dx 3.71e-3, temperature 1.97e-3, qkv.weight 4.22e-3, qkv.bias 3.68e-3,
    proj.weight 3.25e-3, proj.bias 0.
Sequence lengths of section 1: the issue's list plus both neighbours of the kernels' steps (32-token reduction steps,
the 128-token streamed chunk, the 256-token resident limit of the backward); N = 1 runs the forward and dv only.
"""
import functools
import os

import pytest
import torch

import fixture_codec as FC
import xca_util as U
from vit_torch_amd import XCA, FusedSGD, VitmiError, ops

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

EMU_SWEEP = {"out": 4.63e-3, "dq": 9.19e-3, "dk": 8.35e-3, "dv": 4.55e-3}
F32_SWEEP = {"out": 4.52e-7, "gh": 4.42e-6, "rq": 2.41e-6, "rk": 2.66e-6, "dq": 3.82e-6, "dk": 4.02e-6, "dv": 5.56e-7,
             "dtemp": 2.39e-6}
EMU_PAIRS = {"out": 4.77e-3, "dq": 4.64e-3, "dk": 4.74e-3, "dv": 5.90e-3}
F32_PAIRS = {"out": 6.56e-7, "gh": 5.96e-7, "rq": 3.05e-7, "rk": 3.33e-7, "dq": 9.32e-7, "dk": 8.85e-7, "dv": 5.07e-7,
             "dtemp": 2.76e-7}
F32_MODULE = {"y": 1.88e-7, "dx": 4.33e-7, "grad/temperature": 1.31e-7, "grad/qkv.weight": 2.84e-7,
              "grad/qkv.bias": 2.80e-7, "grad/proj.weight": 2.53e-7, "grad/proj.bias": 0.0}
EMU_MODULE = {"y": 1.22e-3, "dx": 3.71e-3, "grad/temperature": 1.97e-3, "grad/qkv.weight": 4.22e-3,
              "grad/qkv.bias": 3.68e-3, "grad/proj.weight": 3.25e-3, "grad/proj.bias": 0.0}


def bounds(dtype, emu, f32):
    b = {k: 4 * v for k, v in f32.items()}
    if dtype == torch.bfloat16:
        b.update({k: 2 * v for k, v in emu.items()})
    return b


def run(qkv, dO, temp, B, N, H, hd, dtype, backward=True):
    q = qkv.to(dtype).cuda().reshape(B * N, 3 * H * hd).contiguous()
    t = torch.tensor(temp, dtype=torch.float32, device="cuda")
    out = torch.full((B, N, H * hd), float("nan"), dtype=dtype, device="cuda")
    stat = torch.full((B, H, hd + 2, hd), float("nan"), dtype=torch.float32, device="cuda")
    dqkv = torch.full((B * N, 3 * H * hd), float("nan"), dtype=dtype, device="cuda")
    dtemp = torch.full((H,), float("nan"), dtype=torch.float32, device="cuda")
    ops.xca_fwd(q, t, out, stat, B, N, H, hd)
    if backward:
        ops.xca_bwd(q, dO.to(dtype).cuda().contiguous(), t, stat, dqkv, dtemp, B, N, H, hd)
    torch.cuda.synchronize()
    return U.XcaRef(out.cpu(), stat.cpu(), dqkv.cpu().reshape(B, N, 3, H, hd), dtemp.cpu())


def judge(name, e, b):
    print(f"\n  {name}: " + "  ".join(f"{k} {v:.2e} ({b[k]:.1e})" for k, v in e.items()), end="")
    bad = {k: (v, b[k]) for k, v in e.items() if not v <= b[k]}
    assert not bad, f"{name}: over the bound: {bad}"


@functools.lru_cache(maxsize=None)
def sweep_reference(hd, N):
    B, N, H, hd, seed, temp = next(c for c in U.sweep_cases() if c[3] == hd and c[1] == N)
    qkv, dO = U.normal_inputs(B, N, H, hd, seed)
    return (B, N, H, hd, temp), qkv, dO, U.torch_xca(qkv, dO, torch.tensor(temp), B, N, H, hd)


SWEEP_IDS = [(c[3], c[1]) for c in U.sweep_cases()]


# ------------------------------------------------------------------------------------------------- 1: the sweep ---
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("hd,N", SWEEP_IDS, ids=[f"hd{h}N{n}" for h, n in SWEEP_IDS])
def test_sweep_against_float64(hd, N, dtype):
    (B, N, H, hd, temp), qkv, dO, want = sweep_reference(hd, N)
    got = run(qkv, dO, temp, B, N, H, hd, dtype)
    assert torch.isfinite(got.out).all() and torch.isfinite(got.stat).all() and torch.isfinite(got.dqkv).all()
    e = U.xca_errors(got, want, grads=N > 1)
    if N == 1:                         # forward and dv only: dq, dk cancel to zero through 1 / r, one-token norms
        e["dv"] = U.rel(got.dqkv[:, :, 2], want.dqkv[:, :, 2])
    judge(f"{dtype} hd{hd} N{N}", e, bounds(dtype, EMU_SWEEP, F32_SWEEP))


# ------------------------------------------------------------------------------------ 2: more pairs than CUs ---
def per_pair_errors(got, want, B, N, H, hd):
    def tok(g, w):
        g, w = g.double(), w.double()
        return ((g - w).abs().amax((1, 3)) / w.abs().amax((1, 3))).max().item()

    def mat(g, w, dims):
        g, w = g.double(), w.double()
        return ((g - w).abs().amax(dims) / w.abs().amax(dims)).max().item()
    e = {"out": tok(got.out.reshape(B, N, H, hd), want.out.reshape(B, N, H, hd))}
    e["gh"] = mat(got.stat[..., :hd, :], want.stat[..., :hd, :], (2, 3))
    e["rq"] = mat(got.stat[..., hd, :], want.stat[..., hd, :], (2,))
    e["rk"] = mat(got.stat[..., hd + 1, :], want.stat[..., hd + 1, :], (2,))
    for i, nm in enumerate("qkv"):
        e["d" + nm] = tok(got.dqkv[:, :, i], want.dqkv[:, :, i])
    e["dtemp"] = U.rel(got.dtemp, want.dtemp)
    return e


@functools.lru_cache(maxsize=None)
def pairs_reference():
    B, N, H, hd = U.PAIRS_CASE
    qkv, dO = U.normal_inputs(B, N, H, hd, 1000 * hd + N)
    return qkv, dO, U.torch_xca(qkv, dO, torch.tensor(U.PAIRS_TEMPERATURE), B, N, H, hd)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_more_pairs_than_cus(dtype):
    B, N, H, hd = U.PAIRS_CASE
    qkv, dO, want = pairs_reference()
    got = run(qkv, dO, U.PAIRS_TEMPERATURE, B, N, H, hd, dtype)
    judge(f"{dtype} 320 pairs", per_pair_errors(got, want, B, N, H, hd), bounds(dtype, EMU_PAIRS, F32_PAIRS))


# ----------------------------------------------------------------------------------- 3: a degenerate channel ---
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_degenerate_channel_forward(dtype):
    B, N, H, hd = 2, 65, 3, 48
    qkv, dO = U.normal_inputs(B, N, H, hd, 77)
    qkv.view(B, N, 3, H, hd)[1, :, 0, 2, 5] = 0.0          # q channel 5 of pair (1, 2)
    temp = U.SWEEP_TEMPERATURE
    want = U.torch_xca(qkv, dO, torch.tensor(temp), B, N, H, hd)
    got = run(qkv, dO, temp, B, N, H, hd, dtype, backward=False)
    assert torch.isfinite(got.out).all() and torch.isfinite(got.stat).all()
    assert got.stat[1, 2, 5].abs().max() == 0 and got.stat[1, 2, hd, 5] == 1e-12     # Gh row 0, r_q clamped
    judge(f"{dtype} zero channel", U.xca_errors(got, want, grads=False), bounds(dtype, EMU_SWEEP, F32_SWEEP))


# ------------------------------------------------------------------------------------------ 4: no stray stores ---
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("N", [1, 65, 197])
def test_no_stray_stores(N, dtype):
    B, H, hd, G = 2, 3, 48, 1024
    qkv, dO = U.normal_inputs(B, N, H, hd, 5 + N)
    q, d = qkv.to(dtype).cuda().reshape(B * N, 3 * H * hd), dO.to(dtype).cuda()
    t = torch.tensor(U.SWEEP_TEMPERATURE, device="cuda")

    def carve(n, dt):
        buf = torch.full((n + 2 * G,), -777.0, dtype=dt, device="cuda")
        return buf, buf[G:G + n]
    bo, out = carve(B * N * H * hd, dtype)
    bs, stat = carve(B * H * (hd + 2) * hd, torch.float32)
    bd, dqkv = carve(B * N * 3 * H * hd, dtype)
    bt, part = carve(B * H, torch.float32)
    lib = ops.load()
    ops.xca_fwd(q, t, out, stat, B, N, H, hd)
    ops.check(lib.vitmi_xca_bwd(q.data_ptr(), d.data_ptr(), t.data_ptr(), stat.data_ptr(), dqkv.data_ptr(), part.data_ptr(),
                                ops.dtype_code(q), B, N, H, hd, None, 0, torch.cuda.current_stream().cuda_stream), "vitmi_xca_bwd")
    torch.cuda.synchronize()
    for name, buf, inner in (("out", bo, out), ("stat", bs, stat), ("dqkv", bd, dqkv), ("dtemp_part", bt, part)):
        assert (buf[:G] == -777.0).all() and (buf[G + inner.numel():] == -777.0).all(), f"{name}: a guard was written"
        assert (inner != -777.0).all(), f"{name}: an element was not written"


# -------------------------------------------------------------------------------------------- 5: determinism ---
def raw_run(q, d, t, B, N, H, hd):
    out = torch.empty((B, N, H * hd), dtype=q.dtype, device="cuda")
    stat = torch.empty((B, H, hd + 2, hd), dtype=torch.float32, device="cuda")
    dqkv = torch.empty_like(q)
    dtemp = torch.empty((H,), dtype=torch.float32, device="cuda")
    ops.xca_fwd(q, t, out, stat, B, N, H, hd)
    ops.xca_bwd(q, d, t, stat, dqkv, dtemp, B, N, H, hd)
    return out, stat, dqkv, dtemp


@pytest.mark.parametrize("B,N,H,hd", [(2, 196, 3, 48), (1, 784, 3, 64)])
def test_bitwise_repeatable(B, N, H, hd):
    qkv, dO = U.normal_inputs(B, N, H, hd, 9)
    q, d = qkv.bfloat16().cuda().reshape(B * N, 3 * H * hd), dO.bfloat16().cuda()
    t = torch.tensor(U.SWEEP_TEMPERATURE, device="cuda")
    a, b = raw_run(q, d, t, B, N, H, hd), raw_run(q, d, t, B, N, H, hd)
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ----------------------------------------------------------------------------------------------- 6: refusals ---
def test_refusals():
    B, N, H = 1, 10, 2
    t = torch.ones(H, device="cuda")

    def bufs(hd, dtype, n=N):
        return (torch.zeros((B * n, 3 * H * hd), dtype=dtype, device="cuda"),
                torch.full((B, n, H * hd), float("nan"), dtype=dtype, device="cuda"),
                torch.full((B, H, hd + 2, hd), float("nan"), dtype=torch.float32, device="cuda"))
    q, out, stat = bufs(40, torch.bfloat16)
    with pytest.raises(VitmiError, match="head dim"):
        ops.xca_fwd(q, t, out, stat, B, N, H, 40)
    with pytest.raises(VitmiError, match="head dim"):
        ops.xca_bwd(q, out, t, stat, torch.empty_like(q), torch.empty(H, device="cuda"), B, N, H, 40)
    assert torch.isnan(out).all() and torch.isnan(stat).all()
    q, out, stat = bufs(48, torch.float16)
    with pytest.raises(VitmiError, match="bf16 or fp32"):
        ops.xca_fwd(q, t, out, stat, B, N, H, 48)
    assert torch.isnan(out).all() and torch.isnan(stat).all()
    q, out, stat = bufs(48, torch.bfloat16, n=0)
    with pytest.raises(VitmiError, match="at least 1"):
        ops.xca_fwd(q, t, torch.empty((B, 0, H * 48), dtype=torch.bfloat16, device="cuda"), stat, B, 0, H, 48)
    assert torch.isnan(stat).all()
    q, out, stat = bufs(48, torch.bfloat16)
    big = torch.zeros(q.numel() + 8, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(VitmiError, match="aligned"):
        ops.xca_fwd(big[1:1 + q.numel()].view_as(q), t, out, stat, B, N, H, 48)
    assert torch.isnan(out).all() and torch.isnan(stat).all()
    assert not ops.xca_supported(torch.bfloat16, H, N, 40) and ops.xca_supported(torch.float32, H, N, 48)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------- 7: graph replay ---
def test_graph_replay():
    B, N, H, hd = 2, 196, 3, 48
    qkv, dO = U.normal_inputs(B, N, H, hd, 21)
    q, d = qkv.bfloat16().cuda().reshape(B * N, 3 * H * hd), dO.bfloat16().cuda()
    t = torch.tensor(U.SWEEP_TEMPERATURE, device="cuda")
    eager = [x.clone() for x in raw_run(q, d, t, B, N, H, hd)]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        raw_run(q, d, t, B, N, H, hd)                     # warm the side stream's workspace outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = raw_run(q, d, t, B, N, H, hd)
    for _ in range(2):
        for x in outs:
            x.fill_(float("nan")) if x.is_floating_point() else None
        g.replay()
        torch.cuda.synchronize()
        for x, y in zip(outs, eager):
            assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------ 8: the module ---
@pytest.fixture(scope="module")
def fx():
    return FC.load(os.path.join(HERE, "golden", "xca.npz"))


def load_module(fx, mode):
    m = XCA(96, 3, qkv_bias=True, compute_dtype=mode)
    m.load_state_dict(FC.group(fx, "state"))
    return m.cuda()


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_module_against_fixture(fx, mode):
    m = load_module(fx, mode)
    x = fx["x"].cuda().requires_grad_(True)
    y = m(x)
    y.backward(fx["dy"].cuda())
    torch.cuda.synchronize()
    got = {"y": y, "dx": x.grad, **{"grad/" + n: p.grad for n, p in m.named_parameters()}}
    b = {k: 4 * v for k, v in F32_MODULE.items()} if mode == "fp32" else {k: 2 * v for k, v in EMU_MODULE.items()}
    judge(f"module {mode}", {k: U.rel_fixture(got[k], fx[k]) for k in b}, b)
    # a second backward accumulates into .grad (torch's contract)
    first = {n: p.grad.clone() for n, p in m.named_parameters()}
    m(x).backward(fx["dy"].cuda())
    torch.cuda.synchronize()
    for n, p in m.named_parameters():
        assert torch.allclose(p.grad, 2 * first[n], rtol=1e-6, atol=0), f"{n}: .grad did not accumulate"


def test_module_fused_sgd_step(fx):
    m = load_module(fx, "bf16")
    opt = FusedSGD(m.parameters(), lr=0.1, momentum=0.9)
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    m(fx["x"].cuda()).backward(fx["dy"].cuda())
    opt.step()
    torch.cuda.synchronize()
    for n, p in m.named_parameters():
        assert not torch.equal(p.detach(), before[n]), f"{n} did not move"
        assert torch.isfinite(p).all()
