"""ops.lpi_fwd / ops.lpi_bwd (vitmi_lpi_fwd / _bwd, csrc/lpi.hip) and the LPI module against float64.

Metric: max |got - want| / max |want| (lpi_util.rel), both sides on the same rounded operands; the reference is
lpi_util.torch_lpi, float64 autograd over the reference's lines.  In bf16 the op's stored u = bf16(gelu(conv1(x))) is an
operand of everything after it (the statistics are DEFINED over it), so the reference takes the op's own stored u
(u_stored=, straight-through) and the stored u itself is checked against the unrounded float64 one.  Every check prints its
error beside its bound (-s).

Bounds, measured on the CPU over each section's own inputs and frozen here (rules of test_vit_attention_gpu.py):
  * bf16 tensors (u, out, dx): 2x the largest error of lpi_util.emulated_lpi (float64 with exactly the declared roundings:
    u, out, dx on store and the staged dc).
      section 1 maxima (train and eval): out 3.54e-3, u 3.31e-3, dx 5.19e-3
      section 2 maxima per image: out 3.75e-3, u 3.30e-3, dx 5.61e-3        section 3: out 1.73e-3, u 2.54e-3, dx 2.78e-3
  * fp32 tensors, and on both dtypes stat (mean, rstd), the running buffers and every parameter gradient: 4x the largest
    error of the closed form evaluated in torch float32 on the CPU (two-pass variance).
      section 1 maxima: out 1.56e-6, u 2.17e-7, dx 6.76e-6, mean 1.52e-7, rstd 1.08e-6, conv1.weight 2.15e-6,
        conv1.bias 2.53e-5, bn.weight 1.17e-6, bn.bias 1.95e-7, conv2.weight 1.00e-6, conv2.bias 5.81e-8,
        running_mean 8.44e-8, running_var 1.19e-7
      section 2 (activations per image): out 3.48e-7, u 2.34e-7, dx 2.89e-7, mean 1.09e-7, rstd 1.03e-7, conv1.weight 3.31e-7,
        conv1.bias 3.39e-6, bn.weight 2.54e-7, bn.bias 1.36e-7, conv2.weight 2.21e-7, conv2.bias 7.16e-8,
        running_mean 1.05e-7, running_var 8.35e-8
      section 3: out 9.39e-7, u 6.61e-8, dx 1.72e-7, mean 2.68e-8, rstd 5.43e-8, conv1.weight 7.47e-8, conv1.bias 2.88e-5,
        bn.weight 2.06e-6, bn.bias 1.73e-7, conv2.weight 2.65e-6, conv2.bias 3.74e-8, running_mean 3.91e-8,
        running_var 8.51e-8   (the float32 closed form with the two-pass variance is itself within these: they are its errors)
  * the module, "fp32": 4x the error of the reference class in float32 (the fixture) against float64 on the fixture's
    inputs: y 1.29e-7, dx 1.94e-7, conv1.weight 1.95e-7, conv1.bias 8.42e-7, bn.weight 1.38e-7, bn.bias 0 and conv2.bias 0
    (sums of grid values: exact in any order), conv2.weight 2.02e-7, running_mean 8.91e-8, running_var 6.70e-8,
    y_eval 7.84e-8.  "bf16": 2x the error of lpi_util.module_ref with the declared roundings: y 2.57e-3, dx 3.87e-3,
    conv1.weight 8.78e-4, conv1.bias 4.22e-3, bn.weight 1.41e-3, bn.bias 0, conv2.weight 1.58e-3, conv2.bias 0,
    running_mean 1.10e-4, running_var 8.57e-5, y_eval 2.19e-3.
Grid sizes of section 1: the issue's list and C = 16 at 48 x 48; the kernels have one decomposition for every grid size, so
there are no path-change neighbours (lpi_util.sweep_cases).
"""
import functools
import os

import pytest
import torch

import fixture_codec as FC
import lpi_util as U
from vit_torch_amd import LPI, FusedSGD, VitmiError, ops

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

EMU_SWEEP = {"out": 3.54e-3, "u": 3.31e-3, "dx": 5.19e-3}
F32_SWEEP = {"out": 1.56e-6, "u": 2.17e-7, "dx": 6.76e-6, "mean": 1.52e-7, "rstd": 1.08e-6, "conv1.weight": 2.15e-6,
             "conv1.bias": 2.53e-5, "bn.weight": 1.17e-6, "bn.bias": 1.95e-7, "conv2.weight": 1.00e-6, "conv2.bias": 5.81e-8,
             "running_mean": 8.44e-8, "running_var": 1.19e-7}
EMU_WIDE = {"out": 3.75e-3, "u": 3.30e-3, "dx": 5.61e-3}
F32_WIDE = {"out": 3.48e-7, "u": 2.34e-7, "dx": 2.89e-7, "mean": 1.09e-7, "rstd": 1.03e-7, "conv1.weight": 3.31e-7,
            "conv1.bias": 3.39e-6, "bn.weight": 2.54e-7, "bn.bias": 1.36e-7, "conv2.weight": 2.21e-7, "conv2.bias": 7.16e-8,
            "running_mean": 1.05e-7, "running_var": 8.35e-8}
EMU_STRESS = {"out": 1.73e-3, "u": 2.54e-3, "dx": 2.78e-3}
F32_STRESS = {"out": 9.39e-7, "u": 6.61e-8, "dx": 1.72e-7, "mean": 2.68e-8, "rstd": 5.43e-8, "conv1.weight": 7.47e-8,
              "conv1.bias": 2.88e-5, "bn.weight": 2.06e-6, "bn.bias": 1.73e-7, "conv2.weight": 2.65e-6, "conv2.bias": 3.74e-8,
              "running_mean": 3.91e-8, "running_var": 8.51e-8}
F32_MODULE = {"y": 1.29e-7, "dx": 1.94e-7, "grad/conv1.weight": 1.95e-7, "grad/conv1.bias": 8.42e-7, "grad/bn.weight": 1.38e-7,
              "grad/bn.bias": 0.0, "grad/conv2.weight": 2.02e-7, "grad/conv2.bias": 0.0, "buf/bn.running_mean": 8.91e-8,
              "buf/bn.running_var": 6.70e-8, "y_eval": 7.84e-8}
EMU_MODULE = {"y": 2.57e-3, "dx": 3.87e-3, "grad/conv1.weight": 8.78e-4, "grad/conv1.bias": 4.22e-3, "grad/bn.weight": 1.41e-3,
              "grad/bn.bias": 0.0, "grad/conv2.weight": 1.58e-3, "grad/conv2.bias": 0.0, "buf/bn.running_mean": 1.10e-4,
              "buf/bn.running_var": 8.57e-5, "y_eval": 2.19e-3}


def bounds(dtype, emu, f32):
    b = {k: 4 * v for k, v in f32.items()}
    if dtype == torch.bfloat16:
        b.update({k: 2 * v for k, v in emu.items()})
    return b


def judge(name, e, b):
    print(f"\n  {name}: " + "  ".join(f"{k} {v:.2e} ({b[k]:.1e})" for k, v in e.items()), end="")
    bad = {k: (v, b[k]) for k, v in e.items() if not v <= b[k]}
    assert not bad, f"{name}: over the bound: {bad}"


def dev_params(p):
    """the nine state entries on the device, fp32 (int64 count), each its own 256-byte aligned allocation"""
    return {k: v.clone().to("cuda", torch.int64 if k.endswith("tracked") else torch.float32).reshape(-1) for k, v in p.items()}


def alloc(B, H, W, C, dtype, fill=float("nan")):
    t = {k: torch.full((B, H * W, C), fill, dtype=dtype, device="cuda") for k in ("u", "out", "dx")}
    t["stat"] = torch.full((2, C), fill, dtype=torch.float32, device="cuda")
    for k in U.GRAD_KEYS:
        t[k] = torch.full((C * 9 if k.endswith("weight") and "conv" in k else C,), fill, dtype=torch.float32, device="cuda")
    return t


def fwd(xd, P, t, B, H, W, C, training):
    ops.lpi_fwd(xd, P["conv1.weight"], P["conv1.bias"], P["bn.weight"], P["bn.bias"], P["conv2.weight"], P["conv2.bias"],
                P["bn.running_mean"], P["bn.running_var"], P["bn.num_batches_tracked"], t["u"], t["stat"], t["out"],
                B, H, W, C, training=training, momentum=U.MOMENTUM, eps=U.EPS)


def bwd(xd, dyd, P, t, B, H, W, C, training):
    ops.lpi_bwd(xd, t["u"], dyd, t["stat"], P["conv1.weight"], P["conv1.bias"], P["bn.weight"], P["bn.bias"], P["conv2.weight"],
                t["dx"], t["conv1.weight"], t["conv1.bias"], t["bn.weight"], t["bn.bias"], t["conv2.weight"], t["conv2.bias"],
                B, H, W, C, training=training)


def run(x, dy, p, B, H, W, dtype, training):
    C = x.shape[-1]
    P, t = dev_params(p), alloc(B, H, W, C, dtype)
    xd, dyd = x.to(dtype).cuda(), dy.to(dtype).cuda()
    fwd(xd, P, t, B, H, W, C, training)
    bwd(xd, dyd, P, t, B, H, W, C, training)
    torch.cuda.synchronize()
    grads = {k: t[k].cpu().reshape(p[k].shape) for k in U.GRAD_KEYS}
    got = U.LpiRef(t["out"].cpu(), t["u"].cpu(), t["stat"][0].cpu(), t["stat"][1].cpu(), t["dx"].cpu(), grads,
                   P["bn.running_mean"].cpu(), P["bn.running_var"].cpu())
    return got, int(P["bn.num_batches_tracked"].item())


def finite(got):
    return all(torch.isfinite(v).all() for v in (got.out, got.u, got.mean, got.rstd, got.dx, got.running_mean, got.running_var,
                                                 *got.grads.values()))


def reference(x, dy, p, B, H, W, training, got, dtype):
    """float64 autograd on the same operands: in bf16 the op's stored u is one of them; `u` stays the unrounded one"""
    if dtype == torch.float32:
        return plain_reference(x, dy, p, B, H, W, training)
    return U.torch_lpi(x, dy, p, B, H, W, training=training, u_stored=got.u)


_REF = {}


def plain_reference(x, dy, p, B, H, W, training):
    key = (x.data_ptr(), training)
    if key not in _REF:
        _REF[key] = (x, U.torch_lpi(x, dy, p, B, H, W, training=training))       # x kept alive: the key is its address
    return _REF[key][1]


@functools.lru_cache(maxsize=None)
def case_inputs(B, H, W, C, seed, stress=False):
    p = (U.stress_params if stress else U.make_params)(C, seed)
    return (p, *U.make_inputs(B, H, W, C, seed + 50))


# ------------------------------------------------------------------------------------------------- 1: the sweep ---
SWEEP = U.sweep_cases()


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("B,H,W,C,seed", SWEEP, ids=[f"C{c[3]}-{c[0]}x{c[1]}x{c[2]}" for c in SWEEP])
def test_sweep_against_float64(B, H, W, C, seed, dtype, training):
    p, x, dy = case_inputs(B, H, W, C, seed)
    got, count = run(x, dy, p, B, H, W, dtype, training)
    assert finite(got)
    assert count == 5 + int(training)
    want = reference(x, dy, p, B, H, W, training, got, dtype)
    if not training:
        assert torch.equal(got.running_mean, p["bn.running_mean"]) and torch.equal(got.running_var, p["bn.running_var"])
    judge(f"{dtype} C{C} {B}x{H}x{W} {'train' if training else 'eval'}", U.lpi_errors(got, want, training),
          bounds(dtype, EMU_SWEEP, F32_SWEEP))


# ------------------------------------------------------------------------- 2: more workgroups than CUs ---
def per_image_errors(got, want):
    e = U.lpi_errors(got, want, True)
    for k in U.ACT_KEYS:
        g, w = getattr(got, k).double(), getattr(want, k).double()
        e[k] = ((g - w).abs().amax((1, 2)) / w.abs().amax((1, 2))).max().item()
    return e


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_more_workgroups_than_cus(dtype):
    B, H, W, C = U.WIDE_CASE
    p, x, dy = case_inputs(B, H, W, C, 4242)
    got, _ = run(x, dy, p, B, H, W, dtype, True)
    want = reference(x, dy, p, B, H, W, True, got, dtype)
    judge(f"{dtype} 40 images", per_image_errors(got, want), bounds(dtype, EMU_WIDE, F32_WIDE))


# ------------------------------------------------------------------------------- 3: statistics under stress ---
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_statistics_under_stress(dtype):
    B, H, W, C = U.STRESS_CASE
    p, x, dy = case_inputs(B, H, W, C, 777, True)
    got, _ = run(x, dy, p, B, H, W, dtype, True)
    assert finite(got)
    want = reference(x, dy, p, B, H, W, True, got, dtype)
    assert got.rstd[5] == torch.tensor(U.EPS, dtype=torch.float32).double().rsqrt().float()  # a constant channel: variance 0
    judge(f"{dtype} stress", U.lpi_errors(got, want, True), bounds(dtype, EMU_STRESS, F32_STRESS))


# -------------------------------------------------------------------------------------- 4: running buffers ---
def test_running_buffers_follow_the_recurrence():
    B, H, W, C = 3, 5, 4, 72
    p = U.make_params(C, 31)
    P, t = dev_params(p), alloc(B, H, W, C, torch.float32)
    rm, rv = p["bn.running_mean"].double(), p["bn.running_var"].double()
    for i in range(3):
        x, _ = U.make_inputs(B, H, W, C, 900 + 10 * i)
        fwd(x.cuda(), P, t, B, H, W, C, True)
        ref = U.emulated_lpi(x, x, p, B, H, W, rounding=False)
        u = ref.u.reshape(-1, C)
        rm = 0.9 * rm + 0.1 * u.mean(0)
        rv = 0.9 * rv + 0.1 * u.var(0, unbiased=True)
    torch.cuda.synchronize()
    assert int(P["bn.num_batches_tracked"].item()) == 5 + 3
    e = {"running_mean": U.rel(P["bn.running_mean"].cpu(), rm), "running_var": U.rel(P["bn.running_var"].cpu(), rv)}
    judge("three training forwards", e, bounds(torch.float32, EMU_SWEEP, F32_SWEEP))
    before = {k: P[k].clone() for k in U.BUF_KEYS}
    fwd(x.cuda(), P, t, B, H, W, C, False)
    torch.cuda.synchronize()
    for k in U.BUF_KEYS:
        assert torch.equal(P[k], before[k]), f"{k}: an eval forward changed it"


# ------------------------------------------------------------------------------------------ 5: no stray stores ---
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("B,H,W", [(2, 1, 1), (2, 7, 9), (2, 14, 14)])
def test_no_stray_stores(B, H, W, dtype):
    C, G = 72, 1024
    p, x, dy = case_inputs(B, H, W, C, 55)
    P = dev_params(p)
    xd, dyd = x.to(dtype).cuda(), dy.to(dtype).cuda()
    bufs = {}

    def carve(name, n, dt, init=None):
        buf = torch.full((n + 2 * G,), -777, dtype=dt, device="cuda")
        if init is not None:
            buf[G:G + n] = init
        bufs[name] = (buf, n, init is None)
        return buf[G:G + n]
    t = {k: carve(k, B * H * W * C, dtype).view(B, H * W, C) for k in ("u", "out", "dx")}
    t["stat"] = carve("stat", 2 * C, torch.float32)
    for k in U.GRAD_KEYS:
        t[k] = carve(k, p[k].numel(), torch.float32)
    for k in U.BUF_KEYS:
        P[k] = carve(k, P[k].numel(), P[k].dtype, init=P[k])
    fwd(xd, P, t, B, H, W, C, True)
    bwd(xd, dyd, P, t, B, H, W, C, True)
    torch.cuda.synchronize()
    for name, (buf, n, fresh) in bufs.items():
        assert (buf[:G] == -777).all() and (buf[G + n:] == -777).all(), f"{name}: a guard was written"
        if fresh:
            assert (buf[G:G + n] != -777).all(), f"{name}: an element was not written"
    assert not torch.equal(P["bn.running_mean"].cpu(), p["bn.running_mean"]) and int(P["bn.num_batches_tracked"].item()) == 6


# -------------------------------------------------------------------------------------------- 6: determinism ---
def raw_run(xd, dyd, P, B, H, W, C):
    t = alloc(B, H, W, C, xd.dtype, fill=0.0)
    fwd(xd, P, t, B, H, W, C, True)
    bwd(xd, dyd, P, t, B, H, W, C, True)
    return t


@pytest.mark.parametrize("B,H,W,C", [(8, 14, 14, 384), (2, 28, 28, 192)])
def test_bitwise_repeatable(B, H, W, C):
    p, x, dy = case_inputs(B, H, W, C, 66)
    xd, dyd = x.bfloat16().cuda(), dy.bfloat16().cuda()
    Pa, Pb = dev_params(p), dev_params(p)
    a, b = raw_run(xd, dyd, Pa, B, H, W, C), raw_run(xd, dyd, Pb, B, H, W, C)
    torch.cuda.synchronize()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    for k in U.BUF_KEYS:
        assert torch.equal(Pa[k], Pb[k]), k


# ----------------------------------------------------------------------------------------------- 7: refusals ---
def test_refusals():
    def setup(B, H, W, C, dtype):
        P = dev_params(U.make_params(C, 1))
        t = alloc(B, H, W, C, dtype)
        return P, t, torch.zeros((B, H * W, C), dtype=dtype, device="cuda")

    def untouched(P, t, count=5):
        return all(torch.isnan(v).all() for v in t.values()) and int(P["bn.num_batches_tracked"].item()) == count

    P, t, x = setup(2, 3, 3, 100, torch.bfloat16)
    with pytest.raises(VitmiError, match="multiple of 8"):
        fwd(x, P, t, 2, 3, 3, 100, True)
    with pytest.raises(VitmiError, match="multiple of 8"):
        bwd(x, x, P, t, 2, 3, 3, 100, True)
    assert untouched(P, t)
    P, t, x = setup(2, 3, 3, 96, torch.float16)
    with pytest.raises(VitmiError, match="bf16 or fp32"):
        fwd(x, P, t, 2, 3, 3, 96, True)
    assert untouched(P, t)
    P, t, x = setup(2, 0, 3, 96, torch.bfloat16)
    with pytest.raises(VitmiError, match="at least 1"):
        fwd(x, P, t, 2, 0, 3, 96, True)
    assert untouched(P, t)
    P, t, x = setup(2, 3, 3, 96, torch.bfloat16)
    big = torch.zeros(x.numel() + 8, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(VitmiError, match="aligned"):
        fwd(big[1:1 + x.numel()].view_as(x), P, t, 2, 3, 3, 96, True)
    assert untouched(P, t)
    P, t, x = setup(1, 1, 1, 96, torch.bfloat16)
    with pytest.raises(VitmiError, match="more than one position"):
        fwd(x, P, t, 1, 1, 1, 96, True)
    assert untouched(P, t)
    assert not ops.lpi_supported(torch.bfloat16, 2, 3, 3, 100) and ops.lpi_supported(torch.float32, 2, 3, 3, 96)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------- 8: graph replay ---
def test_graph_replay():
    B, H, W, C = 2, 14, 14, 192
    p, x, dy = case_inputs(B, H, W, C, 88)
    xd, dyd = x.bfloat16().cuda(), dy.bfloat16().cuda()
    Pe = dev_params(p)
    eager = raw_run(xd, dyd, Pe, B, H, W, C)            # one forward from the starting buffers
    torch.cuda.synchronize()
    P = dev_params(p)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        raw_run(xd, dyd, P, B, H, W, C)                 # warm the side stream's workspace outside the capture: forward 1
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = raw_run(xd, dyd, P, B, H, W, C)
    torch.cuda.synchronize()
    assert int(P["bn.num_batches_tracked"].item()) == 6, "the capture itself must execute no forward"
    for executed in (2, 3):                              # the warm-up was forward 1
        for v in outs.values():
            v.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        for k in outs:                                   # batch statistics do not depend on the running buffers
            assert torch.equal(outs[k], eager[k]), k
        assert int(P["bn.num_batches_tracked"].item()) == 5 + executed
        u = outs["u"].double().cpu().reshape(-1, C)      # the stored u: what the statistics are defined over
        rm, rv = p["bn.running_mean"].double(), p["bn.running_var"].double()
        for _ in range(executed):
            rm, rv = 0.9 * rm + 0.1 * u.mean(0), 0.9 * rv + 0.1 * u.var(0, unbiased=True)
        e = {"running_mean": U.rel(P["bn.running_mean"].cpu(), rm), "running_var": U.rel(P["bn.running_var"].cpu(), rv)}
        judge(f"replay {executed - 1}", e, bounds(torch.float32, EMU_SWEEP, F32_SWEEP))


# ------------------------------------------------------------------------------------------------ 9: the module ---
@pytest.fixture(scope="module")
def fx():
    return FC.load(os.path.join(HERE, "golden", "lpi.npz"))


FH, FW = 3, 5


def load_module(fx, mode):
    m = LPI(96, compute_dtype=mode)
    m.load_state_dict(FC.group(fx, "state"))
    return m.cuda()


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_module_against_fixture(fx, mode):
    m = load_module(fx, mode).train()
    x = fx["x"].cuda().requires_grad_(True)
    y = m(x, FH, FW)
    y.backward(fx["dy"].cuda())
    torch.cuda.synchronize()
    assert int(m.bn.num_batches_tracked.item()) == int(fx["after/bn.num_batches_tracked"].item())
    got = {"y": y, "dx": x.grad, **{"grad/" + n: p.grad for n, p in m.named_parameters()},
           "buf/bn.running_mean": m.bn.running_mean, "buf/bn.running_var": m.bn.running_var}
    want = {k: fx[k.replace("buf/", "after/")] for k in got}
    first = {n: p.grad.clone() for n, p in m.named_parameters()}
    m.eval()
    with torch.no_grad():
        got["y_eval"] = m(fx["x"].cuda(), FH, FW)
    want["y_eval"] = fx["y_eval"]
    b = {k: 4 * v for k, v in F32_MODULE.items()} if mode == "fp32" else {k: 2 * v for k, v in EMU_MODULE.items()}
    judge(f"module {mode}", {k: U.rel(got[k].detach().float().cpu(), want[k]) for k in b}, b)
    # a second backward accumulates into .grad (torch's contract)
    m.train()
    m(x, FH, FW).backward(fx["dy"].cuda())
    torch.cuda.synchronize()
    for n, p in m.named_parameters():
        assert torch.allclose(p.grad, 2 * first[n], rtol=1e-6, atol=1e-7), f"{n}: .grad did not accumulate"


def test_module_fused_sgd_step(fx):
    m = load_module(fx, "bf16").train()
    opt = FusedSGD(m.parameters(), lr=0.1, momentum=0.9)
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    m(fx["x"].cuda(), FH, FW).backward(fx["dy"].cuda())
    torch.cuda.synchronize()
    bufs = {k: getattr(m.bn, k.split(".")[1]).clone() for k in U.BUF_KEYS}
    opt.step()
    torch.cuda.synchronize()
    for n, p in m.named_parameters():
        assert not torch.equal(p.detach(), before[n]), f"{n} did not move"
        assert torch.isfinite(p).all()
    for k in U.BUF_KEYS:
        assert torch.equal(getattr(m.bn, k.split(".")[1]), bufs[k]), f"{k}: the optimizer step changed a buffer"
