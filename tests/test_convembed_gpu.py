"""The conv-stem kernels (csrc/convstem.hip: ops.conv3s2_im2col / conv3s2_col2im / conv3s2_wcopy / bn_act_fwd / bn_act_bwd)
and the ConvPatchEmbed module on the GPU.

Metric: max |got - want| / max |want| (convembed_util.rel).  Every check prints its error beside its bound (-s).

Gather kernels: EQUALITY with F.unfold / F.fold on inputs that are multiples of 1/8 in [-2, 2]: every cast is exact and a
col2im sum has at most 4 terms with |sum| <= 8, exact in bf16 and fp32 (test_convembed_cpu.py confirms the premise).

Bounds of the rest, measured on the CPU over each section's own inputs and frozen here (rules of test_lpi_gpu.py):
  * bn_act, reference = float64 autograd over the SAME y and dout (y is the operand the statistics are defined over; in bf16
    it is the stored tensor itself, so the reference is straight-through by construction):
      bf16 tensors (out, dy): 2x the error of convembed_util.closed_bn_act with out and dy rounded on store.
        sweep maxima (train and eval, GELU on and off): out 3.60e-3, dy 3.59e-3          stress: out 2.47e-3, dy 2.49e-3
      fp32 tensors, and on both dtypes stat, the running buffers, dgamma, dbeta: 4x the float32 closed form's error.
        sweep maxima: out 2.61e-7, dy 4.13e-4 (M = 2 in training: yh = +-1 and dy is a cancellation down to ~eps / var; every
        other M is below 1e-6), mean 7.85e-8, rstd 1.46e-7, dgamma 3.47e-7, dbeta 2.64e-7, running_mean 1.00e-7,
        running_var 9.37e-8
        stress: out 1.50e-7, dy 1.29e-7, mean 6.41e-9, rstd 5.43e-8, dgamma 2.37e-7, dbeta 1.25e-7, running_mean 2.90e-8,
        running_var 4.31e-8
  * the module against the fixture (the reference class in float32): "fp32": 4x the fixture's own error against float64
    (F32_MODULE below); "bf16": 2x the error of convembed_util.closed_stem with the declared roundings (image -> col, weight
    shadows, y, out, dy, dcol, dx) against the fixture (EMU_MODULE below), for every tensor: the roundings of one stage are
    the operands of the next, so no tensor of the module is an "fp32 tensor on the same operands".  The emulation runs in
    float64, so it carries the declared roundings and nothing of the fp32 accumulation that the bf16 path also has (the last
    stage's bias gradient is a plain sum of the bf16-valued dy: the emulation's error there is exactly 0, an fp32 sum's is
    not); the float32 figure measures exactly that part, so the "bf16" bound of every tensor is 2x the emulation's error
    PLUS 4x the float32 figure of the same tensor (module_bound).  The stored y of each stage against the unrounded float64
    one: 2x EMU_YS.
  * more workgroups than CUs ([64, 3, 64, 64], patch 8, E = 64) against float64 autograd: "fp32" 4x F32_WIDE (the float32
    closed form), "bf16" 2x EMU_WIDE + 4x F32_WIDE, as above.
Measured on an MI355X (one run; DESIGN.md 4.7 has the list): bn_act sweep bf16 out 3.60e-3, dy 3.59e-3; fp32 out 2.61e-7, dy
4.14e-4 at M = 2 and 1.73e-6 elsewhere; dgamma 6.52e-7, dbeta 5.82e-7; module "fp32" tokens 1.24e-6 / 5.83e-7, "bf16" 1.54e-2 /
4.65e-3; the wide case "fp32" weight gradients at most 8.40e-7 (5.93e-6 before the module summed them in two levels).
"""
import functools
import os

import pytest
import torch

import convembed_util as U
import fixture_codec as FC
from vit_torch_amd import ConvPatchEmbed, FusedSGD, VitmiError, ops

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])

EMU_BN = {"out": 3.60e-03, "dy": 3.59e-03}
F32_BN = {"out": 2.61e-07, "dy": 4.13e-04, "mean": 7.85e-08, "rstd": 1.46e-07, "dgamma": 3.47e-07, "dbeta": 2.64e-07,
          "running_mean": 1.00e-07, "running_var": 9.37e-08}
EMU_STRESS = {"out": 2.47e-03, "dy": 2.49e-03}
F32_STRESS = {"out": 1.50e-07, "dy": 1.29e-07, "mean": 6.41e-09, "rstd": 5.43e-08, "dgamma": 2.37e-07, "dbeta": 1.25e-07,
              "running_mean": 2.90e-08, "running_var": 4.31e-08}
F32_MODULE = {
    "p16": {"y": 1.11e-06, "y_eval": 4.77e-07, "grad/proj.0.0.weight": 5.60e-07, "grad/proj.0.1.weight": 1.72e-06,
            "grad/proj.0.1.bias": 5.86e-07, "grad/proj.2.0.weight": 1.07e-06, "grad/proj.2.1.weight": 6.86e-07,
            "grad/proj.2.1.bias": 8.70e-07, "grad/proj.4.0.weight": 9.25e-07, "grad/proj.4.1.weight": 1.18e-06,
            "grad/proj.4.1.bias": 1.06e-06, "grad/proj.6.0.weight": 1.21e-06, "grad/proj.6.1.weight": 1.12e-06,
            "grad/proj.6.1.bias": 0.0, "buf/proj.0.1.running_mean": 6.40e-08, "buf/proj.0.1.running_var": 3.92e-08,
            "buf/proj.2.1.running_mean": 3.65e-08, "buf/proj.2.1.running_var": 5.82e-08, "buf/proj.4.1.running_mean": 5.31e-08,
            "buf/proj.4.1.running_var": 8.78e-08, "buf/proj.6.1.running_mean": 7.73e-08, "buf/proj.6.1.running_var": 7.35e-08},
    "p8": {"y": 3.80e-07, "y_eval": 4.19e-07, "grad/proj.0.0.weight": 5.09e-07, "grad/proj.0.1.weight": 4.37e-07,
           "grad/proj.0.1.bias": 6.30e-07, "grad/proj.2.0.weight": 5.05e-07, "grad/proj.2.1.weight": 4.28e-07,
           "grad/proj.2.1.bias": 5.07e-07, "grad/proj.4.0.weight": 4.98e-07, "grad/proj.4.1.weight": 3.44e-07,
           "grad/proj.4.1.bias": 0.0, "buf/proj.0.1.running_mean": 3.27e-08, "buf/proj.0.1.running_var": 5.19e-08,
           "buf/proj.2.1.running_mean": 8.01e-08, "buf/proj.2.1.running_var": 7.00e-08, "buf/proj.4.1.running_mean": 6.90e-08,
           "buf/proj.4.1.running_var": 7.28e-08}}
EMU_MODULE = {
    "p16": {"y": 1.54e-02, "y_eval": 5.38e-03, "grad/proj.0.0.weight": 7.54e-03, "grad/proj.0.1.weight": 1.50e-02,
            "grad/proj.0.1.bias": 9.38e-03, "grad/proj.2.0.weight": 1.36e-02, "grad/proj.2.1.weight": 1.11e-02,
            "grad/proj.2.1.bias": 1.44e-02, "grad/proj.4.0.weight": 1.21e-02, "grad/proj.4.1.weight": 1.18e-02,
            "grad/proj.4.1.bias": 1.01e-02, "grad/proj.6.0.weight": 3.26e-02, "grad/proj.6.1.weight": 1.96e-02,
            "grad/proj.6.1.bias": 0.0, "buf/proj.0.1.running_mean": 7.57e-05, "buf/proj.0.1.running_var": 3.89e-05,
            "buf/proj.2.1.running_mean": 1.07e-04, "buf/proj.2.1.running_var": 3.23e-05, "buf/proj.4.1.running_mean": 2.44e-04,
            "buf/proj.4.1.running_var": 8.99e-05, "buf/proj.6.1.running_mean": 5.07e-04, "buf/proj.6.1.running_var": 2.65e-04},
    "p8": {"y": 4.65e-03, "y_eval": 4.61e-03, "grad/proj.0.0.weight": 6.90e-03, "grad/proj.0.1.weight": 6.65e-03,
           "grad/proj.0.1.bias": 9.75e-03, "grad/proj.2.0.weight": 7.95e-03, "grad/proj.2.1.weight": 7.43e-03,
           "grad/proj.2.1.bias": 6.05e-03, "grad/proj.4.0.weight": 6.42e-03, "grad/proj.4.1.weight": 5.60e-03,
           "grad/proj.4.1.bias": 0.0, "buf/proj.0.1.running_mean": 3.60e-05, "buf/proj.0.1.running_var": 4.04e-05,
           "buf/proj.2.1.running_mean": 1.31e-04, "buf/proj.2.1.running_var": 4.69e-05, "buf/proj.4.1.running_mean": 2.37e-04,
           "buf/proj.4.1.running_var": 1.10e-04}}
EMU_YS = {"p16": (2.86e-03, 3.33e-03, 4.63e-03, 5.01e-03), "p8": (1.99e-03, 2.61e-03, 4.69e-03)}
F32_WIDE = {"y": 6.88e-07, "buf/proj.0.1.running_mean": 7.54e-08, "buf/proj.0.1.running_var": 7.46e-08,
            "buf/proj.2.1.running_mean": 7.02e-08, "buf/proj.2.1.running_var": 9.25e-08, "buf/proj.4.1.running_mean": 7.01e-08,
            "buf/proj.4.1.running_var": 4.31e-08, "grad/proj.0.0.weight": 6.02e-07, "grad/proj.0.1.weight": 8.70e-07,
            "grad/proj.0.1.bias": 8.30e-07, "grad/proj.2.0.weight": 4.70e-07, "grad/proj.2.1.weight": 6.13e-07,
            "grad/proj.2.1.bias": 1.03e-06, "grad/proj.4.0.weight": 6.27e-07, "grad/proj.4.1.weight": 4.05e-07,
            "grad/proj.4.1.bias": 6.01e-08}
EMU_WIDE = {"y": 5.01e-03, "buf/proj.0.1.running_mean": 3.68e-06, "buf/proj.0.1.running_var": 4.15e-06,
            "buf/proj.2.1.running_mean": 2.29e-05, "buf/proj.2.1.running_var": 2.74e-06, "buf/proj.4.1.running_mean": 3.22e-05,
            "buf/proj.4.1.running_var": 6.47e-06, "grad/proj.0.0.weight": 5.90e-03, "grad/proj.0.1.weight": 7.24e-03,
            "grad/proj.0.1.bias": 5.04e-03, "grad/proj.2.0.weight": 5.19e-03, "grad/proj.2.1.weight": 6.58e-03,
            "grad/proj.2.1.bias": 6.55e-03, "grad/proj.4.0.weight": 5.41e-03, "grad/proj.4.1.weight": 3.35e-03,
            "grad/proj.4.1.bias": 0.0}


def bounds(dtype, emu, f32):
    b = {k: 4 * v for k, v in f32.items()}
    if dtype == torch.bfloat16:
        b.update({k: 2 * v for k, v in emu.items()})
    return b


def module_bound(mode, emu, f32):
    """the module's bounds: "fp32" 4x the float32 figure; "bf16" 2x the float64 emulation's error plus that (docstring)"""
    return {k: 4 * v + (2 * emu[k] if mode == "bf16" else 0.0) for k, v in f32.items()}


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


# ------------------------------------------------------------------------------------------- 1: the gathers, exact ---
@DTYPES
@pytest.mark.parametrize("B", U.GATHER_B)
@pytest.mark.parametrize("H,W", U.GATHER_GRIDS)
def test_im2col_image_form_is_exact(H, W, B, dtype):
    Ho, Wo = U.out_grid(H, W)
    x = U.grid_values((B, 3, H, W), 100 * H + W + B)
    want = U.unfold_cols(x)
    for form, xd in (("nchw", x.cuda()), ("channels_last", x.cuda().contiguous(memory_format=torch.channels_last))):
        buf, col = guarded(B * Ho * Wo * 32, dtype)
        ops.conv3s2_im2col(xd, col.view(-1, 32), B, H, W, 3)
        torch.cuda.synchronize()
        got = col.view(-1, 32).float().cpu()
        assert torch.equal(got[:, :27], want), form
        assert (got[:, 27:] == 0).all() and guards_untouched(buf, col.numel()), form


TOKEN_CASES = [(C, 9 * C) for C in U.GATHER_C] + [(24, 9 * 24 + 8)]


@DTYPES
@pytest.mark.parametrize("C,ld", TOKEN_CASES, ids=[f"C{c}-ld{l}" for c, l in TOKEN_CASES])
@pytest.mark.parametrize("B", U.GATHER_B)
@pytest.mark.parametrize("H,W", U.GATHER_GRIDS)
def test_im2col_and_col2im_token_form_are_exact(H, W, B, C, ld, dtype):
    Ho, Wo = U.out_grid(H, W)
    M = B * Ho * Wo
    x = U.grid_values((B, H * W, C), 100 * H + W + B + C)
    buf, col = guarded(M * ld, dtype)
    ops.conv3s2_im2col(x.to(dtype).cuda(), col.view(M, ld), B, H, W, C)
    torch.cuda.synchronize()
    got = col.view(M, ld).float().cpu()
    assert torch.equal(got[:, :9 * C], U.unfold_cols(U.tok_to_grid(x, B, H, W)))
    assert (got[:, 9 * C:] == 0).all() and guards_untouched(buf, col.numel())
    dcol = torch.zeros((M, ld))
    dcol[:, :9 * C] = U.grid_values((M, 9 * C), 7 * H + W + C)
    dcol[:, 9 * C:] = 1.0                                      # pad columns belong to no pixel: they must not be read into dx
    dbuf, dx = guarded(B * H * W * C, dtype)
    ops.conv3s2_col2im(dcol.to(dtype).cuda(), dx.view(B, H * W, C), B, H, W, C)
    torch.cuda.synchronize()
    want = U.grid_to_tok(U.fold_cols(dcol[:, :9 * C].double(), B, H, W))
    assert torch.equal(dx.view(B, H * W, C).double().cpu(), want) and guards_untouched(dbuf, dx.numel())


@DTYPES
def test_wcopy_pads_and_copies_back(dtype):
    w = U.grid_values((16, 27), 5).to(dtype).cuda()
    buf, img = guarded(16 * 32, dtype)
    ops.conv3s2_wcopy(w, img.view(16, 32), 27)
    back_buf, back = guarded(16 * 27, dtype)
    ops.conv3s2_wcopy(img.view(16, 32), back.view(16, 27), 27)
    torch.cuda.synchronize()
    assert torch.equal(img.view(16, 32)[:, :27], w) and (img.view(16, 32)[:, 27:] == 0).all() and guards_untouched(buf, 512)
    assert torch.equal(back.view(16, 27), w) and guards_untouched(back_buf, 16 * 27)


# ------------------------------------------------------------------------------------------------- 2: bn_act ---
def dev_bn(p):
    return {k: v.clone().to("cuda", torch.int64 if k.endswith("tracked") else torch.float32).reshape(-1) for k, v in p.items()}


def bn_alloc(M, C, dtype, fill=float("nan")):
    t = {k: torch.full((M, C), fill, dtype=dtype, device="cuda") for k in ("out", "dy")}
    t["stat"] = torch.full((2, C), fill, dtype=torch.float32, device="cuda")
    t["dgamma"], t["dbeta"] = (torch.full((C,), fill, dtype=torch.float32, device="cuda") for _ in range(2))
    return t


def bn_fwd(yd, P, t, M, C, gelu, training):
    ops.bn_act_fwd(yd, P["weight"], P["bias"], P["running_mean"], P["running_var"], P["num_batches_tracked"], t["stat"],
                   t["out"], M, C, gelu=gelu, training=training, momentum=U.MOMENTUM, eps=U.EPS)


def bn_bwd(dd, yd, P, t, M, C, gelu, training):
    ops.bn_act_bwd(dd, yd, t["stat"], P["weight"], P["bias"], t["dy"], t["dgamma"], t["dbeta"], M, C, gelu=gelu,
                   training=training)


def bn_run(y, d, p, dtype, gelu, training):
    M, C = y.shape
    P, t = dev_bn(p), bn_alloc(M, C, dtype)
    yd, dd = y.to(dtype).cuda(), d.to(dtype).cuda()
    bn_fwd(yd, P, t, M, C, gelu, training)
    bn_bwd(dd, yd, P, t, M, C, gelu, training)
    torch.cuda.synchronize()
    got = U.BnRef(t["out"].cpu(), t["stat"][0].cpu(), t["stat"][1].cpu(), t["dy"].cpu(), t["dgamma"].cpu(), t["dbeta"].cpu(),
                  P["running_mean"].cpu(), P["running_var"].cpu())
    return got, int(P["num_batches_tracked"].item())


def bn_finite(got):
    return all(torch.isfinite(v).all() for v in got)


@functools.lru_cache(maxsize=None)
def bn_case(M, C, seed):
    return (U.bn_params(C, seed), *U.bn_inputs(M, C, seed + 50))


@functools.lru_cache(maxsize=None)
def bn_reference(M, C, seed, gelu, training):
    p, y, d = bn_case(M, C, seed)
    return U.torch_bn_act(y, d, p, gelu, training)


BN_CASES = U.bn_cases()


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("gelu", [True, False], ids=["gelu", "plain"])
@DTYPES
@pytest.mark.parametrize("M,C,seed", BN_CASES, ids=[f"C{c[1]}-M{c[0]}" for c in BN_CASES])
def test_bn_act_against_float64(M, C, seed, dtype, gelu, training):
    p, y, d = bn_case(M, C, seed)
    got, count = bn_run(y, d, p, dtype, gelu, training)
    assert bn_finite(got) and count == 5 + int(training)
    if not training:
        assert torch.equal(got.running_mean, p["running_mean"]) and torch.equal(got.running_var, p["running_var"])
    judge(f"{dtype} C{C} M{M} {'gelu' if gelu else 'plain'} {'train' if training else 'eval'}",
          U.bn_errors(got, bn_reference(M, C, seed, gelu, training), training), bounds(dtype, EMU_BN, F32_BN))


@pytest.mark.parametrize("gelu", [True, False], ids=["gelu", "plain"])
@DTYPES
def test_bn_act_statistics_under_stress(dtype, gelu):
    p, y, d = U.bn_stress()
    got, _ = bn_run(y, d, p, dtype, gelu, True)
    assert bn_finite(got)
    assert got.rstd[3] == torch.tensor(U.EPS, dtype=torch.float32).double().rsqrt().float()     # a constant channel: M2 = 0
    judge(f"{dtype} stress", U.bn_errors(got, U.torch_bn_act(y, d, p, gelu, True)), bounds(dtype, EMU_STRESS, F32_STRESS))


def test_bn_act_running_buffers_follow_the_recurrence():
    M, C = 257, 24
    p = U.bn_params(C, 31)
    P, t = dev_bn(p), bn_alloc(M, C, torch.float32)
    rm, rv = p["running_mean"].double(), p["running_var"].double()
    for i in range(3):
        y, _ = U.bn_inputs(M, C, 900 + 10 * i)
        bn_fwd(y.cuda(), P, t, M, C, True, True)
        rm, rv = 0.9 * rm + 0.1 * y.double().mean(0), 0.9 * rv + 0.1 * y.double().var(0, unbiased=True)
    torch.cuda.synchronize()
    assert int(P["num_batches_tracked"].item()) == 5 + 3
    e = {"running_mean": U.rel(P["running_mean"].cpu(), rm), "running_var": U.rel(P["running_var"].cpu(), rv)}
    judge("three training forwards", e, bounds(torch.float32, EMU_BN, F32_BN))
    before = {k: P[k].clone() for k in ("running_mean", "running_var", "num_batches_tracked")}
    bn_fwd(y.cuda(), P, t, M, C, True, False)
    torch.cuda.synchronize()
    for k, v in before.items():
        assert torch.equal(P[k], v), f"{k}: an eval forward changed it"


@DTYPES
def test_bn_act_bitwise_repeatable_and_no_stray_stores(dtype):
    M, C = 4100, 96
    p, y, d = bn_case(M, C, 66)
    yd, dd = y.to(dtype).cuda(), d.to(dtype).cuda()
    runs = []
    for _ in range(2):
        P = dev_bn(p)
        bufs = {k: guarded(n, dt) for k, n, dt in (("out", M * C, dtype), ("dy", M * C, dtype), ("stat", 2 * C, torch.float32),
                                                   ("dgamma", C, torch.float32), ("dbeta", C, torch.float32))}
        t = {k: v[1].view((M, C) if k in ("out", "dy") else (2, C) if k == "stat" else (C,)) for k, v in bufs.items()}
        bn_fwd(yd, P, t, M, C, True, True)
        bn_bwd(dd, yd, P, t, M, C, True, True)
        torch.cuda.synchronize()
        for k, (buf, view) in bufs.items():
            assert guards_untouched(buf, view.numel()) and not torch.isnan(view).any(), k
        runs.append({**t, **{k: P[k] for k in ("running_mean", "running_var", "num_batches_tracked")}})
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k


# ------------------------------------------------------------------------------------------------ 3: the module ---
@pytest.fixture(scope="module")
def fx():
    return FC.load(os.path.join(HERE, "golden", "conv_patch_embed.npz"))


def load_module(st, patch, mode, E=64):
    m = ConvPatchEmbed(img_size=32, patch_size=patch, embed_dim=E, compute_dtype=mode)
    m.load_state_dict(st)
    return m.cuda()


def module_outputs(m, x, dy, patch):
    y, grid = m(x.cuda())
    y.backward(dy.cuda())
    torch.cuda.synchronize()
    got = {"y": y.detach(), **{"grad/" + n: p.grad for n, p in m.named_parameters()}}
    got.update({"buf/" + k: m.state_dict()[k] for k in U.buffer_keys(patch) if not k.endswith("tracked")})
    return got, grid


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["p16", "p8"])
def test_module_against_fixture(fx, name, mode):
    x, dy, st, patch, want = U.fixture_case(fx, name)
    m = load_module(st, patch, mode).train()
    y, grid = m(x.cuda())
    ys = [s[1].float().cpu() for s in m._saved[0]]                 # each stage's conv output as stored
    y.backward(dy.cuda())
    torch.cuda.synchronize()
    assert tuple(grid) == tuple(FC.group(fx, name)["grid"].tolist()) and y.dtype == torch.float32
    sd = m.state_dict()
    for k in U.buffer_keys(patch):
        if k.endswith("tracked"):
            assert int(sd[k]) == int(FC.group(fx, name)["after/" + k])
    got = {"y": y.detach(), **{"grad/" + n: p.grad for n, p in m.named_parameters()}}
    got.update({"buf/" + k: sd[k] for k in U.buffer_keys(patch) if not k.endswith("tracked")})
    first = {n: p.grad.clone() for n, p in m.named_parameters()}
    m.eval()
    with torch.no_grad():
        got["y_eval"] = m(x.cuda())[0]
    b = module_bound(mode, EMU_MODULE[name], F32_MODULE[name])
    judge(f"module {name} {mode}", U.module_errors(got, want), b)
    if mode == "bf16":                                             # each stage's stored y against the unrounded float64 one
        exact = U.torch_stem(x, None, st, patch, True)["ys"]
        judge(f"stored y {name}", {f"y{i}": U.rel(a.reshape(e.shape), e) for i, (a, e) in enumerate(zip(ys, exact))},
              {f"y{i}": 2 * v for i, v in enumerate(EMU_YS[name])})
    m.train()                                                      # a second backward accumulates into .grad
    m(x.cuda())[0].backward(dy.cuda())
    torch.cuda.synchronize()
    for n, p in m.named_parameters():
        assert torch.allclose(p.grad, 2 * first[n], rtol=1e-5, atol=1e-6), f"{n}: .grad did not accumulate"


def test_module_fused_sgd_step(fx):
    x, dy, st, patch, _ = U.fixture_case(fx, "p16")
    m = load_module(st, patch, "bf16").train()
    opt = FusedSGD(m.parameters(), lr=0.1, momentum=0.9)
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    m(x.cuda())[0].backward(dy.cuda())
    torch.cuda.synchronize()
    opt.step()
    torch.cuda.synchronize()
    for n, p in m.named_parameters():
        assert not torch.equal(p.detach(), before[n]), f"{n} did not move"
        assert torch.isfinite(p).all()


def test_module_graph_replay(fx):
    x, dy, st, patch, _ = U.fixture_case(fx, "p8")
    xd = x.cuda()
    eager = load_module(st, patch, "bf16").train()
    with torch.no_grad():
        want = eager(xd)[0]
    m = load_module(st, patch, "bf16").train()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        m(xd)                                                       # warm-up outside the capture: forward 1
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    count = lambda: [int(m.state_dict()[k]) for k in U.buffer_keys(patch) if k.endswith("tracked")]  # noqa: E731
    start = count()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g), torch.no_grad():
        out = m(xd)[0]
    torch.cuda.synchronize()
    assert count() == start, "the capture itself must execute no forward"
    for n in (1, 2):
        out.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want)                               # batch statistics do not depend on the running buffers
        assert count() == [c + n for c in start]


@functools.lru_cache(maxsize=None)
def wide_reference():
    shape, patch, E = U.WIDE_CASE
    st = U.wide_state(patch, E, 97)
    x, dy = U.bf16(U.gen(shape, 98)), U.bf16(U.gen((shape[0], 64, E), 99))
    return st, x, dy, U.torch_stem(x, dy, st, patch, True)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_module_more_workgroups_than_cus(mode):
    _, patch, E = U.WIDE_CASE
    st, x, dy, ref = wide_reference()
    got, grid = module_outputs(load_module(st, patch, mode, E).train(), x, dy, patch)
    assert tuple(grid) == (8, 8)
    b = module_bound(mode, EMU_WIDE, F32_WIDE)
    judge(f"wide {mode}", {k: U.rel(got[k].float().cpu(), ref[k]) for k in b}, b)


# ------------------------------------------------------------------------------------------------ 4: refusals ---
def test_refusals():
    def untouched(t, P):
        return all(torch.isnan(v).all() for v in t.values()) and int(P["num_batches_tracked"].item()) == 5

    def setup(M, C, dtype):
        return dev_bn(U.bn_params(C, 1)), bn_alloc(M, C, dtype), torch.zeros((M, C), dtype=dtype, device="cuda")

    P, t, y = setup(9, 100, torch.bfloat16)
    with pytest.raises(VitmiError, match="multiple of 8"):
        bn_fwd(y, P, t, 9, 100, True, True)
    with pytest.raises(VitmiError, match="multiple of 8"):
        bn_bwd(y, y, P, t, 9, 100, True, True)
    assert untouched(t, P)
    P, t, y = setup(9, 96, torch.float16)
    with pytest.raises(VitmiError, match="bf16 or fp32"):
        bn_fwd(y, P, t, 9, 96, True, True)
    assert untouched(t, P)
    P, t, y = setup(1, 96, torch.bfloat16)
    with pytest.raises(VitmiError, match="more than one row"):
        bn_fwd(y, P, t, 1, 96, True, True)
    assert untouched(t, P)
    P, t, y = setup(9, 96, torch.bfloat16)
    big = torch.zeros(y.numel() + 8, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(VitmiError, match="aligned"):
        bn_fwd(big[1:1 + y.numel()].view_as(y), P, t, 9, 96, True, True)
    with pytest.raises(VitmiError, match="aligned"):
        bn_bwd(big[1:1 + y.numel()].view_as(y), y, P, t, 9, 96, True, True)
    assert untouched(t, P)
    assert not ops.bn_act_supported(torch.bfloat16, 9, 100) and ops.bn_act_supported(torch.float32, 9, 96)
    # the gathers
    B, H, W = 2, 5, 3
    col = torch.full((B * 3 * 2, 9 * 24), float("nan"), dtype=torch.bfloat16, device="cuda")
    x = torch.zeros((B, H * W, 24), dtype=torch.bfloat16, device="cuda")
    with pytest.raises(VitmiError, match="multiple of 8"):
        ops.conv3s2_im2col(torch.zeros((B, H * W, 12), dtype=torch.bfloat16, device="cuda"), col[:, :112], B, H, W, 12)
    with pytest.raises(VitmiError, match="bf16 or fp32"):
        ops.conv3s2_im2col(x.half(), col.half(), B, H, W, 24)
    big = torch.zeros(x.numel() + 8, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(VitmiError, match="aligned"):
        ops.conv3s2_im2col(big[1:1 + x.numel()].view_as(x), col, B, H, W, 24)
    dx = torch.full((B, H * W, 24), float("nan"), dtype=torch.bfloat16, device="cuda")
    with pytest.raises(VitmiError, match="aligned"):
        ops.conv3s2_col2im(col, big[1:1 + x.numel()].view_as(x), B, H, W, 24)
    with pytest.raises(VitmiError, match="fp32 \\[B, C, H, W\\]"):
        ops.conv3s2_im2col(torch.zeros((B, 3, H, W), dtype=torch.bfloat16, device="cuda"),
                           torch.empty((B * 3 * 2, 32), dtype=torch.bfloat16, device="cuda"), B, H, W, 3)
    torch.cuda.synchronize()
    assert torch.isnan(col).all() and torch.isnan(dx).all() and (big == 0).all()
    assert not ops.conv3s2_supported(torch.bfloat16, B, H, W, 12, 112) and ops.conv3s2_supported(torch.float32, B, H, W, 3, 32, image=True)
    # the module
    m = ConvPatchEmbed(32, 16, embed_dim=64).cuda().train()
    with pytest.raises(VitmiError, match="requires_grad"):
        m(torch.zeros((2, 3, 32, 32), device="cuda", requires_grad=True))
    with pytest.raises(VitmiError, match="at least two output positions"):
        m(torch.zeros((1, 3, 16, 16), device="cuda"))
    assert all(int(v) == 0 for k, v in m.state_dict().items() if k.endswith("tracked"))
