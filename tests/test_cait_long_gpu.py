"""CaiT at 384 and 448 pixels: talking-heads attention over 576 / 784 patch tokens with 4, 6, 8 or 16 heads, and class
attention over 577 / 785 tokens.  Before these kernels existed every shape here raised VitmiError.

  * th_softmax_fwd / _bwd over rows of up to 1024 keys and up to 16 heads (the workgroup-per-row kernels of
    cait_ops.hip), composed with the batched products as the engine runs them: the three-call form (fp32 parity modes)
    and the bf16 long op (ops.th_long_fwd / _bwd: the same kernels, the score tensors recomputed by the backward).
  * class_attn_fwd / _bwd over 577 and 785 tokens, the bf16 vector form and the generic fp32 form.
  * the seven newly running arch names at reduced depth against oracle/cait_ref.py, and cait_S24 at full size.

Error metric: max |got - want| / max |want| over the whole tensor (util.rel_err), both sides on the same bf16-rounded
operands, against float64 (tests/cait_util.py).  Bounds, each 2-3x the largest value measured on an MI355X (in brackets;
every check prints its error beside its bound with -s):
  * fp32: FP32 = 3e-6, the bound of tests/test_cait_attention_c4_gpu.py [talking heads 1.7e-6, class attention 1.2e-6].
    The kernels compute and store in fp32; the longer rows add only longer fp32 sums.
  * bf16 talking heads: S, P and P' are stored in bf16 between the calls, as in the three-call form at 224 pixels, so O
    carries three roundings of the score path and its own store [5.0e-3]: OUT = 1.5e-2; dq / dk / dv add bf16 dP' and dS
    [4.8e-3]: DQKV = 1.2e-2; dWl / dWw / dbw are fp32 sums of products of those bf16 operands [5.9e-3]: DW = 1.2e-2.
  * bf16 class attention: one bf16 rounding at the store [2.7e-3]: VEC = 8e-3; the saved softmax is fp32: FP32 [7e-7].
  * Peaked rows (qkv scaled 3.5x, median row maximum of P 0.97): a large bf16 score is rounded by up to 2^-8 of itself,
    which moves its exponential by several percent [O 2.8e-2, dqkv 5.1e-2, dWl 3.5e-2]: PEAK_OUT = 7e-2 for O; PEAK =
    1.5e-1 for dqkv and the parameter gradients, the C4 file's bound for dq / dk / dv in the same case.
  * Against the reference's own classes (tests/golden/*_576.npz, *_577.npz): FIX_FP32 = 1e-4, the bound of the window-12
    fixture tests; FIX_BF16 below.
"""
from functools import partial

import pytest
import torch
import torch.nn as nn

from cait_util import torch_class_attention, torch_talking_heads
from util import assert_close, bf16_round, rel_err

pytestmark = pytest.mark.gpu

F64, bt, f32 = torch.float64, torch.bfloat16, torch.float32
HD = 48
FP32 = 3e-6
OUT, DQKV, DW = 1.5e-2, 1.2e-2, 1.2e-2
VEC = 8e-3
PEAK_OUT, PEAK = 7e-2, 1.5e-1


@pytest.fixture(scope="module")
def ops(lib):
    from vit_torch_amd import ops as _o
    return _o


def gen(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator("cpu").manual_seed(seed)) * scale


def nan(shape, dt):
    return torch.full(shape, float("nan"), device="cuda", dtype=dt)


def check(name, got, want, bound):
    g = got.detach().float().cpu()
    assert tuple(g.shape) == tuple(want.shape), f"{name}: shape {tuple(g.shape)} vs {tuple(want.shape)}"
    assert torch.isfinite(g).all(), f"{name}: non-finite values in result"
    e = rel_err(got.detach().double().cpu(), want.double())
    print(f"\n  {name}: {e:.2e} (bound {bound:.1e})", end="")
    assert e <= bound, f"{name}: rel-to-max error {e:.3e} > {bound:.1e}"


def th_params(H, seed):
    g = torch.Generator("cpu").manual_seed(seed)
    eye = torch.eye(H)
    return (eye + 0.3 * torch.randn(H, H, generator=g), 0.2 * torch.randn(H, generator=g),
            eye + 0.3 * torch.randn(H, H, generator=g), 0.05 * torch.randn(H, generator=g))


def th_inputs(B, H, N, dt, seed, scale=0.7):
    rd = (lambda t: t) if dt == f32 else bf16_round
    return rd(gen((B, N, 3, H, HD), seed) * scale), rd(gen((B, N, H, HD), seed + 1)), th_params(H, seed + 2)


def th_run(ops, qkv, dO, W, dt):
    """forward + backward on the device as the engine runs them: bf16 through the long op, fp32 through the three-call
    form.  Returns (O [B,N,H*hd], dqkv [B,N,3,H,hd], [dWl, dbl, dWw, dbw])."""
    B, N, _, H, hd = qkv.shape
    D = H * hd
    Q = qkv.to("cuda", dt).contiguous()
    G = dO.to("cuda", dt).reshape(B * N, D).contiguous()
    Wd = [t.to("cuda", f32).contiguous() for t in W]
    O = nan((B * N, D), dt)
    dqkv = nan((B * N, 3 * D), dt)
    gr = [nan((H, H), f32), nan((H,), f32), nan((H, H), f32), nan((H,), f32)]
    if dt == bt:
        ops.th_long_fwd(Q, *Wd, O, B, H, N, hd, hd ** -0.5)
        ops.th_long_bwd(Q, G, *Wd, dqkv, *gr, B, H, N, hd, hd ** -0.5)
    else:
        NS = (N + 7) // 8 * 8
        S, P, Pm = ops.th_three_call_fwd(Q, *Wd, O, B, H, N, hd, hd ** -0.5, NS)
        ops.th_three_call_bwd(Q, G, S, P, Pm, Wd[0], Wd[2], dqkv, *gr, B, H, N, hd, hd ** -0.5, NS)
    torch.cuda.synchronize()
    return O.view(B, N, D), dqkv.view(B, N, 3, H, hd), gr


def th_against_float64(ops, tag, qkv, dO, W, dt, b_out, b_dqkv, b_dw):
    r = torch_talking_heads(qkv, dO, *W, HD ** -0.5, dtype=F64, images_per_chunk=1)
    O, dqkv, gr = th_run(ops, qkv, dO, W, dt)
    check(f"{tag}.out", O, r.out, b_out)
    check(f"{tag}.dqkv", dqkv, r.dqkv, b_dqkv)
    check(f"{tag}.dWl", gr[0], r.dWl, b_dw)
    check(f"{tag}.dWw", gr[2], r.dWw, b_dw)
    check(f"{tag}.dbw", gr[3], r.dbw, b_dw)
    # d bl is analytically zero: rounding noise only, bounded against the scale of dWl
    assert gr[1].abs().max().item() <= (1e-5 if dt == f32 else 2e-2) * r.dWl.abs().max().item()


# (H, N): the 384 / 448-pixel variants' attention, the XXS _224 shape, and a row that is no multiple of 4, 8 or 16
TH_SHAPES = [(4, 196), (4, 576), (6, 576), (8, 576), (16, 576), (16, 784), (6, 301)]


@pytest.mark.parametrize("dt", [bt, f32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("H,N", TH_SHAPES, ids=[f"h{h}n{n}" for h, n in TH_SHAPES])
def test_long_talking_heads_against_float64(ops, H, N, dt):
    B = 2 if N * H <= 4608 else 1
    qkv, dO, W = th_inputs(B, H, N, dt, 100 + H + N)
    fp = dt == f32
    th_against_float64(ops, f"th.{'fp32' if fp else 'bf16'}.h{H}n{N}", qkv, dO, W, dt,
                       FP32 if fp else OUT, FP32 if fp else DQKV, FP32 if fp else DW)


@pytest.mark.parametrize("dt", [bt, f32], ids=["bf16", "fp32"])
def test_long_talking_heads_max_on_the_last_key(ops, dt):
    """Every row's largest mixed score on key N - 1 = 575, the last key of the row (as the C4 file's case at 196)."""
    H, N = 8, 576
    g = torch.Generator("cpu").manual_seed(5)
    u = torch.randn(1, 1, H, HD, generator=g) * 0.5
    x = torch.randn(1, N, 3, H, HD, generator=g) * 0.5
    x[:, :, 0] += u                                   # every query leans on u ...
    x[:, N - 1, 1] = 4.0 * u[0, 0]                    # ... and so does the last key, strongly
    qkv = x if dt == f32 else bf16_round(x)
    dO = gen((1, N, H, HD), 6)
    dO = dO if dt == f32 else bf16_round(dO)
    _, bl, Ww, bw = th_params(H, 7)
    Wl = torch.eye(H) + 0.1 * gen((H, H), 8)          # proj_l rows sum to about 1: the mix keeps key N - 1 on top
    q = qkv.double()[:, :, 0].permute(0, 2, 1, 3) * HD ** -0.5
    S = q @ qkv.double()[:, :, 1].permute(0, 2, 3, 1)
    Sm = (S.permute(0, 2, 3, 1) @ Wl.double().t() + bl.double()).permute(0, 3, 1, 2)
    assert (Sm.argmax(-1) == N - 1).float().mean().item() == 1.0
    fp = dt == f32
    th_against_float64(ops, f"th.last_key.{'fp32' if fp else 'bf16'}", qkv, dO, (Wl, bl, Ww, bw), dt,
                       FP32 if fp else OUT, FP32 if fp else DQKV, FP32 if fp else DW)


def test_long_talking_heads_peaked_rows(ops):
    """qkv scaled 3.5x at H = 16, N = 576: softmax rows nearly one-hot (median row maximum of P above 0.9)."""
    H, N = 16, 576
    qkv, dO, W = th_inputs(1, H, N, bt, 11, scale=3.5)
    q = qkv.double()[:, :, 0].permute(0, 2, 1, 3) * HD ** -0.5
    P = ((q @ qkv.double()[:, :, 1].permute(0, 2, 3, 1)).permute(0, 2, 3, 1) @ W[0].double().t()
         + W[1].double()).permute(0, 3, 1, 2).softmax(-1)
    print(f"\n  peaked: median row max of P {P.amax(-1).median().item():.3f}", end="")
    assert P.amax(-1).median().item() > 0.9
    th_against_float64(ops, "th.peaked.bf16", qkv, dO, W, bt, PEAK_OUT, PEAK, PEAK)


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


@pytest.mark.parametrize("H,N", [(8, 576), (16, 784)], ids=["h8n576", "h16n784"])
def test_long_talking_heads_deterministic_and_batch_invariant(ops, H, N):
    """Two runs bit-identical (outputs and parameter gradients); each image's O and dqkv rows equal, bit for bit, a
    launch of that image alone."""
    B = 3
    qkv, dO, W = th_inputs(B, H, N, bt, 21)
    a = th_run(ops, qkv, dO, W, bt)
    b = th_run(ops, qkv, dO, W, bt)
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])
    for x, y in zip(a[2], b[2]):
        assert same_bits(x, y)
    for i in range(B):
        one = th_run(ops, qkv[i:i + 1], dO[i:i + 1], W, bt)
        assert same_bits(a[0][i:i + 1], one[0]), f"image {i}: O differs from a single-image launch"
        assert same_bits(a[1][i:i + 1], one[1]), f"image {i}: dqkv differs from a single-image launch"


def test_long_shapes_are_refused_past_their_limits(ops):
    from vit_torch_amd._lib import VitmiError
    assert not ops.th_long_supported(bt, 17, 576, HD) and not ops.th_long_supported(bt, 8, 1025, HD)
    assert not ops.th_long_supported(f32, 8, 576, HD)
    q = torch.zeros((1, 1025, 3, 8, HD), dtype=bt, device="cuda")
    W = [t.cuda() for t in th_params(8, 1)]
    with pytest.raises(VitmiError, match="N <= 1024"):
        ops.th_long_fwd(q, *W, torch.empty((1025, 8 * HD), dtype=bt, device="cuda"), 1, 8, 1025, HD, 0.1)
    S = torch.zeros((1, 17, 4, 8), dtype=f32, device="cuda")
    with pytest.raises(VitmiError, match="at most 16"):
        ops.th_softmax_fwd(S, *[torch.zeros(17 * 17, device="cuda")] * 4, S, S, 1, 17, 4, 4, 8)
    S = torch.zeros((1, 1, 1, 1032), dtype=f32, device="cuda")
    W1 = torch.zeros(1, device="cuda")
    with pytest.raises(VitmiError, match=r"\[1, 1024\]"):
        ops.th_softmax_fwd(S, W1, W1, W1, W1, S, S, 1, 1, 1, 1025, 1032)
    # the fused op's own query answers as before
    assert not ops.th_attn_supported(bt, 8, 576, HD) and not ops.th_attn_supported(bt, 16, 196, HD)


# ------------------------------------------------------------------------------------------ class attention ---
def class_attention(ops, q, kv, do, B, H, N, hd, dt):
    D = H * hd
    Q, DO = q.to("cuda", dt).contiguous(), do.to("cuda", dt).contiguous()
    KV = kv.to("cuda", dt)
    k, v = KV[:, :D].contiguous(), KV[:, D:].contiguous()
    out, ps = nan((B, D), dt), nan((B * H * N,), f32)
    ops.class_attn_fwd(Q, k, v, D, out, ps, B, H, N, hd, hd ** -0.5)
    dq, dk, dv = nan((B, D), dt), nan((B * N, D), dt), nan((B * N, D), dt)
    ops.class_attn_bwd(Q, k, v, D, DO, ps, dq, dk, dv, D, B, H, N, hd, hd ** -0.5)
    torch.cuda.synchronize()
    return out, ps, dq, dk.view(B, N, D), dv.view(B, N, D)


CA_CASES = [(8, 577, bt), (8, 577, f32), (16, 785, bt), (16, 785, f32), (4, 1025, bt), (6, 1025, f32)]


@pytest.mark.parametrize("H,N,dt", CA_CASES, ids=[f"h{h}n{n}-{'bf16' if d == bt else 'fp32'}" for h, n, d in CA_CASES])
def test_long_class_attention_against_float64(ops, H, N, dt):
    B = 4
    D = H * HD
    rd = (lambda t: t) if dt == f32 else bf16_round
    q, kv, do = rd(gen((B, D), 40 + N)), rd(gen((B * N, 2 * D), 41 + N)), rd(gen((B, D), 42 + N))
    kr, vr = kv.view(B, N, 2 * D)[..., :D], kv.view(B, N, 2 * D)[..., D:]
    r = torch_class_attention(q, kr, vr, do, H)
    got = class_attention(ops, q, kv, do, B, H, N, HD, dt)
    bound = FP32 if dt == f32 else VEC
    tag = f"class_attn.h{H}n{N}.{'fp32' if dt == f32 else 'bf16'}"
    check(f"{tag}.out", got[0], r[0], bound)
    check(f"{tag}.p", got[1].view(B, H, N), r[1], FP32)
    for nm, x, w in zip(("dq", "dk", "dv"), got[2:], r[2:]):
        check(f"{tag}.{nm}", x, w, bound)


def test_long_class_attention_deterministic_and_batch_invariant(ops):
    B, H, N = 3, 16, 785
    D = H * HD
    q, kv, do = bf16_round(gen((B, D), 50)), bf16_round(gen((B * N, 2 * D), 51)), bf16_round(gen((B, D), 52))
    a = class_attention(ops, q, kv, do, B, H, N, HD, bt)
    b = class_attention(ops, q, kv, do, B, H, N, HD, bt)
    for x, y in zip(a, b):
        assert same_bits(x, y)
    one = class_attention(ops, q[1:2], kv.view(B, N, 2 * D)[1], do[1:2], 1, H, N, HD, bt)
    for x, y in zip((a[0][1:2], a[2][1:2], a[3][1:2], a[4][1:2]), (one[0], one[2], one[3], one[4])):
        assert same_bits(x, y)


def test_class_attention_refuses_past_1025_tokens(ops):
    from vit_torch_amd._lib import VitmiError
    with pytest.raises(VitmiError, match="N <= 1025"):
        class_attention(ops, gen((1, 8 * HD), 1), gen((1026, 16 * HD), 2), gen((1, 8 * HD), 3), 1, 8, 1026, HD, f32)


# ------------------------------------------------------------------------------------------------- engine ---
LONG_ARCHS = ["cait_XXS24", "cait_XXS36", "cait_XS24", "cait_S24", "cait_S36", "cait_M36", "cait_M48"]


def zero_grad_param(n):
    return n.endswith("proj_l.bias") or (n.startswith("blocks_token_only") and n.endswith("attn.k.bias"))


def reduced_cfg(arch):
    from vit_torch_amd.cait import VARIANTS
    img, d, _, heads, _ = VARIANTS[arch]
    return img, dict(img_size=img, patch_size=16, embed_dim=d, depth=2, num_heads=heads, mlp_ratio=4, qkv_bias=True,
                     norm_layer=partial(nn.LayerNorm, eps=1e-6), init_scale=1e-1, depth_token_only=2, num_classes=10)


def make_pair(cfg, compute, residual="fp32"):
    from oracle.cait_ref import CaiT
    from oracle.vit_ref import seeded_init_
    from vit_torch_amd import cait_models
    ref = CaiT(**cfg)
    seeded_init_(ref, 3)
    with torch.no_grad():
        for n, p in ref.named_parameters():
            if "gamma_" in n:
                p.copy_(0.3 + 0.1 * torch.randn(p.shape, generator=torch.Generator("cpu").manual_seed(len(n))))
    m = cait_models(**cfg, compute_dtype=compute, residual_dtype=residual)
    res = m.load_state_dict(ref.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return ref, m.cuda()


def step(ref, m, B, S):
    from vit_torch_amd import CrossEntropyLoss
    g = torch.Generator("cpu").manual_seed(0)
    x, y = torch.randn(B, 3, S, S, generator=g), torch.randint(0, 10, (B,), generator=g)
    lo = ref(x)
    lr = nn.functional.cross_entropy(lo, y)
    ref.zero_grad()
    lr.backward()
    out = m(x.cuda())
    loss = CrossEntropyLoss()(out, y.cuda())
    m.zero_grad()
    loss.backward()
    return lo.detach(), lr.detach(), out.detach(), loss.detach()


@pytest.mark.parametrize("arch", LONG_ARCHS)
def test_reduced_depth_fp32_matches_oracle(arch):
    """The bounds of test_cait_gpu.py::test_cait_tiny_fp32_matches_oracle: logits 1e-4, every gradient 3e-4."""
    img, cfg = reduced_cfg(arch)
    ref, m = make_pair(cfg, "fp32")
    lo, lr, out, loss = step(ref, m, 2, img)
    e = assert_close(f"{arch} logits", out, lo, 1e-4)
    assert abs(loss.item() - lr.item()) < 1e-4
    worst = 0.0
    for (n, pr), (n2, pm) in zip(ref.named_parameters(), m.named_parameters()):
        assert n == n2
        if zero_grad_param(n):
            assert pm.grad.abs().max().item() < 1e-5
            continue
        worst = max(worst, assert_close(f"{arch} grad[{n}]", pm.grad, pr.grad, 3e-4))
    print(f"\n{arch} depth 2 fp32: logits rel err {e:.2e}, worst grad rel err {worst:.2e}")


@pytest.mark.parametrize("arch", LONG_ARCHS)
def test_reduced_depth_bf16_close_to_oracle(arch):
    """The bounds of test_cait_gpu.py::test_cait_tiny_bf16_close_to_oracle: logits 1e-2, loss 5e-3, grad norms 1.2e-2;
    and the bf16 trunk keeps no [B, H, N, N] tensor for the backward."""
    img, cfg = reduced_cfg(arch)
    ref, m = make_pair(cfg, "bf16")
    lo, lr, out, loss = step(ref, m, 2, img)
    e = assert_close(f"{arch} logits", out, lo, 1e-2)
    assert abs(loss.item() - lr.item()) < 5e-3
    worst = 0.0
    for (n, pr), (_, pm) in zip(ref.named_parameters(), m.named_parameters()):
        if zero_grad_param(n):
            continue
        gn_ref, gn = pr.grad.norm().item(), pm.grad.float().norm().item()
        rel = abs(gn - gn_ref) / max(gn_ref, 1e-12)
        worst = max(worst, rel)
        assert rel < 1.2e-2, f"{arch} grad-norm[{n}]: {gn:.4g} vs {gn_ref:.4g}"
    print(f"\n{arch} depth 2 bf16: logits rel err {e:.2e}, worst grad-norm rel err {worst:.2e}")


def test_bf16_long_path_saves_nothing_quadratic():
    _, cfg = reduced_cfg("cait_M48")
    _, m = make_pair(cfg, "bf16")
    x = torch.randn(2, 3, 448, 448, device="cuda")
    eng = m.engine()
    eng.forward(x, save=True)
    s = eng.saved
    assert s["th_mode"] == "long"
    B, Np, H = s["B"], s["Np"], s["H"]
    for layer in s["trunk"]:
        assert layer[5] is None and layer[6] is None and layer[7] is None, "S / P / P' kept for the backward"
        for t in layer:
            if isinstance(t, torch.Tensor):
                assert t.numel() < B * H * Np * Np, f"a saved tensor of {tuple(t.shape)} is quadratic in N"
    eng.saved = None


@pytest.mark.parametrize("compute", ["bf16", "fp32", "bf16x3"])
@pytest.mark.parametrize("arch", LONG_ARCHS)
def test_long_arch_trains_a_step(arch, compute):
    """Forward, backward and an SGD step with a finite loss, and the loss of the next forward below the first."""
    from vit_torch_amd import CrossEntropyLoss, FusedSGD
    _, cfg = reduced_cfg(arch)
    _, m = make_pair(cfg, compute)
    g = torch.Generator("cpu").manual_seed(3)
    x = torch.randn(2, 3, cfg["img_size"], cfg["img_size"], generator=g).cuda()
    y = torch.randint(0, 10, (2,), generator=g).cuda()
    opt = FusedSGD(m.parameters(), lr=1e-2)
    crit = CrossEntropyLoss()
    losses = []
    for _ in range(2):
        opt.zero_grad()
        loss = crit(m(x), y)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert all(torch.isfinite(torch.tensor(losses))), losses
    assert losses[1] < losses[0], losses


def test_graphed_step_matches_eager_on_the_long_path(lib):
    from vit_torch_amd import CrossEntropyLoss, FusedSGD
    from vit_torch_amd.graph import GraphedStep
    _, cfg = reduced_cfg("cait_S24")                 # cait_S24's attention: D = 384, 8 heads, 576 tokens; depth 2
    g = torch.Generator("cpu").manual_seed(1)
    data = [(torch.randn(2, 3, 384, 384, generator=g).cuda(), torch.randint(0, 10, (2,), generator=g).cuda())
            for _ in range(3)]

    def make():
        _, m = make_pair(cfg, "bf16", "auto")
        return m, CrossEntropyLoss(), FusedSGD(m.parameters(), lr=5e-2, momentum=0.9)

    m, crit, opt = make()
    eager = []
    for x, y in data:
        opt.zero_grad()
        loss = crit(m(x), y)
        loss.backward()
        opt.step()
        eager.append(loss.item())
    p_eager = m.engine().pack.flat.clone()
    m2, crit2, opt2 = make()
    start = m2.engine().pack.flat.clone()
    st = GraphedStep(m2, crit2, opt2, *data[0], warmup=1)
    with torch.no_grad():
        m2.engine().pack.flat.copy_(start)
    opt2.reset_state()
    graphed = [st(x, y).item() for x, y in data]
    assert graphed == pytest.approx(eager, rel=1e-5, abs=1e-6), (graphed, eager)
    torch.testing.assert_close(m2.engine().pack.flat, p_eager, rtol=1e-5, atol=1e-6)
    st.close()


def test_cait_s24_384_full_size_fp32_logits_within_1e3():
    """cait_S24 at 384 x 384, batch 2, parity mode (as test_cait_gpu.py does for cait_S24_224)."""
    from oracle import cait_ref
    from oracle.vit_ref import seeded_init_
    from vit_torch_amd import VisionModelZoo
    ref = cait_ref.build("cait_S24", num_classes=10)
    seeded_init_(ref, 5)
    with torch.no_grad():
        for n, p in ref.named_parameters():
            if "gamma_" in n:
                p.fill_(0.1)
    m = VisionModelZoo.get_model("cait_S24", pretrained=False, classifier=None, compute_dtype="fp32")
    m.head = nn.Linear(384, 10)
    m.load_state_dict(ref.state_dict(), strict=True)
    m = m.cuda()
    lo, lr, out, loss = step(ref, m, 2, 384)
    e = assert_close("cait_S24 logits", out, lo, 1e-3)
    assert abs(loss.item() - lr.item()) < 1e-3
    print(f"\ncait_S24 (384) fp32: logits rel err {e:.2e}, loss diff {abs(loss.item() - lr.item()):.2e}")


# ------------------------------------------------------------------- fixtures of the reference's own classes ---
def _fixture(name):
    import os
    from fixture_codec import load
    return load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz"))


# Against the fixtures each result is compared whole, or (over 4096 entries) as a fixed sample plus its row sums
# (tests/fixture_codec.py).  fp32: FIX_FP32 = 1e-4, the window-12 fixture tests' bound [6.6e-6].  bf16 talking heads:
# the attention's operands are rounded to bf16 and S, P, P' are stored in bf16; a row sum (of y, or of a weight gradient)
# adds up the bf16 errors of O, which within one head share the rounding of the same P' row, while the signal partly
# cancels [y 2.1e-2, proj.weight 2.8e-2]: FIX_BF16 = 6e-2.  bf16 class attention: one rounding of q, k, v and of the
# stored results [6.3e-3]: FIX_CA_BF16 = 1.5e-2.
FIX_FP32, FIX_BF16, FIX_CA_BF16 = 1e-4, 6e-2, 1.5e-2


def fixture_err(got, want):
    """the error fixture_codec.check bounds: rel-to-max over the whole result, or the worse of sample and row sums"""
    from fixture_codec import Compact
    g = got.detach().float().cpu()
    if not isinstance(want, Compact):
        return rel_err(g, want)
    return max(rel_err(g.reshape(-1)[::want.stride], want.sample), rel_err(g.double().sum(-1).float(), want.rows))


def fixture_checks(tag, pairs, tol):
    """every error printed before any is asserted"""
    errs = {k: fixture_err(g, w) for k, (g, w) in pairs.items()}
    print(f"\n  {tag}: " + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()) + f" (bound {tol:.1e})", end="")
    for k, (g, w) in pairs.items():
        assert torch.isfinite(g.detach().float()).all(), f"{tag}.{k}: non-finite values"
        assert errs[k] <= tol, f"{tag}.{k}: error {errs[k]:.3e} > {tol:.1e}"


@pytest.mark.parametrize("dt", [f32, bt], ids=["fp32", "bf16"])
def test_talking_heads_576_fixture(ops, dt):
    """The reference's Attention_talking_head over 576 tokens (tests/golden/talking_heads_576.npz) through the kernels
    the engine runs at that shape (bf16: the long op; fp32: the three-call form).  The two Linears around the attention
    are plain fp32 matrix products here: what is under test is the attention and its four mixing-parameter gradients."""
    from fixture_codec import group
    f = _fixture("talking_heads_576")
    st = {k: v.cuda() for k, v in group(f, "state").items()}
    H, N = 8, 576
    D = H * HD
    x, dy = f["x"][0].cuda(), f["dy"][0].cuda()
    qkv = (x @ st["qkv.weight"].t() + st["qkv.bias"]).view(1, N, 3, H, HD).cpu()
    dO = (dy @ st["proj.weight"]).view(1, N, H, HD).cpu()
    W = [st[k].cpu() for k in ("proj_l.weight", "proj_l.bias", "proj_w.weight", "proj_w.bias")]
    O, dqkv, gr = th_run(ops, qkv, dO, W, dt)
    O, dqkv = O.float().view(N, D), dqkv.float().view(N, 3 * D)
    want = group(f, "grad")
    fixture_checks("talking_heads_576." + ("fp32" if dt == f32 else "bf16"), {
        "y": ((O @ st["proj.weight"].t() + st["proj.bias"]).view(1, N, D), f["y"]),
        "dx": ((dqkv @ st["qkv.weight"]).view(1, N, D), f["dx"]),
        "qkv.weight": (dqkv.t() @ x, want["qkv.weight"]),
        "qkv.bias": (dqkv.sum(0), want["qkv.bias"]),
        "proj.weight": (dy.t() @ O, want["proj.weight"]),
        "proj_l.weight": (gr[0], want["proj_l.weight"]),
        "proj_w.weight": (gr[2], want["proj_w.weight"]),
        "proj_w.bias": (gr[3], want["proj_w.bias"])}, FIX_FP32 if dt == f32 else FIX_BF16)


@pytest.mark.parametrize("dt", [f32, bt], ids=["fp32", "bf16"])
def test_class_attention_577_fixture(ops, dt):
    """The reference's Class_Attention over 577 tokens, two images (tests/golden/class_attention_577.npz), through
    class_attn_fwd / _bwd; q, k, v and the output projection are fp32 products here."""
    from fixture_codec import group
    f = _fixture("class_attention_577")
    st = {k: v.cuda() for k, v in group(f, "state").items()}
    H, N, B = 8, 577, 2
    D = H * HD
    x, dy = f["x"].cuda(), f["dy"].cuda().view(B, D)
    xf = x.reshape(B * N, D)
    lin = lambda t, n: t @ st[n + ".weight"].t() + st[n + ".bias"]
    q, k, v = (lin(x[:, 0], "q").to(dt).contiguous(), lin(xf, "k").to(dt).contiguous(), lin(xf, "v").to(dt).contiguous())
    out, ps = nan((B, D), dt), nan((B * H * N,), f32)
    ops.class_attn_fwd(q, k, v, D, out, ps, B, H, N, HD, HD ** -0.5)
    dout = (dy @ st["proj.weight"]).to(dt).contiguous()
    dq, dk, dv = nan((B, D), dt), nan((B * N, D), dt), nan((B * N, D), dt)
    ops.class_attn_bwd(q, k, v, D, dout, ps, dq, dk, dv, D, B, H, N, HD, HD ** -0.5)
    torch.cuda.synchronize()
    out, dq, dk, dv = out.float(), dq.float(), dk.float(), dv.float()
    dx = (dk @ st["k.weight"] + dv @ st["v.weight"]).view(B, N, D)
    dx[:, 0] += dq @ st["q.weight"]
    want = group(f, "grad")
    fixture_checks("class_attention_577." + ("fp32" if dt == f32 else "bf16"), {
        "y": (lin(out, "proj").view(B, 1, D), f["y"]),
        "dx": (dx, f["dx"]),
        "q.weight": (dq.t() @ x[:, 0], want["q.weight"]),
        "v.weight": (dv.t() @ xf, want["v.weight"]),
        "k.weight": (dk.t() @ xf, want["k.weight"]),
        "proj.weight": (dy.t() @ out, want["proj.weight"])}, FIX_FP32 if dt == f32 else FIX_CA_BF16)
