"""Float64 restatement of XCiT's XCABlock (the reference's models/xcit.py:264-292, with its XCA :243-254, Mlp and LPI
:132-141 inside) for the kernel and module tests, the closed-form forward / backward the module runs, the float32 closed
form, the float64 emulation with the roundings the "bf16" path declares, and a float64 reference of the junction kernel
(ops.ls_residual_ln_fwd, csrc/layernorm.hip) alone.  Neither touches the library nor the reference tree;
tests/golden/xcab.npz pins it to the reference's class.

    x1 = x + g1 (xca(LN1(x) Wqkv^T + bqkv) Wp^T + bp)
    x2 = x1 + g3 lpi(LN3(x1), H, W)
    out = x2 + g2 (gelu(LN2(x2) W1^T + b1) W2^T + b2)

Declared roundings of compute_dtype "bf16" (everything else is fp32; the emulation carries them in float64 arithmetic):
the weight shadows of qkv, proj, fc1, fc2; the stored activations l1, qkv, the attention output, f1 = proj(...) (kept for
dgamma1; x1 itself is formed from the fp32 accumulator), l3, the LPI's u and output p, l2, gelu'(pre), the hidden rows, f2 (as
f1); the stored gradients gm = g2 G, dH, dl2, gp = g3 G1, dl3 (the LPI's dx), ga = g1 G2, datt, dqkv, dl1; and what the XCA and
LPI kernels round inside (xca_util.emulated_xca, lpi_util.emulated_lpi).  The bias gradients of fc2 and proj are column sums
of the stored gm and ga."""
import functools

import torch
import torch.nn.functional as F

from lpi_util import EPS as BN_EPS, MOMENTUM, emulated_lpi
from vit_attn_util import bf16, gen, rel  # noqa: F401
from xca_util import emulated_xca
from xcit_ca_util import _dgelu, _ln_bwd, _ln_fwd

EPS = 1e-6
LPI_PARAMS = ("conv1.weight", "conv1.bias", "bn.weight", "bn.bias", "conv2.weight", "conv2.bias")
PARAM_KEYS = ("gamma1", "gamma2", "gamma3", "norm1.weight", "norm1.bias", "attn.temperature", "attn.qkv.weight", "attn.qkv.bias",
              "attn.proj.weight", "attn.proj.bias", "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias",
              "mlp.fc2.weight", "mlp.fc2.bias", "norm3.weight", "norm3.bias") + tuple("local_mp." + k for k in LPI_PARAMS)
BUF_KEYS = ("local_mp.bn.running_mean", "local_mp.bn.running_var", "local_mp.bn.num_batches_tracked")
STATE_KEYS = PARAM_KEYS[:-2] + BUF_KEYS + PARAM_KEYS[-2:]                       # the reference's state-dict order
TRAIN_KEYS = ("out", "dx") + tuple("grad/" + k for k in PARAM_KEYS) + tuple("buf/" + k for k in BUF_KEYS[:2])
KEYS = TRAIN_KEYS + ("out_eval",)                                               # what a bound is frozen for


def torch_block(x, dy, st, heads, Hg, Wg, training=True, eps=EPS, dtype=torch.float64):
    """The reference's lines under autograd in `dtype` on the CPU: {"out", "dx", "grad/<param>", "buf/<buffer>"} (the
    buffers after the forward; unchanged in eval mode)."""
    B, N, D = x.shape
    hd = D // heads
    xg = x.to(dtype).clone().requires_grad_(True)
    p = {k: st[k].to(dtype).clone().requires_grad_(True) for k in PARAM_KEYS}
    rm, rv = st[BUF_KEYS[0]].to(dtype).clone(), st[BUF_KEYS[1]].to(dtype).clone()
    # x + gamma1 * attn(norm1(x))
    l1 = F.layer_norm(xg, (D,), p["norm1.weight"], p["norm1.bias"], eps)
    qkv = (l1 @ p["attn.qkv.weight"].t() + p["attn.qkv.bias"]).reshape(B, N, 3, heads, hd).permute(2, 0, 3, 1, 4)
    q, k, v = (t.transpose(-2, -1) for t in (qkv[0], qkv[1], qkv[2]))
    attn = (F.normalize(q, dim=-1) @ F.normalize(k, dim=-1).transpose(-2, -1)) * p["attn.temperature"]
    a = (attn.softmax(dim=-1) @ v).permute(0, 3, 1, 2).reshape(B, N, D)
    x1 = xg + p["gamma1"] * (a @ p["attn.proj.weight"].t() + p["attn.proj.bias"])
    # x + gamma3 * local_mp(norm3(x), H, W)
    l3 = F.layer_norm(x1, (D,), p["norm3.weight"], p["norm3.bias"], eps)
    g = l3.permute(0, 2, 1).reshape(B, D, Hg, Wg)
    g = F.gelu(F.conv2d(g, p["local_mp.conv1.weight"], p["local_mp.conv1.bias"], padding=1, groups=D))
    g = F.batch_norm(g, rm, rv, p["local_mp.bn.weight"], p["local_mp.bn.bias"], training, MOMENTUM, BN_EPS)
    g = F.conv2d(g, p["local_mp.conv2.weight"], p["local_mp.conv2.bias"], padding=1, groups=D)
    x2 = x1 + p["gamma3"] * g.reshape(B, D, N).permute(0, 2, 1)
    # x + gamma2 * mlp(norm2(x))
    l2 = F.layer_norm(x2, (D,), p["norm2.weight"], p["norm2.bias"], eps)
    out = x2 + p["gamma2"] * (F.gelu(l2 @ p["mlp.fc1.weight"].t() + p["mlp.fc1.bias"]) @ p["mlp.fc2.weight"].t() + p["mlp.fc2.bias"])
    out.backward(dy.to(dtype))
    nbt = st[BUF_KEYS[2]].clone() + (1 if training else 0)
    return {"out": out.detach(), "dx": xg.grad, **{"grad/" + k_: t.grad for k_, t in p.items()},
            "buf/" + BUF_KEYS[0]: rm, "buf/" + BUF_KEYS[1]: rv, "buf/" + BUF_KEYS[2]: nbt}


def _lpi_state(st, dtype):
    return {k[len("local_mp."):]: st[k].to(dtype) if st[k].is_floating_point() else st[k] for k in STATE_KEYS if k.startswith("local_mp.")}


def closed_block(x, dy, st, heads, Hg, Wg, training=True, eps=EPS, dtype=torch.float64, emulate=False):
    """The module's own forward and backward, step by step, in `dtype` (float32: the float32 closed form).  emulate: the
    declared bf16 roundings (docstring) in otherwise-`dtype` arithmetic."""
    r = bf16 if emulate else (lambda t: t)
    B, N, D = x.shape
    M, hd = B * N, D // heads
    xf, G = x.to(dtype).reshape(M, D), dy.to(dtype).reshape(M, D)
    p = {k: st[k].to(dtype) for k in PARAM_KEYS}
    Wqkv, Wp, W1, W2 = (r(p[k]) for k in ("attn.qkv.weight", "attn.proj.weight", "mlp.fc1.weight", "mlp.fc2.weight"))
    g1, g2, g3, temp = p["gamma1"], p["gamma2"], p["gamma3"], p["attn.temperature"].reshape(heads)
    lst = _lpi_state(st, dtype)
    xca = lambda qkv_, do_: emulated_xca(qkv_.reshape(B, N, 3 * D), do_.reshape(B, N, D), temp, B, N, heads, hd, dtype=dtype,  # noqa: E731
                                         rounding=emulate)
    lpi = lambda l_, d_: emulated_lpi(l_.reshape(B, N, D), d_.reshape(B, N, D), lst, B, Hg, Wg, training=training, dtype=dtype,  # noqa: E731
                                      rounding=emulate)
    # forward
    l1, mean1, rstd1 = _ln_fwd(xf, p["norm1.weight"], p["norm1.bias"], eps)
    l1 = r(l1)
    qkv = r(l1 @ Wqkv.t() + p["attn.qkv.bias"])
    att = xca(qkv, torch.zeros_like(xf)).out.reshape(M, D)
    f1 = att @ Wp.t() + p["attn.proj.bias"]
    x1 = xf + g1 * f1
    l3, mean3, rstd3 = _ln_fwd(x1, p["norm3.weight"], p["norm3.bias"], eps)
    l3 = r(l3)
    lf = lpi(l3, torch.zeros_like(xf))
    pp = lf.out.reshape(M, D)
    x2 = x1 + g3 * pp
    l2, mean2, rstd2 = _ln_fwd(x2, p["norm2.weight"], p["norm2.bias"], eps)
    l2 = r(l2)
    pre = l2 @ W1.t() + p["mlp.fc1.bias"]
    hid, dg = r(F.gelu(pre)), r(_dgelu(pre))                             # "bf16" keeps gelu'(pre); "fp32" the pre-activation
    f2 = hid @ W2.t() + p["mlp.fc2.bias"]
    out = x2 + g2 * f2
    # backward
    gr = {}
    gr["gamma2"] = (G * r(f2)).sum(0)
    gm = r(g2 * G)
    gr["mlp.fc2.weight"], gr["mlp.fc2.bias"] = gm.t() @ hid, gm.sum(0)
    dH = r((gm @ W2) * dg)
    gr["mlp.fc1.weight"], gr["mlp.fc1.bias"] = dH.t() @ l2, dH.sum(0)
    dxl, gr["norm2.weight"], gr["norm2.bias"] = _ln_bwd(r(dH @ W1), x2, mean2, rstd2, p["norm2.weight"])
    G1 = G + dxl
    gr["gamma3"] = (G1 * pp).sum(0)
    lb = lpi(l3, r(g3 * G1))
    for k in LPI_PARAMS:
        gr["local_mp." + k] = lb.grads[k]
    dxl, gr["norm3.weight"], gr["norm3.bias"] = _ln_bwd(lb.dx.reshape(M, D), x1, mean3, rstd3, p["norm3.weight"])
    G2 = G1 + dxl
    gr["gamma1"] = (G2 * r(f1)).sum(0)
    ga = r(g1 * G2)
    gr["attn.proj.weight"], gr["attn.proj.bias"] = ga.t() @ att, ga.sum(0)
    xb = xca(qkv, r(ga @ Wp))
    dqkv = xb.dqkv.reshape(M, 3 * D)
    gr["attn.temperature"] = xb.dtemp.reshape(heads, 1, 1)
    gr["attn.qkv.weight"], gr["attn.qkv.bias"] = dqkv.t() @ l1, dqkv.sum(0)
    dxl, gr["norm1.weight"], gr["norm1.bias"] = _ln_bwd(r(dqkv @ Wqkv), xf, mean1, rstd1, p["norm1.weight"])
    nbt = st[BUF_KEYS[2]].clone() + (1 if training else 0)
    return {"out": out.reshape(B, N, D), "dx": (G2 + dxl).reshape(B, N, D), **{"grad/" + k: v for k, v in gr.items()},
            "buf/" + BUF_KEYS[0]: lf.running_mean, "buf/" + BUF_KEYS[1]: lf.running_var, "buf/" + BUF_KEYS[2]: nbt}


def with_eval(fn, x, dy, st, heads, Hg, Wg, **k):
    """fn's train-mode result plus "out_eval": fn's eval-mode output on the buffers its own train-mode forward left"""
    res = fn(x, dy, st, heads, Hg, Wg, training=True, **k)
    st2 = dict(st)
    for b in BUF_KEYS[:2]:
        st2[b] = res["buf/" + b]
    res["out_eval"] = fn(x, dy, st2, heads, Hg, Wg, training=False, **k)["out"]
    return res


def errors(got, want, keys=KEYS):
    return {k: rel(got[k], want[k]) for k in keys}


def make_state(D, heads, mlp_ratio, seed, eta=0.5):
    """a seeded state with non-trivial norms, gammas (neither 1 nor all equal), temperature and running buffers; Linear
    weights ~ fan_in^-1/2, conv taps ~ N(0, 0.3)"""
    Dh = int(D * mlp_ratio)
    shapes = {"gamma1": (D,), "gamma2": (D,), "gamma3": (D,), "norm1.weight": (D,), "norm1.bias": (D,),
              "attn.temperature": (heads, 1, 1), "attn.qkv.weight": (3 * D, D), "attn.qkv.bias": (3 * D,),
              "attn.proj.weight": (D, D), "attn.proj.bias": (D,), "norm2.weight": (D,), "norm2.bias": (D,),
              "mlp.fc1.weight": (Dh, D), "mlp.fc1.bias": (Dh,), "mlp.fc2.weight": (D, Dh), "mlp.fc2.bias": (D,),
              "norm3.weight": (D,), "norm3.bias": (D,), "local_mp.conv1.weight": (D, 1, 3, 3), "local_mp.conv1.bias": (D,),
              "local_mp.bn.weight": (D,), "local_mp.bn.bias": (D,), "local_mp.bn.running_mean": (D,),
              "local_mp.bn.running_var": (D,), "local_mp.conv2.weight": (D, 1, 3, 3), "local_mp.conv2.bias": (D,)}
    st = {}
    for i, (k, s) in enumerate(shapes.items()):
        t = gen(s, seed + i)
        if k.startswith("gamma"):
            st[k] = eta + 0.2 * t.clamp(-2, 2)
        elif k.endswith("temperature"):
            st[k] = 1.25 + 0.5 * t.clamp(-1, 1)
        elif k.endswith("running_var"):
            st[k] = 0.5 + t.abs()
        elif k.endswith("running_mean"):
            st[k] = 0.2 * t
        elif k.endswith("weight") and len(s) == 1:
            st[k] = 1 + 0.3 * t.clamp(-2.5, 2.5)
        elif len(s) == 2:
            st[k] = t * s[1] ** -0.5
        elif len(s) == 4:
            st[k] = 0.3 * t
        else:
            st[k] = 0.2 * t
    st["local_mp.bn.num_batches_tracked"] = torch.tensor(5)
    return {k: st[k] for k in STATE_KEYS}


# (B, H, W, dim, heads): head dims 32, 48, 64, 48; a two-token grid, odd grids, the 14 x 14 grid of the 224-pixel models
MODULE_CASES = ((2, 1, 2, 64, 2), (2, 3, 5, 96, 2), (3, 7, 9, 128, 2), (2, 14, 14, 192, 4))
MLP_RATIO = 2.0


def case_name(c):
    return "B%d-%dx%d-D%d-h%d" % c


CASE_NAMES = tuple(case_name(c) for c in MODULE_CASES)


@functools.lru_cache(maxsize=None)
def module_case(name):
    """(x, dy, state, heads, H, W) of a MODULE_CASES entry; the inputs are bf16-representable so that both compute dtypes see them"""
    i = CASE_NAMES.index(name)
    B, Hg, Wg, D, heads = MODULE_CASES[i]
    return (bf16(gen((B, Hg * Wg, D), 5000 + 10 * i)), bf16(gen((B, Hg * Wg, D), 5001 + 10 * i)),
            make_state(D, heads, MLP_RATIO, 5100 + 100 * i), heads, Hg, Wg)


@functools.lru_cache(maxsize=None)
def module_reference(name):
    """the float64 reference of a module case, train mode plus "out_eval" (with_eval); computed once, never modified"""
    return with_eval(torch_block, *module_case(name))


def fixture_case(fx):
    """(x, dy, state, heads, H, W, want) of tests/golden/xcab.npz; want holds the reference class's float32 results"""
    import fixture_codec as FC
    st = FC.group(fx, "state")
    st = {k: st[k].reshape(()) if k == BUF_KEYS[2] else st[k] for k in STATE_KEYS}
    want = {"out": fx["out"], "dx": fx["dx"], "out_eval": fx["out_eval"], **{"grad/" + k: fx["grad/" + k] for k in PARAM_KEYS},
            **{"buf/" + k: fx["after/" + k] for k in BUF_KEYS}}
    Hg, Wg = (int(v) for v in fx["grid"])
    return fx["x"], fx["dy"], st, int(fx["heads"]), Hg, Wg, want


def fixture_errors(got, want):
    """errors against fixture entries: whole tensors, or the sample and the row sums of a sampled one (the worse of the two)"""
    import fixture_codec as FC
    e = {}
    for k, w in want.items():
        g = got[k].detach().float().cpu()
        if isinstance(w, FC.Compact):
            e[k] = max(rel(g.reshape(-1)[::w.stride], w.sample), rel(g.double().sum(-1).float(), w.rows))
        else:
            e[k] = rel(g.reshape(w.shape), w)
    return e


def measure(x, dy, st, heads, Hg, Wg, ref=None):
    """(float32 closed form's error, bf16 emulation's error) against float64 on the same inputs, per tensor of KEYS"""
    ref = ref or with_eval(torch_block, x, dy, st, heads, Hg, Wg)
    return (errors(with_eval(closed_block, x, dy, st, heads, Hg, Wg, dtype=torch.float32), ref),
            errors(with_eval(closed_block, x, dy, st, heads, Hg, Wg, emulate=True), ref))


# ---- the junction kernel on its own: y = x + gamma * b, l = LayerNorm(y)
KERNEL_D = (8, 64, 72, 136, 192, 384, 392, 512, 768, 1032, 2048)    # every lane-group width and chunk count, a row that does
KERNEL_M = (1, 3, 5, 67)                                            # not fill its lane group, the upper limit; rows per wave never divide M
KERNEL_KEYS = ("y", "l", "mean", "rstd")


@functools.lru_cache(maxsize=None)
def kernel_inputs(M, D, offset=0.25):
    """x fp32 = offset + N(0, 1) (a row mean away from zero keeps `mean` well conditioned), a bf16-representable b, gamma, and
    a non-trivial norm weight / bias"""
    s = 9000 + 10 * D + M
    return {"x": offset + gen((M, D), s), "b": bf16(gen((M, D), s + 1)), "gamma": 0.5 + 0.2 * gen((D,), s + 2).clamp(-2, 2),
            "w": 1 + 0.3 * gen((D,), s + 3).clamp(-2.5, 2.5), "bias": 0.2 * gen((D,), s + 4)}


def kernel_reference(t, eps=EPS, dtype=torch.float64, emulate=False):
    """{"y", "l", "mean", "rstd"} in `dtype`; emulate rounds l, the one output in the branch dtype"""
    x, b, gamma, w, bias = (t[k].to(dtype) for k in ("x", "b", "gamma", "w", "bias"))
    y = x + gamma * b
    l, mean, rstd = _ln_fwd(y, w, bias, eps)
    return {"y": y, "l": bf16(l) if emulate else l, "mean": mean.squeeze(-1), "rstd": rstd.squeeze(-1)}


def kernel_measure(D, offset=0.25, Ms=KERNEL_M):
    """the worst (float32, bf16-emulation) errors over the M of KERNEL_M at one D, per output"""
    f32, emu = dict.fromkeys(KERNEL_KEYS, 0.0), dict.fromkeys(KERNEL_KEYS, 0.0)
    for M in Ms:
        t = kernel_inputs(M, D, offset)
        ref = kernel_reference(t)
        for acc, got in ((f32, kernel_reference(t, dtype=torch.float32)), (emu, kernel_reference(t, emulate=True))):
            for k in KERNEL_KEYS:
                acc[k] = max(acc[k], rel(got[k], ref[k]))
    return f32, emu
