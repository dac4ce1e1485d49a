"""Float64 restatement of XCiT's class-attention block (the reference's models/xcit.py:144-218) for the kernel and module
tests, the closed-form backward the module runs, the float32 closed form, and the float64 emulation with the roundings the
"bf16" path declares.  Neither touches the library nor the reference tree; tests/golden/xcit_ca.npz pins it to the
reference's class.

With c the CLS row and p the patch rows of x [B, N1, D]:
    l = LN1(x);  q = l_c Wq^T + bq;  [k v] = l Wkv^T + bkv;  o = softmax(scale q k^T) v per head;  a = o Wp^T + bp
    x1_c = x_c + g1 a, x1_p = x_p + g1 l_p;  x2 = LN2(x1) (tokens_norm) or x2_c = LN2(x1_c), x2_p = x1_p
    m = fc2(gelu(fc1(x2_c)));  out_c = x2_c + g2 m, out_p = 2 x2_p

Declared roundings of compute_dtype "bf16" (everything else is fp32; the emulation carries them in float64 arithmetic):
the weight shadows of qkv, proj, fc1, fc2; the stored activations l, [k v], q, o, a, the MLP's operand x2_c, gelu'(pre), the
hidden row and m; the stored operand-dtype gradients gm = g2 G_c, dH, da, do, dq, dk, dv."""
import functools

import torch
import torch.nn.functional as F

from vit_attn_util import bf16, gen, rel  # noqa: F401

EPS = 1e-6
PARAM_KEYS = ("gamma1", "gamma2", "norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight",
              "attn.proj.bias", "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias")
KEYS = ("out", "dx") + tuple("grad/" + k for k in PARAM_KEYS)


def torch_block(x, dy, st, H, tokens_norm, eps=EPS, scale=None, dtype=torch.float64):
    """The block's forward as stated above under autograd in `dtype`: {"out", "dx", "grad/<param>"}"""
    B, N1, D = x.shape
    hd = D // H
    scale = scale or hd ** -0.5
    xg = x.to(dtype).clone().requires_grad_(True)
    p = {k: st[k].to(dtype).clone().requires_grad_(True) for k in PARAM_KEYS}
    l = F.layer_norm(xg, (D,), p["norm1.weight"], p["norm1.bias"], eps)
    Wqkv, bqkv = p["attn.qkv.weight"], p["attn.qkv.bias"]
    q = (l[:, 0] @ Wqkv[:D].t() + bqkv[:D]).view(B, H, 1, hd)
    kv = l @ Wqkv[D:].t() + bqkv[D:]
    k, v = (t.view(B, N1, H, hd).permute(0, 2, 1, 3) for t in (kv[..., :D], kv[..., D:]))
    att = ((q * k).sum(-1) * scale).softmax(-1)                                   # [B, H, N1]
    o = (att.unsqueeze(2) @ v).transpose(1, 2).reshape(B, D)
    a = o @ p["attn.proj.weight"].t() + p["attn.proj.bias"]
    x1 = xg + p["gamma1"] * torch.cat([a.unsqueeze(1), l[:, 1:]], dim=1)
    if tokens_norm:
        x2 = F.layer_norm(x1, (D,), p["norm2.weight"], p["norm2.bias"], eps)
    else:
        x2 = torch.cat([F.layer_norm(x1[:, :1], (D,), p["norm2.weight"], p["norm2.bias"], eps), x1[:, 1:]], dim=1)
    m = F.gelu(x2[:, 0] @ p["mlp.fc1.weight"].t() + p["mlp.fc1.bias"]) @ p["mlp.fc2.weight"].t() + p["mlp.fc2.bias"]
    out = x2 + torch.cat([(p["gamma2"] * m).unsqueeze(1), x2[:, 1:]], dim=1)
    out.backward(dy.to(dtype))
    return {"out": out.detach(), "dx": xg.grad, **{"grad/" + k: t.grad for k, t in p.items()}}


def _ln_fwd(x, w, b, eps):
    mean = x.mean(-1, keepdim=True)
    rstd = (x.var(-1, unbiased=False, keepdim=True) + eps).rsqrt()
    return (x - mean) * rstd * w + b, mean, rstd


def _ln_bwd(dy, x, mean, rstd, w):
    """dx, dgamma, dbeta"""
    xh = (x - mean) * rstd
    g = dy * w
    dx = rstd * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    flat = lambda t: t.reshape(-1, t.shape[-1])      # noqa: E731
    return dx, flat(dy * xh).sum(0), flat(dy).sum(0)


def _dgelu(t):
    return 0.5 * (1 + torch.erf(t * 2 ** -0.5)) + t * torch.exp(-0.5 * t * t) * (2 * torch.pi) ** -0.5


def closed_block(x, dy, st, H, tokens_norm, eps=EPS, scale=None, dtype=torch.float64, emulate=False):
    """The module's own forward and backward, step by step, in `dtype` (float32: the float32 closed form).  emulate: the
    declared bf16 roundings (docstring) in otherwise-`dtype` arithmetic."""
    r = bf16 if emulate else (lambda t: t)
    B, N1, D = x.shape
    hd = D // H
    scale = scale or hd ** -0.5
    x, G = x.to(dtype), dy.to(dtype)
    p = {k: st[k].to(dtype) for k in PARAM_KEYS}
    Wqkv, Wp, W1, W2 = (r(p[k]) for k in ("attn.qkv.weight", "attn.proj.weight", "mlp.fc1.weight", "mlp.fc2.weight"))
    bqkv, g1, g2 = p["attn.qkv.bias"], p["gamma1"], p["gamma2"]
    heads = lambda t: t.reshape(B, N1, H, hd).permute(0, 2, 1, 3)      # noqa: E731   [B, H, N1, hd]
    # forward
    l, mean1, rstd1 = _ln_fwd(x, p["norm1.weight"], p["norm1.bias"], eps)
    l = r(l)
    q = r(l[:, 0] @ Wqkv[:D].t() + bqkv[:D])
    kv = r(l @ Wqkv[D:].t() + bqkv[D:])
    k, v = heads(kv[..., :D]), heads(kv[..., D:])
    qh = q.view(B, H, 1, hd)
    P = ((qh * k).sum(-1) * scale).softmax(-1)                          # [B, H, N1]
    o = r((P.unsqueeze(2) @ v).reshape(B, D))
    a = r(o @ Wp.t() + p["attn.proj.bias"])
    x1 = x + g1 * torch.cat([a.unsqueeze(1), l[:, 1:]], dim=1)
    if tokens_norm:
        x2, mean2, rstd2 = _ln_fwd(x1, p["norm2.weight"], p["norm2.bias"], eps)
        x2c, x2p = x2[:, 0], x2[:, 1:]
    else:
        x2c, mean2, rstd2 = _ln_fwd(x1[:, 0], p["norm2.weight"], p["norm2.bias"], eps)
        x2p = x1[:, 1:]
    xc = r(x2c)
    pre = xc @ W1.t() + p["mlp.fc1.bias"]
    hid = r(F.gelu(pre))
    dg = r(_dgelu(pre))                                                  # "bf16" keeps gelu'(pre); "fp32" the pre-activation
    m = r(hid @ W2.t() + p["mlp.fc2.bias"])
    out = torch.cat([(x2c + g2 * m).unsqueeze(1), 2 * x2p], dim=1)
    # backward
    gr = {}
    Gc = G[:, 0]
    gr["gamma2"] = (Gc * m).sum(0)
    gm = r(g2 * Gc)
    dH = r((gm @ W2) * dg)
    gr["mlp.fc2.weight"], gr["mlp.fc2.bias"] = gm.t() @ hid, gm.sum(0)
    gr["mlp.fc1.weight"], gr["mlp.fc1.bias"] = dH.t() @ xc, dH.sum(0)
    dx2c = Gc + dH @ W1
    if tokens_norm:
        dx1, gr["norm2.weight"], gr["norm2.bias"] = _ln_bwd(torch.cat([dx2c.unsqueeze(1), 2 * G[:, 1:]], dim=1), x1, mean2, rstd2,
                                                            p["norm2.weight"])
    else:
        dx1c, gr["norm2.weight"], gr["norm2.bias"] = _ln_bwd(dx2c, x1[:, 0], mean2, rstd2, p["norm2.weight"])
        dx1 = torch.cat([dx1c.unsqueeze(1), 2 * G[:, 1:]], dim=1)
    gr["gamma1"] = (dx1[:, 0] * a).sum(0) + (dx1[:, 1:] * l[:, 1:]).sum((0, 1))
    da = r(g1 * dx1[:, 0])
    gr["attn.proj.weight"], gr["attn.proj.bias"] = da.t() @ o, da.sum(0)
    do = r(da @ Wp).view(B, H, hd)
    # class attention backward: one query per (image, head)
    dP = (do.unsqueeze(2) * v).sum(-1)                                   # [B, H, N1]
    dS = P * (dP - (P * dP).sum(-1, keepdim=True))
    dq = r((dS.unsqueeze(-1) * k).sum(2) * scale).reshape(B, D)
    dk = r(dS.unsqueeze(-1) * qh * scale)                                # [B, H, N1, hd]
    dv = r(P.unsqueeze(-1) * do.unsqueeze(2))
    dkv = torch.cat([t.permute(0, 2, 1, 3).reshape(B, N1, D) for t in (dk, dv)], dim=-1)
    gW = torch.cat([dq.t() @ l[:, 0], dkv.reshape(-1, 2 * D).t() @ l.reshape(-1, D)], dim=0)
    gr["attn.qkv.weight"], gr["attn.qkv.bias"] = gW, torch.cat([dq.sum(0), dkv.reshape(-1, 2 * D).sum(0)])
    dl = torch.cat([torch.zeros_like(dx1[:, :1]), g1 * dx1[:, 1:]], dim=1) + dkv @ Wqkv[D:]
    dl = torch.cat([(dl[:, 0] + dq @ Wqkv[:D]).unsqueeze(1), dl[:, 1:]], dim=1)
    dxl, gr["norm1.weight"], gr["norm1.bias"] = _ln_bwd(dl, x, mean1, rstd1, p["norm1.weight"])
    return {"out": out, "dx": dx1 + dxl, **{"grad/" + k: v_ for k, v_ in gr.items()}}


def errors(got, want, keys=KEYS):
    return {k: rel(got[k], want[k]) for k in keys}


def make_state(D, H, mlp_ratio, seed, eta=0.5):
    """a seeded state with non-trivial norms and gammas (neither 1 nor all equal); weights ~ fan_in^-1/2"""
    Dh = int(D * mlp_ratio)
    shapes = {"gamma1": (D,), "gamma2": (D,), "norm1.weight": (D,), "norm1.bias": (D,), "attn.qkv.weight": (3 * D, D),
              "attn.qkv.bias": (3 * D,), "attn.proj.weight": (D, D), "attn.proj.bias": (D,), "norm2.weight": (D,),
              "norm2.bias": (D,), "mlp.fc1.weight": (Dh, D), "mlp.fc1.bias": (Dh,), "mlp.fc2.weight": (D, Dh), "mlp.fc2.bias": (D,)}
    st = {}
    for i, (k, s) in enumerate(shapes.items()):
        t = gen(s, seed + i)
        if k.startswith("gamma"):
            st[k] = eta + 0.2 * t.clamp(-2, 2)
        elif k.endswith("norm1.weight") or k.endswith("norm2.weight"):
            st[k] = 1 + 0.3 * t.clamp(-2.5, 2.5)
        elif len(s) == 2:
            st[k] = t * s[1] ** -0.5
        else:
            st[k] = 0.2 * t
    return st


# (name, B, N1, D, H, mlp_ratio): the module's cases beside the fixture's
MODULE_CASES = (("single-patch", 2, 2, 64, 2, 2.0), ("n197-hd48", 2, 197, 96, 2, 2.0), ("n197-hd64", 2, 197, 128, 2, 2.0),
                ("n785-hd32", 2, 785, 64, 2, 2.0), ("wide", 64, 197, 192, 4, 4.0))


@functools.lru_cache(maxsize=None)
def module_case(name):
    """(x, dy, state, H) of a MODULE_CASES entry; the inputs are bf16-representable so that both compute dtypes see them"""
    i, (_, B, N1, D, H, ratio) = next((i, c) for i, c in enumerate(MODULE_CASES) if c[0] == name)
    return bf16(gen((B, N1, D), 4000 + 10 * i)), bf16(gen((B, N1, D), 4001 + 10 * i)), make_state(D, H, ratio, 4100 + 100 * i), H


@functools.lru_cache(maxsize=None)
def module_reference(name, tokens_norm):
    x, dy, st, H = module_case(name)
    return torch_block(x, dy, st, H, tokens_norm)


def fixture_case(fx, name):
    """(x, dy, state, H, tokens_norm, want) of one configuration of tests/golden/xcit_ca.npz"""
    import fixture_codec as FC
    d = FC.group(fx, name)
    st = FC.group(d, "state")
    want = {"out": d["out"], "dx": d["dx"], **{"grad/" + k: d["grad/" + k] for k in PARAM_KEYS}}
    return d["x"], d["dy"], st, int(d["heads"]), bool(int(d["tokens_norm"])), want


def fixture_errors(got, want):
    """errors against fixture entries: whole tensors, or the sample and the row sums of a sampled one (the worse of the two)"""
    import fixture_codec as FC
    e = {}
    for k, w in want.items():
        g = got[k].detach().float().cpu()
        if isinstance(w, FC.Compact):
            e[k] = max(rel(g.reshape(-1)[::w.stride], w.sample), rel(g.double().sum(-1).float(), w.rows))
        else:
            e[k] = rel(g, w)
    return e


def measure(x, dy, st, H, tokens_norm, ref=None):
    """(float32 closed form's error, bf16 emulation's error) against float64 on the same inputs, per tensor"""
    ref = ref or torch_block(x, dy, st, H, tokens_norm)
    return (errors(closed_block(x, dy, st, H, tokens_norm, dtype=torch.float32), ref),
            errors(closed_block(x, dy, st, H, tokens_norm, emulate=True), ref))


# ---- the glue kernels on their own
GLUE_SHAPES = tuple((B, N1, D) for N1 in (2, 7, 197) for D in (64, 192) for B in (1, 3))


@functools.lru_cache(maxsize=None)
def glue_inputs(B, N1, D):
    """fp32 residual-stream tensors, bf16-representable branch tensors, two gammas"""
    s = 7000 + 100 * B + 10 * N1 + D
    t = {"x": gen((B, N1, D), s), "G": gen((B, N1, D), s + 1), "l": bf16(gen((B, N1, D), s + 2)), "a": bf16(gen((B, D), s + 3)),
         "m": bf16(gen((B, D), s + 4)), "xc": gen((B, D), s + 5), "g1": 0.5 + 0.2 * gen((D,), s + 6).clamp(-2, 2),
         "g2": 0.5 + 0.2 * gen((D,), s + 7).clamp(-2, 2)}
    return t


def glue_reference(t, dtype=torch.float64, emulate=False):
    """the four kernels' outputs from glue_inputs in `dtype`; emulate rounds the operand-dtype outputs (da, gm)"""
    r = bf16 if emulate else (lambda v: v)
    x, G, l, a, m, xc, g1, g2 = (t[k].to(dtype) for k in ("x", "G", "l", "a", "m", "xc", "g1", "g2"))
    br = torch.cat([a.unsqueeze(1), l[:, 1:]], dim=1)
    out = {"x1": x + g1 * br,
           "da": r(g1 * G[:, 0]), "dl": torch.cat([torch.zeros_like(G[:, :1]), g1 * G[:, 1:]], dim=1), "dgamma1": (G * br).sum((0, 1)),
           "out": torch.cat([(xc + g2 * m).unsqueeze(1), 2 * x[:, 1:]], dim=1),
           "dx2": torch.cat([G[:, :1], 2 * G[:, 1:]], dim=1), "gm": r(g2 * G[:, 0])}
    return out


GLUE_KEYS = ("x1", "da", "dl", "dgamma1", "out", "dx2", "gm")


def glue_measure():
    """the worst (float32, bf16-emulation) errors over GLUE_SHAPES per output"""
    f32, emu = dict.fromkeys(GLUE_KEYS, 0.0), dict.fromkeys(GLUE_KEYS, 0.0)
    for shape in GLUE_SHAPES:
        t = glue_inputs(*shape)
        ref = glue_reference(t)
        for acc, got in ((f32, glue_reference(t, torch.float32)), (emu, glue_reference(t, emulate=True))):
            for k in GLUE_KEYS:
                acc[k] = max(acc[k], rel(got[k], ref[k]))
    return f32, emu
