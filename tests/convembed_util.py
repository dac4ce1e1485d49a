"""The plain-PyTorch ConvPatchEmbed (XCiT's stem, the reference's models/xcit.py:58-108) that the conv-stem kernel tests
compare against, and the closed form with the roundings the bf16 path declares.  Neither touches the library nor the
reference tree.

  torch_stem      the reference's lines (F.conv2d stride 2 padding 1, F.batch_norm, F.gelu) under autograd in `dtype`.
  closed_stem     the same mathematics the way the library computes it: F.unfold, a matrix product, the closed-form batch
                  norm backward, F.fold.  rounding=True applies exactly the declared bf16 roundings: the image on its way
                  into col, the weight shadows, y, out, dy, dcol and dx on store; dtype=float32, rounding=False is "the
                  float32 closed form" of the fp32 bounds; float64 without rounding equals autograd.
  torch_bn_act / closed_bn_act   the same pair for the bn_act op alone, over a GIVEN y [M, C]: the statistics are defined
                  over y as stored, so y is an operand (in bf16 the op's own stored y: straight-through by construction).
"""
from collections import namedtuple

import torch
import torch.nn.functional as F

from lpi_util import make_inputs as lpi_inputs  # noqa: F401
from vit_attn_util import bf16, gen, rel  # noqa: F401

MOMENTUM, EPS = 0.1, 1e-5
CHANS = {16: (8, 4, 2, 1), 8: (4, 2, 1)}


def stage_channels(patch, E):
    return [3] + [E // f for f in CHANS[patch]]


def param_keys(patch):
    ks = []
    for k in range(len(CHANS[patch])):
        ks += [f"proj.{2 * k}.0.weight", f"proj.{2 * k}.1.weight", f"proj.{2 * k}.1.bias"]
    return ks


def buffer_keys(patch):
    return [f"proj.{2 * k}.1.{n}" for k in range(len(CHANS[patch])) for n in ("running_mean", "running_var", "num_batches_tracked")]


# ------------------------------------------------------------------------------------------------ gathers ---
def out_grid(H, W):
    return (H + 1) // 2, (W + 1) // 2


def tok_to_grid(t, B, H, W):
    return t.reshape(B, H, W, -1).permute(0, 3, 1, 2)


def grid_to_tok(t):
    B, C, H, W = t.shape
    return t.permute(0, 2, 3, 1).reshape(B, H * W, C)


def unfold_cols(x_nchw):
    """[B*Ho*Wo, C*9], k = c*9 + i*3 + j: F.unfold's own order"""
    B, C = x_nchw.shape[:2]
    return F.unfold(x_nchw, 3, padding=1, stride=2).transpose(1, 2).reshape(-1, C * 9)


def fold_cols(dcol, B, H, W):
    """the transpose of unfold_cols: [B, C, H, W]"""
    Ho, Wo = out_grid(H, W)
    return F.fold(dcol.reshape(B, Ho * Wo, -1).transpose(1, 2), (H, W), 3, padding=1, stride=2)


def grid_values(shape, seed):
    """multiples of 1/8 in [-2, 2]: exact in bf16, and any sum of at most four of them is exact in bf16 and fp32"""
    g = torch.Generator("cpu").manual_seed(seed)
    return torch.randint(-16, 17, shape, generator=g).float() / 8


GATHER_GRIDS = ((1, 1), (2, 2), (3, 5), (5, 3), (4, 6), (7, 9), (14, 14), (16, 16))
GATHER_B = (1, 3)
GATHER_C = (8, 24, 48)

# ------------------------------------------------------------------------------------------------ bn + act ---
BnRef = namedtuple("BnRef", "out mean rstd dy dgamma dbeta running_mean running_var")
BN_ACT = ("out", "dy")
BN_F32 = ("mean", "rstd", "dgamma", "dbeta")
BN_M = (2, 3, 50, 257, 4100)
BN_C = (8, 24, 96, 192)


def bn_params(C, seed):
    """lpi_util.make_params' recipe for the norm: gamma = 1 +- 0.3, beta ~ N(0, 0.2), non-default running buffers"""
    return {"weight": 1 + gen((C,), seed + 2, 0.3).clamp(-0.9, 0.9), "bias": gen((C,), seed + 3, 0.2),
            "running_mean": gen((C,), seed + 4, 0.2), "running_var": 0.5 + gen((C,), seed + 5).abs(),
            "num_batches_tracked": torch.tensor(5)}


def bn_inputs(M, C, seed):
    """bf16-rounded unit-normal y and dout [M, C] (lpi_util.make_inputs' recipe)"""
    y, d = lpi_inputs(1, M, 1, C, seed)
    return y.reshape(M, C), d.reshape(M, C)


def bn_cases():
    return [(M, C, 1000 * C + M) for C in BN_C for M in BN_M]


def bn_stress(seed=4321):
    """M = 600, C = 16: channel 3 constant (M2 = 0 exactly), channel 5 with mean 8 and unit variance"""
    M, C = 600, 16
    y, d = bn_inputs(M, C, seed)
    y[:, 3] = 0.75
    y[:, 5] = bf16(y[:, 5] + 8)
    return bn_params(C, seed), y, d


def torch_bn_act(y, dout, p, gelu, training=True, dtype=torch.float64):
    yg = y.to(dtype).clone().requires_grad_(True)
    g, b = (p[k].to(dtype).clone().requires_grad_(True) for k in ("weight", "bias"))
    rm, rv = p["running_mean"].to(dtype).clone(), p["running_var"].to(dtype).clone()
    mean = yg.detach().mean(0) if training else rm.clone()
    var = yg.detach().var(0, unbiased=False) if training else rv.clone()
    z = F.batch_norm(yg, rm, rv, g, b, training, MOMENTUM, EPS)
    out = F.gelu(z) if gelu else z
    out.backward(dout.to(dtype))
    return BnRef(out.detach(), mean, (var + EPS).rsqrt(), yg.grad, g.grad, b.grad, rm, rv)


def _dgelu(z):
    return 0.5 * (1 + torch.erf(z * 0.7071067811865476)) + z * torch.exp(-0.5 * z * z) * 0.3989422804014327


def closed_bn_act(y, dout, p, gelu, training=True, dtype=torch.float64, rounding=False):
    """the closed form; rounding: out and dy rounded to bf16 on store (the statistics and the sums are not rounded)"""
    r = bf16 if rounding else (lambda t: t)
    y, dout = y.to(dtype), dout.to(dtype)
    M = y.shape[0]
    g, b = p["weight"].to(dtype), p["bias"].to(dtype)
    rm, rv = p["running_mean"].to(dtype).clone(), p["running_var"].to(dtype).clone()
    if training:
        mean = y.mean(0)
        var = ((y - mean) ** 2).mean(0)
        rm = (1 - MOMENTUM) * rm + MOMENTUM * mean
        rv = (1 - MOMENTUM) * rv + MOMENTUM * var * (M / max(M - 1, 1))
    else:
        mean, var = rm.clone(), rv.clone()
    rstd = 1 / (var + EPS).sqrt()
    yh = (y - mean) * rstd
    z = yh * g + b
    out = r(F.gelu(z) if gelu else z)
    dz = dout * _dgelu(z) if gelu else dout
    dbeta, dgamma = dz.sum(0), (dz * yh).sum(0)
    dy = g * rstd * (dz - dbeta / M - yh * dgamma / M) if training else g * rstd * dz
    return BnRef(out, mean, rstd, r(dy), dgamma, dbeta, rm, rv)


def bn_errors(got, want, training=True):
    e = {k: rel(getattr(got, k), getattr(want, k)) for k in BN_ACT + BN_F32}
    if training:
        e["running_mean"] = rel(got.running_mean, want.running_mean)
        e["running_var"] = rel(got.running_var, want.running_var)
    return e


# ------------------------------------------------------------------------------------------------ the stem ---
def torch_stem(x, dy, st, patch, training=True, dtype=torch.float64):
    """{"y", "ys" (each stage's conv output), "grad/<key>", "buf/<key>"} of the reference's lines under autograd"""
    n = len(CHANS[patch])
    q = {k: st[k].to(dtype).clone().requires_grad_(True) for k in param_keys(patch)}
    t, out, ys = x.to(dtype), {}, []
    for k in range(n):
        pre = f"proj.{2 * k}."
        rm, rv = st[pre + "1.running_mean"].to(dtype).clone(), st[pre + "1.running_var"].to(dtype).clone()
        t = F.conv2d(t, q[pre + "0.weight"], None, stride=2, padding=1)
        ys.append(grid_to_tok(t.detach()))
        t = F.batch_norm(t, rm, rv, q[pre + "1.weight"], q[pre + "1.bias"], training, MOMENTUM, EPS)
        if k + 1 < n:
            t = F.gelu(t)
        out["buf/" + pre + "1.running_mean"], out["buf/" + pre + "1.running_var"] = rm, rv
    y = grid_to_tok(t)
    if dy is not None:
        y.backward(dy.to(dtype))
        out.update({"grad/" + k: v.grad for k, v in q.items()})
    out["y"], out["ys"] = y.detach(), ys
    return out


def closed_stem(x, dy, st, patch, training=True, dtype=torch.float64, rounding=False):
    """the library's route (unfold, product, closed-form norm, fold) in `dtype`, with the declared bf16 roundings if asked"""
    r = bf16 if rounding else (lambda t: t)
    n = len(CHANS[patch])
    B = x.shape[0]
    t, (h, w) = r(x.to(dtype)), x.shape[2:]
    kept, out = [], {"ys": []}
    for k in range(n):
        pre = f"proj.{2 * k}."
        W = r(st[pre + "0.weight"].to(dtype))
        col = unfold_cols(t)                                       # t is already on the bf16 grid: the gather is a copy
        y = r(col @ W.reshape(W.shape[0], -1).T)
        p = {"weight": st[pre + "1.weight"], "bias": st[pre + "1.bias"], "running_mean": st[pre + "1.running_mean"],
             "running_var": st[pre + "1.running_var"]}
        kept.append((col, y, W, p, (h, w)))
        h, w = out_grid(h, w)
        f = closed_bn_act(y, torch.zeros_like(y), p, k + 1 < n, training, dtype, rounding)
        out["buf/" + pre + "1.running_mean"], out["buf/" + pre + "1.running_var"] = f.running_mean, f.running_var
        out["ys"].append(y.reshape(B, h * w, -1))
        t = tok_to_grid(f.out.reshape(B, h * w, -1), B, h, w)
    out["y"] = grid_to_tok(t)
    if dy is None:
        return out
    d = r(dy.to(dtype)).reshape(-1, dy.shape[-1])
    for k in range(n - 1, -1, -1):
        pre = f"proj.{2 * k}."
        col, y, W, p, (h, w) = kept[k]
        f = closed_bn_act(y, d, p, k + 1 < n, training, dtype, rounding)
        out["grad/" + pre + "1.weight"], out["grad/" + pre + "1.bias"] = f.dgamma, f.dbeta
        out["grad/" + pre + "0.weight"] = (f.dy.T @ col).reshape(W.shape)
        if k:
            dcol = r(f.dy @ W.reshape(W.shape[0], -1))
            d = r(grid_to_tok(fold_cols(dcol, B, h, w))).reshape(-1, W.shape[1])
    return out


def fx_rel(got, want):
    """rel of a computed tensor against a fixture entry: whole, or (fixture_codec.Compact) its sample and its row sums"""
    g = got.detach().double().cpu()
    if isinstance(want, torch.Tensor):
        return rel(g, want)
    return max(rel(g.reshape(-1)[::want.stride], want.sample), rel(g.sum(-1), want.rows))


def fixture_case(fx, name):
    """(x, dy, state, patch, want) of one configuration of tests/golden/conv_patch_embed.npz; want: y, y_eval, grad/*, buf/*"""
    import fixture_codec as FC
    d = FC.group(fx, name)
    st = FC.group(d, "state")
    patch = 16 if name == "p16" else 8
    want = {"y": d["y"], "y_eval": d["y_eval"]}
    want.update({"grad/" + k: d["grad/" + k] for k in param_keys(patch)})
    want.update({"buf/" + k: d["after/" + k] for k in buffer_keys(patch) if not k.endswith("tracked")})
    return d["x"], d["dy"], st, patch, want


def module_errors(got, want):
    return {k: fx_rel(got[k], want[k]) for k in want}


WIDE_CASE = ((64, 3, 64, 64), 8, 64)              # image, patch, embed_dim: more workgroups than CUs in the first stage


def wide_state(patch, E, seed):
    st, ch = {}, stage_channels(patch, E)
    for k, (ci, co) in enumerate(zip(ch[:-1], ch[1:])):
        pre = f"proj.{2 * k}."
        st[pre + "0.weight"] = bf16(gen((co, ci, 3, 3), seed + 10 * k, (9 * ci) ** -0.5))
        b = bn_params(co, seed + 10 * k)
        st.update({pre + "1." + n: v for n, v in b.items()})
    return st
