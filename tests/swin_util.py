"""The plain-PyTorch window attention that the Swin kernel tests compare against."""
from collections import namedtuple

import torch

from util import bf16_round, rel_err

F64 = torch.float64

WindowAttentionRef = namedtuple("WindowAttentionRef", "out mask dqkv dbias lse ds_max qb_max")
WindowAttentionRef.__doc__ = """out [B,L,C], mask [nW,N,N] or None, dqkv [B,L,3C], dbias [H,N,N], lse [Bw*H*N] (the
kernels' layout); ds_max / qb_max [Bw,H]:
per (window, head), max |d(score)| and max |column sum of that window's dq/dk/dv rows of that head|, i.e. what
dropping one window from a head's walk would take out of dbias and of the qkv-bias sums."""


def torch_window_attention(qkv, do, bias, B, Hh, Ww, ws, shift, H, hd, dtype=torch.float32, images_per_chunk=None):
    """roll -> window_partition -> attention(+bias,+mask) -> window_reverse -> roll back (models/swin.py:241-261) in
    `dtype` on the CPU, `images_per_chunk` images at a time (windows are independent; dbias sums over the chunks).
    Returns a WindowAttentionRef; its first four fields unpack as (out, mask, dqkv, dbias)."""
    from oracle.swin_ref import shift_attn_mask, window_partition, window_reverse
    C, N, L = H * hd, ws * ws, Hh * Ww
    nW = (Hh // ws) * (Ww // ws)
    scale = hd ** -0.5
    mask = shift_attn_mask(Hh, Ww, ws, shift) if shift > 0 else None
    md = mask.to(dtype) if mask is not None else None
    step = images_per_chunk or B
    out = torch.empty((B, L, C), dtype=dtype)
    dqkv = torch.empty((B, L, 3 * C), dtype=dtype)
    dbias = torch.zeros((H, N, N), dtype=dtype)
    lse, ds_max, qb_max = [], [], []
    for b0 in range(0, B, step):
        b1 = min(B, b0 + step)
        nb = b1 - b0
        qr = qkv[b0:b1].to(dtype).clone().requires_grad_(True)
        br = bias.to(dtype).clone().requires_grad_(True)
        x = qr.view(nb, Hh, Ww, 3 * C)
        if shift:
            x = torch.roll(x, shifts=(-shift, -shift), dims=(1, 2))
        xw = window_partition(x, ws).view(-1, N, 3, H, hd).permute(2, 0, 3, 1, 4)
        q, k, v = xw[0] * scale, xw[1], xw[2]
        attn = q @ k.transpose(-2, -1) + br.unsqueeze(0)
        if md is not None:
            attn = (attn.view(nb, nW, H, N, N) + md.unsqueeze(1).unsqueeze(0)).view(-1, H, N, N)
        attn.retain_grad()
        lse.append(attn.detach().logsumexp(-1).reshape(-1))
        o = (attn.softmax(-1) @ v).transpose(1, 2).reshape(-1, ws, ws, C)
        o = window_reverse(o, ws, Hh, Ww)
        if shift:
            o = torch.roll(o, shifts=(shift, shift), dims=(1, 2))
        o = o.reshape(nb, L, C)
        o.backward(do[b0:b1].to(dtype))
        out[b0:b1] = o.detach()
        dqkv[b0:b1] = qr.grad
        dbias += br.grad
        ds_max.append(attn.grad.abs().amax((-2, -1)))
        g = qr.grad.view(nb, Hh, Ww, 3 * C)
        if shift:
            g = torch.roll(g, shifts=(-shift, -shift), dims=(1, 2))
        qb_max.append(window_partition(g, ws).view(-1, N, 3, H, hd).sum(1).abs().amax((1, 3)))
    return WindowAttentionRef(out, mask, dqkv, dbias, torch.cat(lse), torch.cat(ds_max), torch.cat(qb_max))


# ------------------------------------------------------------------ helpers of the float64 kernel-level test files ---
def gen(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator("cpu").manual_seed(seed)) * scale


def check(name, got, want, bound):
    """rel-to-max error, printed beside its bound before it is asserted."""
    g = got.detach().float().cpu()
    assert tuple(g.shape) == tuple(want.shape), f"{name}: shape {tuple(g.shape)} vs {tuple(want.shape)}"
    assert torch.isfinite(g).all(), f"{name}: non-finite values in result"
    e = rel_err(got.detach().double().cpu(), want.double())
    print(f"\n  {name}: {e:.2e} (bound {bound:.1e})", end="")
    assert e <= bound, f"{name}: rel-to-max error {e:.3e} > {bound:.1e}"
    return e


def bounds(c, path):
    """(out, lse, dqkv, dbias) bounds of a path: 'fp32', 'vector' (bf16) or 'mfma' (bf16).  `c`: a test file's own
    constants, a dict with FP32_GRADE, VEC_OUT, VEC_DQKV, MFMA_OUT, MFMA_DQKV and QKV_BIAS."""
    return {"fp32": (c["FP32_GRADE"], c["FP32_GRADE"], c["FP32_GRADE"], c["FP32_GRADE"]),
            "vector": (c["VEC_OUT"], c["FP32_GRADE"], c["VEC_DQKV"], c["FP32_GRADE"]),
            "mfma": (c["MFMA_OUT"], c["FP32_GRADE"], c["MFMA_DQKV"], c["FP32_GRADE"])}[path]


def nan(shape, dt):
    return torch.full(shape, float("nan"), device="cuda", dtype=dt)


def inputs(B, Hh, Ww, ws, H, hd, seed):
    """bf16-rounded qkv / dO (both sides see identical operands in both dtypes) and an fp32 bias table."""
    C, N, L = H * hd, ws * ws, Hh * Ww
    return (bf16_round(gen((B, L, 3 * C), seed)), bf16_round(gen((B, L, C), seed + 1)),
            gen((H, N, N), seed + 2, 0.5))


def bits(t):
    """a tensor's bits as integers, so that torch.equal compares NaNs and signed zeros too."""
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def run(ops, qkv, do, bias, mask, B, Hh, Ww, ws, shift, H, hd, dt, qkv_bias=False):
    """forward + backward on the device, every output NaN-filled first; returns (O, lse, dqkv, dbias, dqkv_bias)."""
    C, N, L = H * hd, ws * ws, Hh * Ww
    Bw = B * (Hh // ws) * (Ww // ws)
    Q = qkv.to("cuda", dt).contiguous()
    O, lse = nan((B, L, C), dt), nan((Bw * H * N,), torch.float32)
    bd = bias.cuda().float().contiguous()
    md = mask.cuda().float().contiguous() if mask is not None else None
    ops.win_attn_fwd(Q, O, lse, bd, md, Bw, H, N, hd, Hh, Ww, ws, shift, hd ** -0.5)
    dqkv, dbias = nan((B, L, 3 * C), dt), nan((H * N * N,), torch.float32)
    qb = nan((3 * C,), torch.float32) if qkv_bias else None
    ops.win_attn_bwd(Q, do.to("cuda", dt).contiguous(), lse, bd, md, dqkv, dbias, Bw, H, N, hd, Hh, Ww, ws, shift,
                     hd ** -0.5, dqkv_bias=qb)
    return O, lse, dqkv, dbias.view(H, N, N), qb


def compare(c, ops, lib, path, B, Hh, Ww, ws, shift, H, hd, seed, tag, images_per_chunk=None, force=True, ref=None):
    """One shape on one path against float64, at the bounds of `c` (see bounds); returns (reference, dbias error,
    qkv-bias error or None).  `force`: the vector path is forced through the MFMA switch (else left to the dispatch).
    `ref`: (qkv, do, bias, reference) of these arguments where the caller already has them."""
    if path == "vector" and force:
        lib.vitmi_debug_win_attn_mfma(0)
    dt = torch.float32 if path == "fp32" else torch.bfloat16
    if ref is None:
        qkv, do, bias = inputs(B, Hh, Ww, ws, H, hd, seed)
        r = torch_window_attention(qkv, do, bias, B, Hh, Ww, ws, shift, H, hd, F64, images_per_chunk)
    else:
        qkv, do, bias, r = ref
    fuse = ops.win_attn_bwd_fuses_qkv_bias(torch.empty(1, dtype=dt), hd)
    assert fuse == (path == "mfma" and hd == 32)
    O, lse, dqkv, dbias, qb = run(ops, qkv, do, bias, r.mask, B, Hh, Ww, ws, shift, H, hd, dt, qkv_bias=fuse)
    bo, bl, bq, bb = bounds(c, path)
    check(f"{tag}.out", O, r.out, bo)
    check(f"{tag}.lse", lse, r.lse, bl)
    check(f"{tag}.dqkv", dqkv, r.dqkv, bq)
    eb = check(f"{tag}.dbias", dbias, r.dbias, bb)
    eq = None
    if fuse:
        eq = check(f"{tag}.dqkv_bias", qb, r.dqkv.reshape(-1, 3 * H * hd).sum(0), c["QKV_BIAS"])
        # the fused sums ride on the same kernel: dqkv is the same to the bit without them
        _, _, dqkv2, _, _ = run(ops, qkv, do, bias, r.mask, B, Hh, Ww, ws, shift, H, hd, dt)
        assert torch.equal(bits(dqkv2), bits(dqkv))
    return r, eb, eq


def dev_err(got, want):
    """rel-to-max error computed on the device (these tensors are hundreds of MB)."""
    g, w = got.double(), want.double()
    assert torch.isfinite(g).all()
    return ((g - w).abs().max() / w.abs().max()).item()


def window_tokens(Hh, Ww, ws, shift, bw, nW):
    """token rows (in image order, over the whole batch) of window bw, through the roll."""
    from oracle.swin_ref import window_partition
    idx = torch.arange(Hh * Ww).view(1, Hh, Ww, 1)
    if shift:
        idx = torch.roll(idx, shifts=(-shift, -shift), dims=(1, 2))
    return window_partition(idx, ws).view(nW, ws * ws)[bw % nW] + (bw // nW) * Hh * Ww


# ------------------------------------------------- the backward walk at windows of more than 64 tokens (9..12) ---
def big_rows(H, Bw):
    """backward workgroups per head at N > 64; workgroup r walks windows r, r + R, ... (swin_ops.hip, win_big_rows)."""
    return max(1, min(256 // H, Bw))


# (ws, H, Hh, Ww, shift, B, R % nW != 0): Bw = B * nW windows, R = min(256 // H, Bw), 2-3 windows per workgroup but
# for h48_long; the batch is the smallest that still walks unevenly at the head count that fixes R
WALKS12 = {
    "h32": (12, 32, 12, 12, 0, 19, False),        # Swin-B stage-4 heads, one window per image: R 8, Bw 19
    "h48": (12, 48, 12, 12, 0, 13, False),        # Swin-L stage-4 heads: R 5, Bw 13
    "h48_long": (12, 48, 12, 12, 0, 42, False),   # R 5, Bw 42: 8-9 read-modify-write steps of the d(bias) partial
    "h24": (12, 24, 24, 24, 6, 6, True),          # R 10, nW 4: the mask window alternates along a walk
    "h6": (12, 6, 24, 24, 6, 23, True),           # Swin-L stage-1 heads: R 42, Bw 92, R % nW = 2
    "h3": (12, 3, 24, 36, 6, 29, True),           # R 85, Bw 174, nW 6, R % nW = 1: the mask window changes every step
    "w9": (9, 24, 18, 18, 4, 6, True),            # the walk of each other template instance: R 10, Bw 24
    "w10": (10, 24, 20, 20, 5, 6, True),
    "w11": (11, 24, 22, 22, 5, 6, True),
}


def walk_shape(case):
    """(B, Hh, Ww, ws, shift, H, Bw, R) of a walk case, with the properties the case is there for asserted."""
    ws, H, Hh, Ww, shift, B, mask_moves = WALKS12[case]
    nW = (Hh // ws) * (Ww // ws)
    Bw = B * nW
    R = big_rows(H, Bw)
    assert Bw > R and Bw % R != 0, f"{case}: Bw {Bw}, R {R} is no uneven walk"
    if mask_moves:
        assert shift > 0 and R % nW != 0, f"{case}: R {R}, nW {nW}: the mask window stays the same along a walk"
    return B, Hh, Ww, ws, shift, H, Bw, R


def drop_margins(r, H, hd):
    """what dropping one (window, head) takes out of dbias and out of the qkv-bias sums at the least, relative to their
    largest element: with random inputs the sums over windows grow like sqrt(Bw), so about one part in sqrt(Bw)."""
    qref = r.dqkv.reshape(-1, 3 * H * hd).sum(0)
    return (r.ds_max / r.dbias.abs().max()).min().item(), (r.qb_max / qref.abs().max()).min().item()
