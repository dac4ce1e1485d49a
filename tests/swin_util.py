"""The plain-PyTorch window attention that the Swin kernel tests compare against."""
from collections import namedtuple

import torch

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
