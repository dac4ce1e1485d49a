"""The plain-PyTorch talking-heads and class attention that the CaiT kernel tests compare against."""
from collections import namedtuple

import torch

TalkingHeadsRef = namedtuple("TalkingHeadsRef", "out dqkv dWl dbl dWw dbw img_dWl img_dWw img_dbw")
TalkingHeadsRef.__doc__ = """out [B,N,H*hd], dqkv [B,N,3,H,hd], dWl / dWw [H,H], dbl / dbw [H]; img_dWl / img_dWw [B,H,H] and
img_dbw [B,H]: each image's contribution to dWl, dWw and dbw, i.e. what dropping that image from a sum over the batch would
take out of them."""


def torch_talking_heads(qkv, dO, Wl, bl, Ww, bw, scale, dtype=torch.float32, images_per_chunk=None):
    """models/cait.py:111-128 (q k^T -> proj_l -> softmax -> proj_w -> @ v) and its backward by autograd in `dtype` on the
    CPU, `images_per_chunk` images at a time (images are independent; the parameter gradients sum over the chunks).
    qkv [B,N,3,H,hd], dO [B,N,H,hd] (or [B,N,H*hd]); returns a TalkingHeadsRef."""
    B, N, _, H, hd = qkv.shape
    step = images_per_chunk or B
    out = torch.empty((B, N, H * hd), dtype=dtype)
    dqkv = torch.empty((B, N, 3, H, hd), dtype=dtype)
    grads = None
    img_dWl, img_dWw, img_dbw = (torch.empty((B, H, H), dtype=dtype), torch.empty((B, H, H), dtype=dtype),
                                 torch.empty((B, H), dtype=dtype))
    for b0 in range(0, B, step):
        b1 = min(B, b0 + step)
        nb = b1 - b0
        x = qkv[b0:b1].to(dtype).clone().requires_grad_(True)
        prm = [t.to(dtype).clone().requires_grad_(True) for t in (Wl, bl, Ww, bw)]
        q, k, v = x[:, :, 0].permute(0, 2, 1, 3) * scale, x[:, :, 1].permute(0, 2, 1, 3), x[:, :, 2].permute(0, 2, 1, 3)
        S = q @ k.transpose(-2, -1)                                                      # [b,H,N,N]
        Sm = (S.permute(0, 2, 3, 1) @ prm[0].t() + prm[1]).permute(0, 3, 1, 2)
        P = Sm.softmax(dim=-1)
        Pm = (P.permute(0, 2, 3, 1) @ prm[2].t() + prm[3]).permute(0, 3, 1, 2)
        Sm.retain_grad()
        Pm.retain_grad()
        o = (Pm @ v).transpose(1, 2).reshape(nb, N, H * hd)
        o.backward(dO[b0:b1].to(dtype).reshape(nb, N, H * hd))
        out[b0:b1] = o.detach()
        dqkv[b0:b1] = x.grad
        if grads is None:
            grads = [p.grad.clone() for p in prm]
        else:
            for g, p in zip(grads, prm):
                g += p.grad
        with torch.no_grad():
            img_dWl[b0:b1] = torch.einsum("bpij,bhij->bph", Sm.grad, S)
            img_dWw[b0:b1] = torch.einsum("boij,bpij->bop", Pm.grad, P)
            img_dbw[b0:b1] = Pm.grad.sum((2, 3))
    return TalkingHeadsRef(out, dqkv, *grads, img_dWl, img_dWw, img_dbw)


def reference(qkv, Wl, bl, Ww, bw, dO, scale):
    """models/cait.py:111-128 in fp32 on the bf16-rounded operands; returns O and every gradient."""
    r = torch_talking_heads(qkv, dO, Wl, bl, Ww, bw, scale)
    return r.out, r.dqkv, r.dWl, r.dbl, r.dWw, r.dbw


def torch_th_softmax(S, dPm, Wl, bl, Ww, bw, dtype=torch.float64):
    """proj_l -> softmax -> proj_w on score rows S [b,H,N,N] and the backward of dPm through it, in `dtype`:
    (P, P', dS, dWl, dbl, dWw, dbw) and each image's contribution to dWl, dWw and dbw ([b,H,H], [b,H,H], [b,H])."""
    Sr = S.to(dtype).clone().requires_grad_(True)
    prm = [t.to(dtype).clone().requires_grad_(True) for t in (Wl, bl, Ww, bw)]
    Sm = (Sr.permute(0, 2, 3, 1) @ prm[0].t() + prm[1]).permute(0, 3, 1, 2)
    P = Sm.softmax(-1)
    Pm = (P.permute(0, 2, 3, 1) @ prm[2].t() + prm[3]).permute(0, 3, 1, 2)
    Sm.retain_grad()
    g = dPm.to(dtype)
    Pm.backward(g)
    with torch.no_grad():
        img = (torch.einsum("bpij,bhij->bph", Sm.grad, Sr), torch.einsum("boij,bpij->bop", g, P), g.sum((2, 3)))
    return (P.detach(), Pm.detach(), Sr.grad) + tuple(p.grad for p in prm) + img


def torch_class_attention(q, k, v, do, H, dtype=torch.float64):
    """The class-attention core (models/cait.py Class_Attention: the CLS query against every token) and its backward in
    `dtype`: q / do [B,D], k / v [B,N,D] (any strides); returns (out, p, dq, dk, dv): out / dq [B,D], the softmax p
    [B,H,N], dk / dv [B,N,D]."""
    B, N, D = k.shape
    hd = D // H
    qr, kr, vr = (t.to(dtype).clone().requires_grad_(True) for t in (q, k, v))
    qh = qr.reshape(B, 1, H, hd).permute(0, 2, 1, 3) * hd ** -0.5
    kh, vh = kr.reshape(B, N, H, hd).permute(0, 2, 1, 3), vr.reshape(B, N, H, hd).permute(0, 2, 1, 3)
    p = (qh @ kh.transpose(-2, -1)).softmax(-1)
    o = (p @ vh).transpose(1, 2).reshape(B, D)
    o.backward(do.to(dtype))
    return o.detach(), p.detach().reshape(B, H, N), qr.grad, kr.grad, vr.grad

