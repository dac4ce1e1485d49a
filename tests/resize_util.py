"""Torch restatement of the device resize pipeline, for the resize tests: Pillow's two integer passes (horizontal
first, uint8 intermediate) vectorised in int64 over the coefficient tables of vit_torch_amd.resize, and the
crop / flip / ToTensor / Normalize chain of utils_datasets.py:553-582 on the result."""
import torch
import torch.nn.functional as F


def _pass(x, tab, axis):
    """One axis of Pillow's 8-bit resample: out[o] = clamp((2^21 + sum_t x[start[o] + t] * k[t][o]) >> 22, 0, 255)."""
    tab = tab.cpu().long()
    taps, n_out = tab.shape[0] - 2, tab.shape[1]
    start, k = tab[0], tab[2:]
    idx = (start[None, :] + torch.arange(taps)[:, None]).clamp(max=x.shape[axis] - 1)    # weights past count are 0
    g = x.index_select(axis, idx.reshape(-1))
    shape = list(x.shape)
    shape[axis:axis + 1] = [taps, n_out]
    kshape = [1] * len(shape)
    kshape[axis], kshape[axis + 1] = taps, n_out
    acc = (g.reshape(shape) * k.reshape(kshape)).sum(axis) + (1 << 21)
    return (acc >> 22).clamp(0, 255)


def resize_u8(img_nhwc, ytab, xtab):
    """uint8 [B,H,W,C] -> uint8 [B,Hr,Wr,C], Pillow's bicubic resize bit for bit."""
    x = img_nhwc.cpu().long()
    return _pass(_pass(x, xtab, 2), ytab, 1).to(torch.uint8)


def crop_flip_normalize(img_u8_nhwc, oy, ox, flip, mean, std, S, pad, fill=128):
    """RandomCrop(S, padding=pad, fill) at the given offsets -> flip -> ToTensor -> Normalize, per image."""
    out = []
    for b in range(img_u8_nhwc.shape[0]):
        im = img_u8_nhwc[b].permute(2, 0, 1)
        im = F.pad(im, (pad, pad, pad, pad), value=fill)
        im = im[:, oy[b]:oy[b] + S, ox[b]:ox[b] + S]
        if flip[b]:
            im = im.flip(-1)
        x = im.float().div(255)
        out.append((x - mean[:, None, None]) / std[:, None, None])
    return torch.stack(out)
