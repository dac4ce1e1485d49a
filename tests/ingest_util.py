"""One plain-torch CPU reference of the four uint8 ingest kernels (csrc/ingest.hip, csrc/resize.hip), and the table of
cases that tests/test_ingest_ref_cpu.py (the reference against Pillow, no GPU) and tests/test_ingest_forms_gpu.py (the
kernels against the reference, bit for bit) both walk.

ingest_ref      : [Pillow bicubic resize ->] RandomCrop(S, padding, fill) -> flip -> ToTensor -> Normalize, fp32 NCHW
patch_rows_ref  : fp32 NCHW -> patch rows [B*(cls_rows + (S/p)^2), ld], k = c*p*p + i*p + j, one rounding
"""
import zlib
from collections import namedtuple

import torch

from tests.resize_util import crop_flip_normalize, resize_u8

MEAN = [0.44671062065972217, 0.43980983983523964, 0.40664644709967324, 0.5]      # STL-10's three, one more for C = 4
STD = [0.2603409782662331, 0.25657727311344447, 0.27126738145225493, 0.25]


def _list(v, B, default):
    if v is None:
        return [default] * B
    return v.cpu().tolist() if torch.is_tensor(v) else list(v)


def ingest_ref(src_u8_nhwc, oy, ox, flip, mean, std, S, pad, fill, ytab=None, xtab=None):
    """uint8 [B,H,W,C] -> fp32 [B,C,S,S].  ytab / xtab: resize first (tests.resize_util.resize_u8).  oy / ox / flip None:
    centre, no flip (oy = ox = pad); mean / std None: 0 / 1."""
    src = src_u8_nhwc.cpu()
    if ytab is not None:
        src = resize_u8(src, ytab, xtab)
    B, C = src.shape[0], src.shape[3]
    mean = torch.zeros(C) if mean is None else torch.as_tensor(mean, dtype=torch.float32).cpu()
    std = torch.ones(C) if std is None else torch.as_tensor(std, dtype=torch.float32).cpu()
    return crop_flip_normalize(src, _list(oy, B, pad), _list(ox, B, pad), _list(flip, B, 0), mean, std, S, pad, fill)


def patch_rows_ref(x_nchw, p, cls_rows, ld, dtype):
    """fp32 [B,C,S,S] -> [B*(cls_rows + (S/p)^2), ld] in dtype: row = one p x p patch (row-major over the patch grid), column
    k = c*p*p + i*p + j; cls rows and columns >= C*p*p zero."""
    B, C, S, _ = x_nchw.shape
    g = S // p
    rows = x_nchw.reshape(B, C, g, p, g, p).permute(0, 2, 4, 1, 3, 5).reshape(B, g * g, C * p * p)
    out = torch.zeros(B, cls_rows + g * g, ld, dtype=torch.float32)
    out[:, cls_rows:, :C * p * p] = rows
    return out.to(dtype).reshape(B * (cls_rows + g * g), ld)


# ------------------------------------------------------------------------------------------------- the case table ---
# offsets "corners": the four corners of [0, max_y] x [0, max_x] and an interior point, with both flip values on the
# interior and on two of the corners (B = 8); None: the evaluation form (no offsets, no flip; B = 5).
# patch: the (p, cls_rows, extra zero columns, dtype) forms of the patchify kernel run on the case (S % p == 0).
Case = namedtuple("Case", "name H W C Hr Wr S pad fill norm offsets interior patch band")
BF, F32 = torch.bfloat16, torch.float32


def _case(name, H, W, C, S, pad, *, Hr=None, Wr=None, fill=128, norm=True, offsets="corners", interior=None, patch=(),
          band=None):
    return Case(name, H, W, C, Hr, Wr, S, pad, fill, norm, offsets, interior, tuple(patch), band)


_ALL_PATCH = [(p, cls, extra, dt) for p in (4, 8, 16) for cls in (0, 1, 2) for extra in (0, 8) for dt in (BF, F32)]

# image_ingest / ingest_patchify
PLAIN_CASES = [
    _case("40x56_c3", 40, 56, 3, 32, 4, patch=_ALL_PATCH),
    _case("56x40_c2_fill0_nonorm", 56, 40, 2, 32, 4, fill=0, norm=False, patch=[(4, 0, 8, F32), (16, 2, 0, BF)]),
    _case("40x56_c1_fill255", 40, 56, 1, 32, 4, fill=255, patch=[(8, 2, 8, BF), (4, 1, 0, F32)]),
    _case("56x40_c4", 56, 40, 4, 32, 4, norm=False, patch=[(8, 1, 0, BF), (16, 0, 8, F32)]),
    _case("eval_32_c3", 32, 32, 3, 32, 0, offsets=None, patch=[(16, 1, 0, BF), (8, 0, 8, F32)]),
    _case("centre_40x56_c3_fill0", 40, 56, 3, 32, 4, fill=0, offsets=None, patch=[(8, 1, 8, BF)]),
    # pad = S: the crops at oy = 0 and oy = max_y (every corner) lie wholly in the padding, the interior one straddles it
    _case("all_padding_8_c3_fill255", 8, 8, 3, 8, 8, fill=255, interior=(4, 11), patch=[(4, 1, 0, F32), (8, 2, 8, BF)]),
]

# resize_ingest / resize_ingest_patchify; band = the rows per workgroup the plain form must run with (the patchify forms
# listed run with the same band: tests/test_ingest_ref_cpu.py asserts both through vitmi_resize_ingest_plan)
RESIZE_CASES = [
    # distinct axes: rows up / columns down and the transpose; S = 40 at a band of 32 leaves a ragged 8-row last band
    _case("48x64_c3_to_72x40", 48, 64, 3, 40, 4, Hr=72, Wr=40, band=32, patch=[(8, 1, 8, BF)]),
    _case("64x48_c2_to_40x72_fill0_nonorm", 64, 48, 2, 40, 4, Hr=40, Wr=72, band=32, fill=0, norm=False,
          patch=[(8, 0, 0, F32)]),
    _case("240x176_c4_to_32x40_fill255", 240, 176, 4, 32, 4, Hr=32, Wr=40, band=4, fill=255, patch=[(4, 2, 8, BF)]),
    _case("176x240_c1_to_40x32", 176, 240, 1, 32, 4, Hr=40, Wr=32, band=32, norm=False, patch=[(16, 1, 0, F32)]),
    # W*C odd (byte-wise staging, every image after the first at an unaligned base); a 4-row last band at S = 36
    _case("37x37_c3_to_100x100_s36", 37, 37, 3, 36, 4, Hr=100, Wr=100, band=32, patch=[(4, 1, 0, F32)]),
    _case("37x37_c3_to_100x100_s40", 37, 37, 3, 40, 4, Hr=100, Wr=100, band=32, patch=[(8, 1, 0, BF)]),
    # W*C a multiple of 16: the 16-byte staging path on every image
    _case("96x96_c1_to_40x40", 96, 96, 1, 32, 4, Hr=40, Wr=40, band=32, patch=[(8, 1, 8, F32)]),
    # the band ladder
    _case("160x160_c3_to_32x32", 160, 160, 3, 32, 4, Hr=32, Wr=32, band=16, patch=[(16, 1, 0, BF)]),
    _case("176x176_c3_to_32x32", 176, 176, 3, 32, 4, Hr=32, Wr=32, band=8, patch=[(8, 0, 8, BF)]),
    _case("240x240_c3_to_32x32", 240, 240, 3, 32, 4, Hr=32, Wr=32, band=4, patch=[(4, 1, 0, F32)]),
    _case("240x240_c4_to_32x32_fill0", 240, 240, 4, 32, 4, Hr=32, Wr=32, band=2, fill=0),
    _case("240x320_c4_to_32x43", 240, 320, 4, 32, 4, Hr=32, Wr=43, band=1, norm=False),
    # bands that lie wholly in the crop padding: pad >= band
    _case("240x240_c3_to_32x32_pad8", 240, 240, 3, 32, 8, Hr=32, Wr=32, band=4, fill=255, patch=[(4, 1, 0, BF)]),
    _case("40x40_c3_to_32x32_pad32", 40, 40, 3, 32, 32, Hr=32, Wr=32, band=32, interior=(32, 21),
          patch=[(8, 1, 0, F32)]),
]

CASES = {c.name: c for c in PLAIN_CASES + RESIZE_CASES}

# run through the plain kernels, and through the resize kernels with resize.table(40, 40) on both axes: the identity
IDENTITY_CASE = _case("identity_40_c3", 40, 40, 3, 32, 4)


def extent(c):
    """The image the crop runs over: the resized one, or the source."""
    return (c.Hr, c.Wr) if c.Hr else (c.H, c.W)


def draws(c):
    """(oy, ox, flip) as lists, pinned: see the table's header.  (None, None, None) for the evaluation form."""
    if c.offsets is None:
        return None, None, None
    eh, ew = extent(c)
    my, mx = eh + 2 * c.pad - c.S, ew + 2 * c.pad - c.S
    iy, ix = c.interior if c.interior else (my // 2, mx // 3 + 1)
    assert 0 <= iy <= my and 0 <= ix <= mx
    oy = [0, 0, my, my, iy, iy, 0, my]
    ox = [0, mx, 0, mx, ix, ix, mx, 0]
    fl = [0, 1, 0, 1, 0, 1, 0, 1]
    return oy, ox, fl


def batch_size(c):
    return 5 if c.offsets is None else 8


def source(c):
    """The case's uint8 NHWC batch: fixed random bytes, another image per batch entry."""
    g = torch.Generator("cpu").manual_seed(zlib.crc32(c.name.encode()))
    return torch.randint(0, 256, (batch_size(c), c.H, c.W, c.C), generator=g, dtype=torch.uint8)


def norm(c):
    """(mean, std) fp32 [C] tensors, or (None, None)."""
    if not c.norm:
        return None, None
    return torch.tensor(MEAN[:c.C], dtype=torch.float32), torch.tensor(STD[:c.C], dtype=torch.float32)


def tables(c):
    """(ytab, xtab) of a resize case, (None, None) of a plain one."""
    if not c.Hr:
        return None, None
    from vit_torch_amd import resize
    return resize.table(c.H, c.Hr), resize.table(c.W, c.Wr)


_REF = {}


def reference(c):
    """ingest_ref of the case on its pinned draws, computed once and shared (do not write to it)."""
    if c.name not in _REF:
        oy, ox, fl = draws(c)
        _REF[c.name] = ingest_ref(source(c), oy, ox, fl, *norm(c), c.S, c.pad, c.fill, *tables(c))
    return _REF[c.name]
