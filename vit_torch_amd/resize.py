"""PIL's bicubic resize coefficients for the device input pipeline (`vitmi_resize_ingest`).

The reference's datasets hand PIL images to `transforms.Resize(S, BICUBIC)` (utils_datasets.py:553-582), so the resize
it trains on is Pillow's `ImagingResample` for 8-bit images, not `F.interpolate(mode="bicubic")` (a = -0.75, float
arithmetic).  Pillow's algorithm, per axis (`precompute_coeffs` + `normalize_coeffs_8bpc` in Resample.c):

- bicubic filter, a = -0.5, support 2; `scale = in/out`, `filterscale = max(scale, 1)`, `support = 2*filterscale`,
  `taps = 2*ceil(support) + 1`;
- output index o: `center = (o + 0.5)*scale`, `start = max(int(center - support + 0.5), 0)`,
  `count = min(int(center + support + 0.5), in) - start`, `w_t = filter((t + start - center + 0.5) / filterscale)`
  (Pillow multiplies by its reciprocal), normalised by their sum, all in double;
- fixed point with 22 fractional bits: `k = int(w*2^22 + 0.5)` for w >= 0, `int(w*2^22 - 0.5)` for w < 0 (`int`
  truncates toward zero).

The kernels never compute a weight: they take these tables as int32 device arrays and run the two integer passes
(horizontal first, uint8 intermediate; each value clamp((2^21 + sum src*k) >> 22, 0, 255)).  Python floats are C
doubles, so the tables here are Pillow's own.

Device layout of one axis (`table`): int32 [2 + taps, out] = start[out], count[out], k[taps][out], zero weights past
each row's count.
"""
from __future__ import annotations

import math

import torch

from ._lib import VitmiError

TAP_LIMIT = 32          # longest coefficient row the kernels take (csrc/resize.hip kTapLimit)
PRECISION_BITS = 32 - 8 - 2


def _bicubic(x: float) -> float:
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def coeffs(in_size: int, out_size: int):
    """(starts, counts, fixed-point weights per output index, taps) of one axis, as Pillow computes them."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size <= 0 or out_size <= 0:
        raise VitmiError(f"resize: sizes must be positive ({in_size} -> {out_size})")
    scale = filterscale = in_size / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = 2.0 * filterscale
    taps = int(math.ceil(support)) * 2 + 1
    if taps > TAP_LIMIT:
        raise VitmiError(f"resize {in_size} -> {out_size} needs {taps} taps per output; the kernels take at most "
                         f"{TAP_LIMIT} (a downscale by more than {(TAP_LIMIT - 1) // 2 / 2:g}x)")
    ss = 1.0 / filterscale
    one = 1 << PRECISION_BITS
    starts, counts, weights = [], [], []
    for o in range(out_size):
        center = (o + 0.5) * scale
        lo = int(center - support + 0.5)
        if lo < 0:
            lo = 0
        hi = int(center + support + 0.5)
        if hi > in_size:
            hi = in_size
        n = hi - lo
        w = [_bicubic((t + lo - center + 0.5) * ss) for t in range(n)]
        total = 0.0
        for v in w:
            total += v
        if total != 0.0:
            w = [v / total for v in w]
        k = [int(-0.5 + v * one) if v < 0 else int(0.5 + v * one) for v in w]
        starts.append(lo)
        counts.append(n)
        weights.append(k)
    return starts, counts, weights, taps


def table(in_size: int, out_size: int, device="cpu") -> torch.Tensor:
    """int32 [2 + taps, out_size]: start, count, then the weights tap by tap (the kernels' layout)."""
    starts, counts, weights, taps = coeffs(in_size, out_size)
    t = torch.zeros((2 + taps, out_size), dtype=torch.int32)
    t[0] = torch.tensor(starts, dtype=torch.int32)
    t[1] = torch.tensor(counts, dtype=torch.int32)
    for o, k in enumerate(weights):
        t[2:2 + len(k), o] = torch.tensor(k, dtype=torch.int32)
    return t.to(device)

