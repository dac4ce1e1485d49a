"""Compact storage of the window-12 golden vectors (tests/golden/*_ws12.npz), shared by their generator and tests.

Three forms keep a fixture small without loosening what it pins:
- inputs and weights are drawn on an int8 grid with a power-of-two scale (`quantize`), so the int8 copy decodes to
  exactly the fp32 values the reference ran on (`q8:<key>` + `q8s:<key>`);
- integer buffers are int16 (`i16:<key>`);
- a float result of more than `limit` entries keeps a fixed-stride sample of its flat entries (`<key>@s`, stride
  `<key>@stride`) and the sums of its rows over the last dimension (`<key>@rows`, summed in float64); smaller results
  are stored whole.  `check` compares a computed tensor with either form.
"""
import math

import numpy as np
import torch

from util import assert_close

SAMPLE = 4096


def pow2_scale(t: torch.Tensor) -> float:
    m = float(t.abs().max())
    return 2.0 ** math.ceil(math.log2(m / 127.0)) if m > 0 else 1.0


def quantize(t: torch.Tensor, scale: float) -> torch.Tensor:
    """the nearest point of the int8 grid k * scale, |k| <= 127 (exact in fp32 for a power-of-two scale)"""
    return (t / scale).round().clamp(-127, 127) * scale


def put_q8(out: dict, key: str, t: torch.Tensor, scale: float) -> None:
    k = (t / scale).round()
    assert torch.equal(k * scale, t) and k.abs().max() <= 127, f"{key} is not on its int8 grid"
    out["q8:" + key] = k.to(torch.int8).numpy()
    out["q8s:" + key] = np.float64(scale)


def put_i16(out: dict, key: str, t: torch.Tensor) -> None:
    assert t.abs().max() < 2 ** 15
    out["i16:" + key] = t.to(torch.int16).numpy()


def put_f(out: dict, key: str, t: torch.Tensor, limit: int = SAMPLE) -> None:
    t = t.detach().float()
    if t.numel() <= limit:
        out[key] = t.numpy()
        return
    stride = -(-t.numel() // limit)
    out[key + "@s"] = t.reshape(-1)[::stride].clone().numpy()
    out[key + "@stride"] = np.int64(stride)
    out[key + "@rows"] = t.double().sum(-1).float().numpy()


class Compact:
    def __init__(self, sample, stride, rows):
        self.sample, self.stride, self.rows = sample, stride, rows


def load(path: str) -> dict:
    """key -> fp32 / int64 tensor (q8, i16, whole results) or Compact (sampled results)"""
    z = np.load(path)
    d = {}
    for k in z.files:
        if k.startswith("q8:"):
            d[k[3:]] = torch.from_numpy(z[k].astype(np.float32) * np.float32(z["q8s:" + k[3:]]))
        elif k.startswith("i16:"):
            d[k[4:]] = torch.from_numpy(z[k].astype(np.int64))
        elif k.endswith("@s"):
            b = k[:-2]
            d[b] = Compact(torch.from_numpy(z[k]), int(z[b + "@stride"]), torch.from_numpy(z[b + "@rows"]))
        elif not (k.startswith("q8s:") or k.endswith("@stride") or k.endswith("@rows")):
            d[k] = torch.from_numpy(z[k])
    return d


def group(d: dict, prefix: str) -> dict:
    return {k[len(prefix) + 1:]: v for k, v in d.items() if k.startswith(prefix + "/")}


def check(name: str, got: torch.Tensor, want, tol: float) -> float:
    """assert_close against a whole result, or against the sample and the row sums of a sampled one"""
    if not isinstance(want, Compact):
        return assert_close(name, got, want, tol)
    g = got.detach().float().cpu()
    e = assert_close(name + "@sample", g.reshape(-1)[::want.stride], want.sample, tol)
    rows = g.double().sum(-1).float()
    return max(e, assert_close(name + "@rows", rows, want.rows, tol))
