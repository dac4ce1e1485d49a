"""XCiT's local patch interaction on one MI355X: ops.lpi_fwd and ops.lpi_bwd alone in training mode (us per call and the
achieved rate against the bytes DESIGN.md 4.6 counts: forward 4 T, backward 8 T, T one [B, H*W, C] bf16 tensor), in bf16,
beside the PyTorch composition of the reference's models/xcit.py:133-141 (permute to NCHW, depthwise conv, GELU, batch
norm, depthwise conv, permute back; forward, and forward + autograd backward minus forward) on the same tensors and device.
No pass / fail threshold.

    python tools/lpi_bench.py        # one JSON line per shape

Run under a time limit (timeout -k 10 <s> python tools/lpi_bench.py)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

SHAPES = [(256, 14, 14, 384), (256, 14, 14, 768), (64, 28, 28, 384), (32, 48, 48, 192)]
FWD_T, BWD_T = 4, 8


def _time(fn, iters=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / iters


def composed(x, p, rm, rv, B, H, W, C):
    t = x.permute(0, 2, 1).reshape(B, C, H, W)
    t = F.conv2d(t, p["w1"], p["b1"], padding=1, groups=C)
    t = F.gelu(t)
    t = F.batch_norm(t, rm, rv, p["gamma"], p["beta"], True, 0.1, 1e-5)
    t = F.conv2d(t, p["w2"], p["b2"], padding=1, groups=C)
    return t.reshape(B, C, H * W).permute(0, 2, 1)


def main():
    from vit_torch_amd import ops
    for B, H, W, C in SHAPES:
        g = torch.Generator("cuda").manual_seed(0)

        def rnd(*shape, scale=1.0):
            return torch.randn(*shape, device="cuda", generator=g) * scale
        x, dout = rnd(B, H * W, C).bfloat16(), rnd(B, H * W, C).bfloat16()
        p = dict(w1=rnd(C, 1, 3, 3, scale=0.3), b1=rnd(C, scale=0.2), gamma=1 + rnd(C, scale=0.1), beta=rnd(C, scale=0.2),
                 w2=rnd(C, 1, 3, 3, scale=0.3), b2=rnd(C, scale=0.2))
        rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
        nbt = torch.zeros(1, dtype=torch.int64, device="cuda")
        u, out, dx = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
        stat = torch.empty((2, C), dtype=torch.float32, device="cuda")
        gr = {k: torch.empty_like(v) for k, v in p.items()}
        fwd = _time(lambda: ops.lpi_fwd(x, p["w1"], p["b1"], p["gamma"], p["beta"], p["w2"], p["b2"], rm, rv, nbt, u, stat, out,
                                        B, H, W, C, training=True))
        bwd = _time(lambda: ops.lpi_bwd(x, u, dout, stat, p["w1"], p["b1"], p["gamma"], p["beta"], p["w2"], dx, gr["w1"],
                                        gr["b1"], gr["gamma"], gr["beta"], gr["w2"], gr["b2"], B, H, W, C, training=True))
        T = 2.0 * B * H * W * C                          # bytes of one [B, H*W, C] bf16 tensor
        pb = {k: v.bfloat16().requires_grad_(True) for k, v in p.items()}
        xa = x.clone().requires_grad_(True)
        rmb, rvb = rm.bfloat16(), rv.bfloat16()
        with torch.no_grad():
            cf = _time(lambda: composed(x, pb, rmb, rvb, B, H, W, C))

        def both():
            xa.grad = None
            for v in pb.values():
                v.grad = None
            composed(xa, pb, rmb, rvb, B, H, W, C).backward(dout)
        cfb = _time(both)
        print(json.dumps(dict(B=B, H=H, W=W, C=C, fwd_us=round(fwd, 1), fwd_TBps=round(FWD_T * T / fwd / 1e6, 2),
                              bwd_us=round(bwd, 1), bwd_TBps=round(BWD_T * T / bwd / 1e6, 2), composed_fwd_us=round(cf, 1),
                              composed_bwd_us=round(cfb - cf, 1), fwd_speedup=round(cf / fwd, 1),
                              bwd_speedup=round((cfb - cf) / bwd, 1))), flush=True)
        del x, dout, u, out, dx, xa


if __name__ == "__main__":
    main()
