"""XCiT's cross-covariance attention on one MI355X: ops.xca_fwd and ops.xca_bwd alone (us per call and the achieved rate
against the bytes the op has to move: forward qkv + out, backward qkv + dqkv + dout once), in bf16, beside the PyTorch
composition of the reference's models/xcit.py:243-254 (forward, and forward + autograd backward minus forward) on the same
tensors and device.

    python tools/xca_bench.py        # one JSON line per shape

Run under a time limit (timeout -k 10 <s> python tools/xca_bench.py)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

SHAPES = [(256, 196, 8, 48), (256, 196, 16, 48), (64, 784, 8, 48), (32, 2304, 4, 32)]


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


def composed(qkv, temperature, B, N, H, hd):
    q, k, v = qkv.reshape(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)
    q, k, v = q.transpose(-2, -1), k.transpose(-2, -1), v.transpose(-2, -1)
    q = torch.nn.functional.normalize(q, dim=-1)
    k = torch.nn.functional.normalize(k, dim=-1)
    attn = ((q @ k.transpose(-2, -1)) * temperature).softmax(dim=-1)
    return (attn @ v).permute(0, 3, 1, 2).reshape(B, N, H * hd)


def main():
    from vit_torch_amd import ops
    for B, N, H, hd in SHAPES:
        g = torch.Generator("cuda").manual_seed(0)
        qkv = torch.randn(B * N, 3 * H * hd, device="cuda", generator=g).bfloat16()
        dout = torch.randn(B, N, H * hd, device="cuda", generator=g).bfloat16()
        temp = torch.linspace(0.5, 2.0, H, device="cuda")
        out, dqkv = torch.empty_like(dout), torch.empty_like(qkv)
        stat = torch.empty((B, H, hd + 2, hd), dtype=torch.float32, device="cuda")
        dtemp = torch.empty(H, dtype=torch.float32, device="cuda")
        fwd = _time(lambda: ops.xca_fwd(qkv, temp, out, stat, B, N, H, hd))
        bwd = _time(lambda: ops.xca_bwd(qkv, dout, temp, stat, dqkv, dtemp, B, N, H, hd))
        tok = 2.0 * B * N * H * hd                       # bytes of one [B, N, H*hd] bf16 tensor
        fb, bb = 4 * tok, 7 * tok
        qa = qkv.clone().requires_grad_(True)
        ta = temp.reshape(H, 1, 1).bfloat16()
        with torch.no_grad():
            cf = _time(lambda: composed(qkv, ta, B, N, H, hd))

        def both():
            qa.grad = None
            composed(qa, ta, B, N, H, hd).backward(dout)
        cfb = _time(both)
        print(json.dumps(dict(B=B, N=N, H=H, hd=hd, fwd_us=round(fwd, 1), fwd_TBps=round(fb / fwd / 1e6, 2),
                              bwd_us=round(bwd, 1), bwd_TBps=round(bb / bwd / 1e6, 2), composed_fwd_us=round(cf, 1),
                              composed_bwd_us=round(cfb - cf, 1), fwd_speedup=round(cf / fwd, 1),
                              bwd_speedup=round((cfb - cf) / bwd, 1))), flush=True)
        del qkv, dout, out, dqkv, qa


if __name__ == "__main__":
    main()
