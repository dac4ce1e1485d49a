"""DINO introspection on one MI355X: ops.attn_probs alone (us per call and the effective write rate, 4 B H N^2 bytes of
P per call) at the vitb8 / 224 px shape (B 64, H 12, N 785) and the vits16 / 224 px shape (B 256, H 6, N 197) in bf16
and fp32, then get_intermediate_layers(x, 1) against forward under torch.no_grad() for dino_vitb16 at batch 256.

    python tools/attn_probs_bench.py ops     # one JSON line per (shape, dtype)
    python tools/attn_probs_bench.py model   # one JSON line: forward / get_intermediate_layers / get_last_selfattention ms

Run each part under its own time limit (timeout -k 10 <s> python tools/attn_probs_bench.py ...)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402


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


def ops_leg():
    from vit_torch_amd import ops
    hd = 64
    for name, B, H, N in (("vitb8_224", 64, 12, 785), ("vits16_224", 256, 6, 197)):
        for dt in (torch.bfloat16, torch.float32):
            g = torch.Generator("cuda").manual_seed(0)
            qkv = torch.randn(B * N, 3 * H * hd, device="cuda", generator=g).to(dt)
            P = torch.empty((B, H, N, N), dtype=torch.float32, device="cuda")
            us = _time(lambda: ops.attn_probs(qkv, P, B, N, H, hd, hd ** -0.5))
            nbytes = 4.0 * B * H * N * N
            print(json.dumps(dict(shape=name, dtype=str(dt).split(".")[-1], B=B, H=H, N=N, us=round(us, 1),
                                  write_GB=round(nbytes / 1e9, 3), write_TBps=round(nbytes / us / 1e6, 2))), flush=True)
            del qkv, P


def model_leg(B=256):
    from vit_torch_amd import VisionModelZoo
    m = VisionModelZoo.get_model("dino_vitb16", pretrained=False).cuda()
    x = torch.randn(B, 3, 224, 224, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    with torch.no_grad():
        fwd = _time(lambda: m(x), iters=10)
        inter = _time(lambda: m.get_intermediate_layers(x, 1), iters=10)
        attn = _time(lambda: m.get_last_selfattention(x), iters=10)
    print(json.dumps(dict(arch="dino_vitb16", batch=B, forward_ms=round(fwd / 1e3, 3),
                          intermediate_layers_1_ms=round(inter / 1e3, 3), last_selfattention_ms=round(attn / 1e3, 3),
                          intermediate_over_forward=round(inter / fwd, 4))), flush=True)


if __name__ == "__main__":
    leg = sys.argv[1] if len(sys.argv) > 1 else "ops"
    {"ops": ops_leg, "model": model_leg}[leg]()
