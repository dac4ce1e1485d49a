"""CaiT at 384 / 448 pixels on one MI355X: per-layer talking-heads attention forward / backward us of the bf16 long op
(ops.th_long_fwd / _bwd) at the cait_S24, cait_M36 and cait_M48 shapes, the XXS _224 shape on the long op against the
three-call form at batch 256, and images/s + peak memory of a full bf16 training step.

    python tools/cait_long_bench.py ops              # per-layer us, one JSON line per shape
    python tools/cait_long_bench.py step ARCH BATCH  # one model: images/s, torch.cuda.max_memory_allocated

Run each part under its own time limit (timeout -k 10 <s> python tools/cait_long_bench.py ...)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

HD = 48


def _time(fn, iters=10, warm=3):
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
    bt, f32 = torch.bfloat16, torch.float32
    for name, B, H, N in (("cait_S24", 64, 8, 576), ("cait_M36", 64, 16, 576), ("cait_M48", 32, 16, 784),
                          ("cait_XXS24_224", 256, 4, 196)):
        D = H * HD
        g = torch.Generator("cuda").manual_seed(0)
        qkv = (torch.randn(B * N, 3 * D, device="cuda", generator=g) * 0.5).to(bt)
        dO = torch.randn(B * N, D, device="cuda", generator=g).to(bt)
        W = [torch.eye(H, device="cuda") + 0.1, torch.zeros(H, device="cuda"), torch.eye(H, device="cuda"),
             torch.zeros(H, device="cuda")]
        O, dqkv = torch.empty(B * N, D, device="cuda", dtype=bt), torch.empty(B * N, 3 * D, device="cuda", dtype=bt)
        gr = [torch.empty(H, H, device="cuda"), torch.empty(H, device="cuda"), torch.empty(H, H, device="cuda"),
              torch.empty(H, device="cuda")]
        sc = HD ** -0.5
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fwd = _time(lambda: ops.th_long_fwd(qkv, *W, O, B, H, N, HD, sc))
        bwd = _time(lambda: ops.th_long_bwd(qkv, dO, *W, dqkv, *gr, B, H, N, HD, sc))
        peak = torch.cuda.max_memory_allocated() - base
        rec = dict(shape=name, B=B, H=H, N=N, long_fwd_us=round(fwd, 1), long_bwd_us=round(bwd, 1),
                   long_peak_transient_MB=round(peak / 2**20, 1))
        if N <= 256:                          # the three-call form keeps S, P, P' instead of recomputing them
            NS = (N + 7) // 8 * 8
            kept = {}

            def f3():
                kept["t"] = ops.th_three_call_fwd(qkv, *W, O, B, H, N, HD, sc, NS)

            fwd3 = _time(f3)
            S, P, Pm = kept["t"]
            bwd3 = _time(lambda: ops.th_three_call_bwd(qkv, dO, S, P, Pm, W[0], W[2], dqkv, *gr, B, H, N, HD, sc, NS))
            rec.update(three_call_fwd_us=round(fwd3, 1), three_call_bwd_us=round(bwd3, 1))
        print(json.dumps(rec), flush=True)
        del qkv, dO, O, dqkv
        torch.cuda.empty_cache()


def step_leg(arch, batch, steps=5):
    from vit_torch_amd import CrossEntropyLoss, FusedSGD, VisionModelZoo
    from vit_torch_amd.cait import VARIANTS
    img = VARIANTS[arch][0]
    m = VisionModelZoo.get_model(arch, pretrained=False, classifier=None, compute_dtype="bf16").cuda()
    opt = FusedSGD(m.parameters(), lr=1e-3, momentum=0.9)
    crit = CrossEntropyLoss()
    g = torch.Generator("cuda").manual_seed(0)
    x = torch.randn(batch, 3, img, img, device="cuda", generator=g)
    y = torch.randint(0, 1000, (batch,), device="cuda", generator=g)
    losses = []

    def one():
        opt.zero_grad()
        loss = crit(m(x), y)
        loss.backward()
        opt.step()
        losses.append(loss)

    torch.cuda.reset_peak_memory_stats()
    us = _time(one, iters=steps, warm=2)
    loss = losses[-1].item()
    print(json.dumps(dict(arch=arch, batch=batch, img=img, ms_per_step=round(us / 1000, 2),
                          images_per_s=round(batch / (us * 1e-6), 1),
                          max_memory_allocated_GB=round(torch.cuda.max_memory_allocated() / 2**30, 2),
                          loss=round(loss, 4), finite=bool(torch.isfinite(torch.tensor(loss))))), flush=True)


if __name__ == "__main__":
    if sys.argv[1] == "ops":
        ops_leg()
    else:
        step_leg(sys.argv[2], int(sys.argv[3]))
