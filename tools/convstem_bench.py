"""XCiT's ConvPatchEmbed on one MI355X: the library's path (ops.conv3s2_im2col + ops.gemm + ops.bn_act_fwd / _bwd +
ops.conv3s2_col2im, as vit_torch_amd.ConvPatchEmbed runs them) in bf16, training mode, forward and backward, with the time of
each kernel family (gather, GEMM, bn_act, col2im) summed over the stages and the module's total, beside the PyTorch
composition of the reference's models/xcit.py:58-108 (nn.Conv2d + nn.BatchNorm2d + nn.GELU, bf16, channels_last; forward, and
forward + autograd backward) on the same device.  20 timed calls after 3.  No pass / fail threshold.

    python tools/convstem_bench.py        # one JSON line per shape

Run under a time limit (timeout -k 10 <s> python tools/convstem_bench.py)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

SHAPES = [(256, 224, 16, 384), (256, 224, 16, 768), (64, 224, 8, 384)]      # batch, image, patch, embed_dim


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


def composed(E, patch):
    ch = [3] + [E // f for f in ((8, 4, 2, 1) if patch == 16 else (4, 2, 1))]
    layers = []
    for k, (ci, co) in enumerate(zip(ch[:-1], ch[1:])):
        if k:
            layers.append(nn.GELU())
        layers += [nn.Conv2d(ci, co, 3, stride=2, padding=1, bias=False), nn.BatchNorm2d(co)]
    return nn.Sequential(*layers).cuda().to(torch.bfloat16).to(memory_format=torch.channels_last).train()


def per_kernel(m, x):
    """us of each kernel family over the stages, on the tensors of one forward (bf16, training mode)"""
    from vit_torch_amd import ops, xcit
    bf, pk = torch.bfloat16, m.pack
    t = dict(gather_fwd=0.0, gemm_fwd=0.0, bn_act_fwd=0.0, bn_act_bwd=0.0, gather_bwd=0.0, gemm_dw=0.0, gemm_dcol=0.0, col2im=0.0)
    stages, B, (h, w), cur = xcit._conv_stages(m), x.shape[0], x.shape[2:], x
    for s, (conv, bn) in enumerate(stages):
        co, ci = conv.weight.shape[:2]
        ho, wo = (h + 1) // 2, (w + 1) // 2
        M, K, gelu = B * ho * wo, (9 * ci if s else 32), s + 1 < len(stages)
        col, y, out = (torch.empty(sh, dtype=bf, device="cuda") for sh in ((M, K), (M, co), (B, ho * wo, co)))
        dy, dout = torch.empty_like(y), torch.randn((M, co), device="cuda").to(bf)
        stat = torch.empty((2, co), dtype=torch.float32, device="cuda")
        wk = xcit._conv_weight(pk, conv, s)
        g = t["gather_fwd"]
        t["gather_fwd"] += _time(lambda: ops.conv3s2_im2col(cur, col, B, h, w, ci))
        t["gather_bwd"] += t["gather_fwd"] - g                      # the backward rebuilds col with the same call
        t["gemm_fwd"] += _time(lambda: ops.gemm(col, wk, y))
        t["bn_act_fwd"] += _time(lambda: ops.bn_act_fwd(y, pk.f32(bn.weight), pk.f32(bn.bias), bn.running_mean, bn.running_var,
                                                        bn.num_batches_tracked, stat, out, M, co, gelu=gelu, training=True))
        t["bn_act_bwd"] += _time(lambda: ops.bn_act_bwd(dout, y, stat, pk.f32(bn.weight), pk.f32(bn.bias), dy, pk.g(bn.weight),
                                                        pk.g(bn.bias), M, co, gelu=gelu, training=True))
        gw = torch.empty((co, K), dtype=torch.float32, device="cuda")
        t["gemm_dw"] += _time(lambda: ops.gemm(dy, col, gw, a_kmajor=False, b_kmajor=False))
        if s:
            dx = torch.empty((B, h * w, ci), dtype=bf, device="cuda")
            t["gemm_dcol"] += _time(lambda: ops.gemm(dy, wk, col, b_kmajor=False))
            t["col2im"] += _time(lambda: ops.conv3s2_col2im(col, dx, B, h, w, ci))
        cur, h, w = out, ho, wo
        del col, y, dy, dout
    return {k: round(v, 1) for k, v in t.items()}


def main():
    from vit_torch_amd import ConvPatchEmbed
    for B, S, patch, E in SHAPES:
        g = torch.Generator("cuda").manual_seed(0)
        x = torch.randn((B, 3, S, S), device="cuda", generator=g)
        m = ConvPatchEmbed(S, patch, 3, E, compute_dtype="bf16").cuda().train()
        n = (S // patch) ** 2
        dout = torch.randn((B, n, E), device="cuda", generator=g)
        with torch.no_grad():
            fwd = _time(lambda: m(x))

        def both():
            for p in m.parameters():
                p.grad = None
            m(x)[0].backward(dout)
        fb = _time(both)
        kern = per_kernel(m, x)
        ref = composed(E, patch)
        xb = x.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        db = dout.to(torch.bfloat16).transpose(1, 2).reshape(B, E, S // patch, S // patch).contiguous(memory_format=torch.channels_last)
        with torch.no_grad():
            cf = _time(lambda: ref(xb))

        def cboth():
            for p in ref.parameters():
                p.grad = None
            ref(xb).backward(db)
        cfb = _time(cboth)
        print(json.dumps(dict(B=B, img=S, patch=patch, E=E, fwd_us=round(fwd, 1), fwd_bwd_us=round(fb, 1), kernels_us=kern,
                              composed_fwd_us=round(cf, 1), composed_fwd_bwd_us=round(cfb, 1),
                              fwd_speedup=round(cf / fwd, 2), fwd_bwd_speedup=round(cfb / fb, 2))), flush=True)
        del x, dout, m, ref, xb, db


if __name__ == "__main__":
    main()
