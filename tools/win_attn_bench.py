"""Window-12 attention kernels at the four Swin-B/384 stage shapes (batch 64 by default): forward and backward
microseconds of the MFMA path and of the fp32 vector path, each against its floor max(FLOP / peak, HBM bytes /
bandwidth).  FLOP: forward 4 N^2 hd per (window, head), backward 2.5x that.  HBM bytes: qkv, O, dO, dqkv in bf16
and lse in fp32.  The fp32 bias [H,N,N] and shift mask [nW,N,N] are read once per (window, head) from L2 and are
reported separately (their per-launch L2 bytes), not counted in the floor.

    python tools/win_attn_bench.py [--batch 64] [--iters 20]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vit_torch_amd import _lib, ops  # noqa: E402

PEAK_BF16 = 2.5e15       # dense bf16 MFMA, MI355X spec
PEAK_F32 = 157.3e12      # fp32 vector, MI355X spec
HBM = 6.3e12             # achievable HBM3E copy rate

# stage: (grid, C, heads)
STAGES = [(96, 128, 4), (48, 256, 8), (24, 512, 16), (12, 1024, 32)]


def timed(fn, iters):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    from oracle.swin_ref import shift_attn_mask
    lib = _lib.load()
    ws = 12
    N = ws * ws
    B = a.batch
    for si, (R, C, H) in enumerate(STAGES):
        hd = C // H
        shift = ws // 2 if R > ws else 0
        L = R * R
        nW = (R // ws) ** 2
        Bw = B * nW
        scale = hd ** -0.5
        qkv = (torch.randn(B, L, 3 * C, device="cuda") * 0.5).to(torch.bfloat16)
        do = torch.randn(B, L, C, device="cuda").to(torch.bfloat16)
        O = torch.empty_like(do)
        lse = torch.empty(Bw * H * N, device="cuda")
        bias = torch.randn(H * N * N, device="cuda") * 0.1
        mask = shift_attn_mask(R, R, ws, shift).cuda().contiguous() if shift else None
        dqkv = torch.empty_like(qkv)
        dbias = torch.empty(H * N * N, device="cuda")
        qb = torch.empty(3 * C, device="cuda")
        fl_f = 4.0 * N * N * hd * Bw * H
        by_f = (B * L * 3 * C + B * L * C) * 2 + Bw * H * N * 4
        by_b = (B * L * 3 * C * 2 + B * L * C) * 2 + Bw * H * N * 4
        l2 = Bw * H * N * N * 4 * (2 if mask is not None else 1)
        print(f"stage {si + 1}: {R}x{R} C {C} H {H} hd {hd} shift {shift} Bw {Bw}; bias+mask L2 reads "
              f"{l2 / 1e6:.0f} MB per launch")
        for mfma in (1, 0):
            lib.vitmi_debug_win_attn_mfma(mfma)
            fuse = ops.win_attn_bwd_fuses_qkv_bias(qkv, hd)
            peak = PEAK_BF16 if mfma else PEAK_F32
            tf = timed(lambda: ops.win_attn_fwd(qkv, O, lse, bias, mask, Bw, H, N, hd, R, R, ws, shift, scale), a.iters)
            tb = timed(lambda: ops.win_attn_bwd(qkv, do, lse, bias, mask, dqkv, dbias, Bw, H, N, hd, R, R, ws, shift,
                                                scale, dqkv_bias=qb if fuse else None), a.iters)
            ff = max(fl_f / peak, by_f / HBM) * 1e6
            fb = max(2.5 * fl_f / peak, by_b / HBM) * 1e6
            name = "mfma  " if mfma else "vector"
            print(f"  {name} fwd {tf:9.1f} us (floor {ff:7.1f}, {ff / tf * 100:5.1f} %)   "
                  f"bwd {tb:9.1f} us (floor {fb:7.1f}, {fb / tb * 100:5.1f} %)")
        lib.vitmi_debug_win_attn_mfma(-1)


if __name__ == "__main__":
    main()
