"""vitmi_resize_ingest and vitmi_resize_ingest_patchify at B = 256 on STL-10-sized sources (96x96x3 resized to 224 and
384), beside vitmi_image_ingest at 224x224 (no resize) in the same process.  Device events after warm-up, median of 20
launches, each preceded by a 512 MB write that flushes the caches; bytes = uint8 in + output."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vit_torch_amd import ops  # noqa: E402
from vit_torch_amd.data import NORM, DeviceAugment  # noqa: E402

B = 256
P = 16


def timed(fn, flush, reps=20):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(reps):
        flush.zero_()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def main():
    g = torch.Generator("cpu").manual_seed(0)
    flush = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")
    cases = []

    src224 = torch.randint(0, 256, (B, 224, 224, 3), generator=g, dtype=torch.uint8).cuda()
    plain = DeviceAugment(224, **NORM["stl10"], train=True, generator=g)
    oy, ox, fl = plain.draw(B, 224, 224)
    out = torch.empty((B, 3, 224, 224), device="cuda")
    cases.append(("image_ingest 224->224 fp32 NCHW", src224.numel(), out.numel() * 4,
                  lambda: ops.image_ingest(src224, out, oy, ox, fl, plain.mean, plain.std, plain.pad)))

    src96 = torch.randint(0, 256, (B, 96, 96, 3), generator=g, dtype=torch.uint8).cuda()
    for S in (224, 384):
        aug = DeviceAugment(S, **NORM["stl10"], train=True, generator=g, resize=True)
        aug.prepare(96, 96)
        t = aug._tables[96]
        ry, rx, rf = aug.draw(B, 96, 96)
        dst = torch.empty((B, 3, S, S), device="cuda")
        gq = S // P
        rows = torch.empty((B * (1 + gq * gq), 3 * P * P), dtype=torch.bfloat16, device="cuda")
        cases.append((f"resize_ingest 96->{S} fp32 NCHW", src96.numel(), dst.numel() * 4,
                      lambda a=aug, t=t, d=dst, y=ry, x=rx, f=rf:
                      ops.resize_ingest(src96, d, t, t, y, x, f, a.mean, a.std, a.pad)))
        cases.append((f"resize_ingest_patchify 96->{S} bf16 p{P}", src96.numel(), rows.numel() * 2,
                      lambda a=aug, t=t, r=rows, y=ry, x=rx, f=rf, S=S:
                      ops.resize_ingest_patchify(src96, r, t, t, y, x, f, a.mean, a.std, S, a.pad, P, 1)))

    print(f"B = {B}; median (min) of 20 launches after a cache flush")
    print(f"{'kernel':42s} {'MB in':>8s} {'MB out':>8s} {'us':>8s} {'min us':>8s} {'TB/s':>6s}")
    for name, nin, nout, fn in cases:
        med, lo = timed(fn, flush)
        print(f"{name:42s} {nin / 1e6:8.2f} {nout / 1e6:8.1f} {med:8.1f} {lo:8.1f} {(nin + nout) / med / 1e6:6.2f}")


if __name__ == "__main__":
    main()
