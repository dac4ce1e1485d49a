"""Device-side input pipeline.

The reference transforms every sample on CPU DataLoader workers
(/root/reference/utils_datasets.py:553-582: `RandomCrop(S, padding=max(2, S//12), fill=128)`,
`RandomHorizontalFlip`, `ToTensor`, `Normalize(mean, std)`; test: `ToTensor`, `Normalize`).
`DeviceAugment` takes the raw uint8 NHWC batch on the GPU and produces the normalised fp32
NCHW tensor in one kernel; the per-sample crop offsets and flip flags are drawn with a torch
generator (pass them explicitly to pin a batch).

`DeviceAugment(S, ..., resize=True)` adds the reference's resize: when the stored (square) image size differs from S,
the chain is `Resize(S, BICUBIC)` first (utils_datasets.py:553-582, `resize=image_size != cls.image_size` at :615-620),
and the crop offsets are drawn over the resized, padded S x S image.  The resize is Pillow's, bit-exact
(`vitmi_resize_ingest`, coefficient tables from `vit_torch_amd.resize`, cached per source size on the device; call
`prepare(H, W)` before capturing a graph).  When the stored size already equals S nothing is resized and the call is
the plain kernel's, bit for bit.  `resize=False` (the default) crops the stored image as it is.

`DeviceAugment.patch_rows(images, patch_size, dtype)` goes one step further (round 3): the same
transform written straight into the patch rows the patch-embedding GEMM contracts
(`vitmi_ingest_patchify`: uint8 NHWC -> bf16 patch rows in one pass, no fp32 NCHW intermediate); the
returned `PatchRows` is accepted by `VisionTransformer.forward` in place of the image tensor; with `resize=True` it is
`vitmi_resize_ingest_patchify`, the resized transform written straight into the patch rows.
"""
from __future__ import annotations

import torch

from . import ops
from . import resize as _resize
from ._lib import VitmiError

NORM = {   # utils_datasets.py:586-589 (STL-10), :644-647 (CIFAR-10)
    "stl10": dict(mean=[0.44671062065972217, 0.43980983983523964, 0.40664644709967324],
                  std=[0.2603409782662331, 0.25657727311344447, 0.27126738145225493]),
    "cifar10": dict(mean=[0.4914, 0.4822, 0.4465], std=[0.247, 0.243, 0.261]),
}


class DeviceAugment:
    def __init__(self, image_size: int, mean=None, std=None, train: bool = True, device="cuda", generator=None,
                 resize: bool = False):
        self.S = int(image_size)
        self.pad = max(2, self.S // 12) if train else 0          # utils_datasets.py:567
        self.train = train
        self.device = torch.device(device)
        self.mean = torch.tensor(mean, dtype=torch.float32, device=self.device) if mean is not None else None
        self.std = torch.tensor(std, dtype=torch.float32, device=self.device) if std is not None else None
        self.generator = generator
        self.resize = bool(resize)
        self._tables = {}                                         # source size -> resize coefficient table (device)

    def _resizes(self, H, W) -> bool:
        if not self.resize:
            return False
        if H != W:
            raise VitmiError(f"DeviceAugment(resize=True) takes square images only (got {H}x{W})")
        return H != self.S

    def prepare(self, H: int, W: int) -> None:
        """Build the resize tables for H x W sources ahead of time (needed before a graph capture)."""
        if self._resizes(H, W) and H not in self._tables:
            self._tables[H] = _resize.table(H, self.S, self.device)

    def _table(self, H):
        t = self._tables.get(H)
        if t is None:
            if torch.cuda.is_current_stream_capturing():
                raise VitmiError(f"DeviceAugment: no resize tables for {H}x{H} sources inside a stream capture; call "
                                 f"prepare({H}, {H}) before capturing")
            self.prepare(H, H)
            t = self._tables[H]
        return t

    def draw(self, B, H, W):
        """(off_y, off_x, flip) as torchvision draws them: top-left uniform in [0, H+2p-S], flip p=0.5 (H, W of the
        resized image when this augment resizes)."""
        if not self.train:
            return None, None, None
        if self._resizes(H, W):
            H = W = self.S
        g = self.generator
        oy = torch.randint(0, H + 2 * self.pad - self.S + 1, (B,), generator=g, dtype=torch.int32)
        ox = torch.randint(0, W + 2 * self.pad - self.S + 1, (B,), generator=g, dtype=torch.int32)
        fl = (torch.rand(B, generator=g) < 0.5).to(torch.uint8)
        return oy.to(self.device), ox.to(self.device), fl.to(self.device)

    def __call__(self, images_u8_nhwc, off_y=None, off_x=None, flip=None):
        x = images_u8_nhwc
        if not x.is_cuda:
            x = x.to(self.device, non_blocking=True)
        B, H, W, C = x.shape
        if self.train and off_y is None:
            off_y, off_x, flip = self.draw(B, H, W)
        out = torch.empty((B, C, self.S, self.S), dtype=torch.float32, device=x.device)
        if self._resizes(H, W):
            t = self._table(H)
            return ops.resize_ingest(x.contiguous(), out, t, t, off_y, off_x, flip, self.mean, self.std, self.pad)
        return ops.image_ingest(x.contiguous(), out, off_y, off_x, flip, self.mean, self.std, self.pad)

    def patch_rows(self, images_u8_nhwc, patch_size: int, dtype=torch.bfloat16, cls_rows: int = 1,
                   off_y=None, off_x=None, flip=None) -> "PatchRows":
        x = images_u8_nhwc
        if not x.is_cuda:
            x = x.to(self.device, non_blocking=True)
        B, H, W, C = x.shape
        if self.train and off_y is None:
            off_y, off_x, flip = self.draw(B, H, W)
        g = self.S // patch_size
        rows = torch.empty((B * (cls_rows + g * g), C * patch_size * patch_size), dtype=dtype, device=x.device)
        if self._resizes(H, W):
            t = self._table(H)
            ops.resize_ingest_patchify(x.contiguous(), rows, t, t, off_y, off_x, flip, self.mean, self.std, self.S,
                                       self.pad, patch_size, cls_rows)
        else:
            ops.ingest_patchify(x.contiguous(), rows, off_y, off_x, flip, self.mean, self.std, self.S, self.pad,
                                patch_size, cls_rows)
        return PatchRows(rows, B, C, self.S, self.S, patch_size, cls_rows)


class PatchRows:
    """A batch already in patch-row form ([B*(cls_rows + gh*gw), C*p*p], the GEMM operand dtype): what
    `VisionTransformer.forward` takes instead of an fp32 [B,C,H,W] tensor when the input pipeline runs on
    the device (the engine then skips its own patch gather)."""
    is_cuda = True

    def __init__(self, rows, B, C, H, W, p, cls_rows):
        self.rows, self.B, self.C, self.H, self.W, self.p, self.cls_rows = rows, B, C, H, W, p, cls_rows
        self.device = rows.device
