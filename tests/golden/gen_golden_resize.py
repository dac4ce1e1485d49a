"""Regenerate tests/golden/resize_bicubic.npz: uint8 sources and Pillow's bicubic resize of each (what
`transforms.Resize(S, BICUBIC)` does to the reference's PIL images), one image per case.

    python tests/golden/gen_golden_resize.py
"""
import os

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [("96_224_c3", 96, 224, 3), ("32_224_c3", 32, 224, 3), ("96_384_c3", 96, 384, 3), ("40_32_c3", 40, 32, 3),
         ("96_224_c1", 96, 224, 1)]


def main():
    rng = np.random.default_rng(20261016)
    arrays = {"pillow_version": np.array(PIL.__version__)}
    for name, n, s, c in CASES:
        src = rng.integers(0, 256, (n, n, c), dtype=np.uint8)
        im = Image.fromarray(src[..., 0] if c == 1 else src)
        out = np.asarray(im.resize((s, s), Image.BICUBIC)).reshape(s, s, c)
        arrays[f"src_{name}"] = src
        arrays[f"out_{name}"] = out
    path = os.path.join(HERE, "resize_bicubic.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
