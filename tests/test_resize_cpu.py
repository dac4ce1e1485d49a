"""Pillow's bicubic resize coefficients (vit_torch_amd/resize.py) and the int64 restatement of its two passes
(tests/resize_util.py), against the committed Pillow fixture and, where Pillow is importable, live Pillow."""
import os

import numpy as np
import pytest
import torch

from tests.resize_util import resize_u8

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resize_bicubic.npz")
CASES = ["96_224_c3", "32_224_c3", "96_384_c3", "40_32_c3", "96_224_c1"]


@pytest.mark.parametrize("name", CASES)
def test_tables_and_restatement_equal_the_fixture(name):
    from vit_torch_amd import resize
    z = np.load(GOLDEN)
    src, want = z[f"src_{name}"], z[f"out_{name}"]
    n, s = src.shape[0], want.shape[0]
    t = resize.table(n, s)
    got = resize_u8(torch.from_numpy(src)[None], t, t)[0].numpy()
    assert got.shape == want.shape and np.array_equal(got, want), np.abs(got.astype(int) - want).max()


SWEEP = [(96, 224), (96, 384), (32, 224), (40, 32), (96, 37), (97, 13), (31, 211), (17, 50), (23, 7), (13, 13 * 7 + 2),
         (101, 67), (64, 31), (7, 3), (3, 29), (120, 17)]


@pytest.mark.parametrize("n,s", SWEEP)
@pytest.mark.parametrize("c", [1, 3])
def test_live_pillow_sweep(n, s, c):
    Image = pytest.importorskip("PIL.Image")
    from vit_torch_amd import resize
    src = np.random.default_rng(n * 1000 + s + c).integers(0, 256, (n, n, c), dtype=np.uint8)
    want = np.asarray(Image.fromarray(src[..., 0] if c == 1 else src).resize((s, s), Image.BICUBIC)).reshape(s, s, c)
    t = resize.table(n, s)
    got = resize_u8(torch.from_numpy(src)[None], t, t)[0].numpy()
    assert np.array_equal(got, want), np.abs(got.astype(int) - want).max()


def test_live_pillow_non_square_tables():
    """The per-axis tables are independent: a non-square 17x23 -> 50x9 resize matches too (the device pipeline itself
    takes square sources only)."""
    Image = pytest.importorskip("PIL.Image")
    from vit_torch_amd import resize
    src = np.random.default_rng(5).integers(0, 256, (17, 23, 3), dtype=np.uint8)
    want = np.asarray(Image.fromarray(src).resize((9, 50), Image.BICUBIC))
    got = resize_u8(torch.from_numpy(src)[None], resize.table(17, 50), resize.table(23, 9))[0].numpy()
    assert np.array_equal(got, want)


@pytest.mark.parametrize("n,s", SWEEP)
def test_tap_counts_and_starts_keep_pillows_bounds(n, s):
    import math
    from vit_torch_amd import resize
    t = resize.table(n, s)
    taps = t.shape[0] - 2
    assert taps == 2 * math.ceil(2 * max(n / s, 1.0)) + 1 and taps <= resize.TAP_LIMIT
    start, count, k = t[0].long(), t[1].long(), t[2:].long()
    assert t.dtype == torch.int32 and t.shape[1] == s
    assert (start >= 0).all() and (count >= 1).all() and (count <= taps).all() and (start + count <= n).all()
    assert (start[1:] >= start[:-1]).all() and ((start + count)[1:] >= (start + count)[:-1]).all()      # monotone windows
    live = torch.arange(taps)[:, None] < count[None, :]
    assert (k[~live] == 0).all()
    assert ((k.sum(0) - (1 << 22)).abs() <= taps).all()          # weights sum to one in 22-bit fixed point, up to rounding


def test_over_long_tables_are_refused():
    from vit_torch_amd import VitmiError, resize
    resize.table(240, 32)                                        # 7.5x down: 31 taps, the longest the kernels take
    with pytest.raises(VitmiError, match="taps"):
        resize.table(241, 32)
    with pytest.raises(VitmiError):
        resize.table(0, 32)


def test_non_square_sources_are_refused():
    from vit_torch_amd import VitmiError
    from vit_torch_amd.data import DeviceAugment
    aug = DeviceAugment(224, train=True, device="cpu", resize=True)
    with pytest.raises(VitmiError, match="square"):
        aug.draw(2, 96, 80)
    with pytest.raises(VitmiError, match="square"):
        aug.prepare(96, 80)
    with pytest.raises(VitmiError, match="square"):
        aug(torch.zeros(2, 96, 80, 3, dtype=torch.uint8))


def test_draw_covers_the_resized_padded_image():
    from vit_torch_amd.data import DeviceAugment
    aug = DeviceAugment(224, train=True, device="cpu", resize=True, generator=torch.Generator("cpu").manual_seed(0))
    oy, ox, fl = aug.draw(4096, 96, 96)
    assert int(oy.min()) == 0 and int(oy.max()) == 2 * aug.pad and int(ox.max()) == 2 * aug.pad
    aug.prepare(96, 96)
    assert tuple(aug._tables[96].shape) == (7, 224)
    aug.prepare(224, 224)                                        # source already at S: nothing to build
    assert set(aug._tables) == {96}
