"""The CPU side of the ingest sweep (no GPU): the reference of tests/ingest_util.py held to account against the committed
Pillow fixture, live Pillow and an index-by-index restatement; the band each resize case runs with, as a fact, through
the host-only vitmi_resize_ingest_plan; and every host-side refusal of the four entry points, which return before any
launch (dummy aligned pointers, as test_abi_cpu.py::test_bad_arguments_are_rejected_without_a_gpu)."""
import os

import numpy as np
import pytest
import torch

from tests import ingest_util as U
from tests.resize_util import resize_u8

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resize_bicubic.npz")
E_BADARG, E_ALIGN, E_DTYPE, E_SHAPE = -1, -2, -3, -4         # include/vitmi.h


# ------------------------------------------------------------------------------------------------ the reference ---
@pytest.mark.parametrize("name", ["96_224_c3", "32_224_c3", "96_384_c3", "40_32_c3", "96_224_c1"])
def test_ingest_ref_equals_the_pillow_fixture(name):
    """Evaluation form (no pad, no offsets, no mean / std) of the fixture's source: the fixture's resized bytes / 255."""
    from vit_torch_amd import resize
    z = np.load(GOLDEN)
    src, out = torch.from_numpy(z[f"src_{name}"]), torch.from_numpy(z[f"out_{name}"])
    n, s = src.shape[0], out.shape[0]
    t = resize.table(n, s)
    got = U.ingest_ref(src[None], None, None, None, None, None, s, 0, 128, t, t)
    want = out.reshape(s, s, -1).permute(2, 0, 1)[None].float() / 255
    assert got.dtype == torch.float32 and torch.equal(got, want)


def _pillow(img_hwc, Hr, Wr):
    """Pillow's bicubic resize of one uint8 HWC image.  RGB as one image; any other channel count channel by channel as
    'L' images (Pillow premultiplies alpha in LA / RGBA, the kernels treat every channel alike)."""
    from PIL import Image
    a = img_hwc.numpy()
    if a.shape[2] == 3:
        return torch.from_numpy(np.asarray(Image.fromarray(a).resize((Wr, Hr), Image.BICUBIC)).copy())
    chans = [np.asarray(Image.fromarray(np.ascontiguousarray(a[..., c])).resize((Wr, Hr), Image.BICUBIC))
             for c in range(a.shape[2])]
    return torch.from_numpy(np.stack(chans, -1).copy())


@pytest.mark.parametrize("name", [c.name for c in U.RESIZE_CASES])
def test_ingest_ref_equals_live_pillow_then_crop_flip_normalize(name):
    pytest.importorskip("PIL.Image")
    c = U.CASES[name]
    src = U.source(c)
    resized = torch.stack([_pillow(src[b], c.Hr, c.Wr) for b in range(src.shape[0])])
    assert tuple(resized.shape) == (src.shape[0], c.Hr, c.Wr, c.C)
    assert torch.equal(resize_u8(src, *U.tables(c)), resized)
    oy, ox, fl = U.draws(c)
    want = U.ingest_ref(resized, oy, ox, fl, *U.norm(c), c.S, c.pad, c.fill)            # no tables: Pillow resized it
    assert torch.equal(U.reference(c), want)


@pytest.mark.parametrize("H,W,C,Hr,Wr", [(256, 256, 3, 224, 224), (240, 472, 4, 32, 64), (17, 23, 2, 50, 9)])
def test_restated_resize_equals_live_pillow_off_the_table(H, W, C, Hr, Wr):
    pytest.importorskip("PIL.Image")
    from vit_torch_amd import resize
    src = torch.from_numpy(np.random.default_rng(H * 7 + W).integers(0, 256, (1, H, W, C), dtype=np.uint8))
    assert torch.equal(resize_u8(src, resize.table(H, Hr), resize.table(W, Wr))[0], _pillow(src[0], Hr, Wr))


def _gather_ref(src, oy, ox, fl, mean, std, S, pad, fill):
    """The transform as the kernels' comment states it, index by index in numpy fp32 (no pad / slice / flip calls):
    dst[b,c,y,x] = (v/255 - mean[c]) / std[c], v = src[b, y + oy - pad, xs + ox - pad, c] or fill outside the image,
    xs = flip ? S-1-x : x."""
    a = src.numpy()
    B, H, W, C = a.shape
    out = np.empty((B, C, S, S), np.float32)
    y, x = np.arange(S)[:, None], np.arange(S)[None, :]
    for b in range(B):
        sy = y + oy[b] - pad + 0 * x
        sx = (S - 1 - x if fl[b] else x) + ox[b] - pad + 0 * y
        inside = (sy >= 0) & (sy < H) & (sx >= 0) & (sx < W)
        for ch in range(C):
            v = np.where(inside, a[b, np.clip(sy, 0, H - 1), np.clip(sx, 0, W - 1), ch], fill).astype(np.float32)
            out[b, ch] = (v / np.float32(255) - np.float32(mean[ch])) / np.float32(std[ch])
    return torch.from_numpy(out)


@pytest.mark.parametrize("name", [c.name for c in U.PLAIN_CASES])
def test_ingest_ref_equals_the_index_by_index_restatement(name):
    c = U.CASES[name]
    B = U.batch_size(c)
    oy, ox, fl = U.draws(c)
    if oy is None:
        oy, ox, fl = [c.pad] * B, [c.pad] * B, [0] * B
    mean, std = U.norm(c)
    mean = [0.0] * c.C if mean is None else mean.tolist()
    std = [1.0] * c.C if std is None else std.tolist()
    ref = U.reference(c)
    assert tuple(ref.shape) == (B, c.C, c.S, c.S) and ref.dtype == torch.float32
    assert torch.equal(ref, _gather_ref(U.source(c), oy, ox, fl, mean, std, c.S, c.pad, c.fill))


def test_the_all_padding_case_is_all_fill_at_its_corners():
    c = U.CASES["all_padding_8_c3_fill255"]
    ref, (mean, std) = U.reference(c), U.norm(c)
    fillv = (torch.tensor(float(c.fill)) / 255 - mean) / std
    assert torch.equal(ref[:4], fillv[None, :, None, None].expand(4, c.C, c.S, c.S))
    assert not torch.equal(ref[4], ref[0])


@pytest.mark.parametrize("p,cls_rows,extra,dt", [(4, 0, 0, torch.float32), (8, 1, 8, torch.bfloat16),
                                                 (16, 2, 8, torch.float32)])
def test_patch_rows_ref_places_every_element(p, cls_rows, extra, dt):
    B, C, S = 3, 2, 32
    x = torch.randn(B, C, S, S, generator=torch.Generator("cpu").manual_seed(p))
    g, ld = S // p, C * p * p + extra
    rows = U.patch_rows_ref(x, p, cls_rows, ld, dt)
    ntok = cls_rows + g * g
    assert tuple(rows.shape) == (B * ntok, ld) and rows.dtype == dt
    want = torch.zeros(B * ntok, ld)
    for b in range(B):
        for py in range(g):
            for px in range(g):
                for ch in range(C):
                    blk = x[b, ch, py * p:(py + 1) * p, px * p:(px + 1) * p]
                    want[b * ntok + cls_rows + py * g + px, ch * p * p:(ch + 1) * p * p] = blk.reshape(-1)   # k = c p^2 + i p + j
    assert torch.equal(rows, want.to(dt))


@pytest.mark.parametrize("n", [1, 8, 37, 40, 224])
def test_a_same_size_table_is_the_identity(n):
    from vit_torch_amd import resize
    t = resize.table(n, n)
    src = torch.randint(0, 256, (2, n, n, 3), generator=torch.Generator("cpu").manual_seed(n), dtype=torch.uint8)
    assert torch.equal(resize_u8(src, t, t), src)
    if n >= 3:
        assert t.shape[0] == 7 and (t[2:].sum(0) == 1 << 22).all() and (t[2:].max(0).values == 1 << 22).all()


def test_draws_are_pinned_to_the_corners_of_each_axis():
    for c in U.CASES.values():
        oy, ox, fl = U.draws(c)
        if oy is None:
            continue
        eh, ew = U.extent(c)
        assert min(oy) == 0 and max(oy) == eh + 2 * c.pad - c.S and min(ox) == 0 and max(ox) == ew + 2 * c.pad - c.S
        assert {0, 1} == set(fl) and len(oy) == len(ox) == len(fl) == U.batch_size(c)
        if eh != ew:
            assert max(oy) != max(ox)


def test_every_argument_value_is_in_the_table():
    forms = [f for c in U.PLAIN_CASES for f in c.patch]
    for i, values in enumerate([(4, 8, 16), (0, 1, 2), (0, 8), (torch.bfloat16, torch.float32)]):
        assert {f[i] for f in forms} == set(values)
    assert {c.C for c in U.PLAIN_CASES} == {1, 2, 3, 4} == {c.C for c in U.RESIZE_CASES}
    assert {c.fill for c in U.PLAIN_CASES} == {0, 128, 255} == {c.fill for c in U.RESIZE_CASES}
    for cases in (U.PLAIN_CASES, U.RESIZE_CASES):
        assert {c.norm for c in cases} == {True, False}
        assert all(c.S % p == 0 for c in cases for p, *_ in c.patch)
    assert {(c.H, c.W) for c in U.PLAIN_CASES} >= {(40, 56), (56, 40)}
    assert any(c.offsets is None and c.pad == 0 for c in U.PLAIN_CASES) and any(c.offsets is None and c.pad for c in U.PLAIN_CASES)
    assert any(c.W * c.C % 2 for c in U.RESIZE_CASES) and any(c.W * c.C % 16 == 0 for c in U.RESIZE_CASES)   # both staging loops
    assert any(c.S % c.band for c in U.RESIZE_CASES)                                                         # a ragged last band


def test_crops_wholly_in_the_padding_are_all_fill_in_the_reference():
    """40x40 -> 32x32 under pad = 32: the crops at oy = 0 and oy = 64 never touch the image (on the device: one band of 32
    rows with no source row to stage), the one at oy = 32 does."""
    c = U.CASES["40x40_c3_to_32x32_pad32"]
    oy, _, _ = U.draws(c)
    ref, (mean, std) = U.reference(c), U.norm(c)
    fillv = ((torch.tensor(float(c.fill)) / 255 - mean) / std)[:, None, None].expand(c.C, c.S, c.S)
    assert sorted(set(oy)) == [0, 32, 64]
    for b, y in enumerate(oy):
        assert torch.equal(ref[b], fillv) == (y != 32)


def test_device_augment_draws_cover_each_axis_of_a_non_square_source():
    from vit_torch_amd.data import DeviceAugment
    aug = DeviceAugment(32, train=True, device="cpu", generator=torch.Generator("cpu").manual_seed(0))
    oy, ox, fl = aug.draw(4096, 40, 56)
    assert aug.pad == 2
    assert int(oy.min()) == 0 and int(oy.max()) == 40 + 2 * aug.pad - 32
    assert int(ox.min()) == 0 and int(ox.max()) == 56 + 2 * aug.pad - 32
    assert 0 < int(fl.sum()) < 4096


# ------------------------------------------------------------------------------------------------- the band plan ---
def _a16(n):
    return (n + 15) & ~15


def _lds(H, W, C, Hr, Wr, ytaps, xtaps, BR):
    """The workgroup's LDS at a band of BR rows: csrc/resize.hip's lds_layout / rows_cap, restated."""
    rows_cap = min(H, ((BR - 1) * H + Hr - 1) // Hr + ytaps + 1)
    return (_a16(C * 256 * 4) + _a16((2 + xtaps) * Wr * 4) + _a16((2 + ytaps) * BR * 4) + _a16(rows_cap * W * C)
            + _a16(C * rows_cap * Wr))


def _taps(n, s):
    from vit_torch_amd import resize
    return resize.coeffs(n, s)[3]


# (H, W, C, Hr, Wr) -> {band_unit: band rows, or None where the launch refuses}
LADDER = [
    ((48, 64, 3, 72, 40), {1: 32, 8: 32}),
    ((160, 160, 3, 32, 32), {1: 16, 16: 16}),
    ((176, 176, 3, 32, 32), {1: 8, 8: 8, 16: None}),
    ((240, 240, 3, 32, 32), {1: 4, 4: 4, 8: None}),
    ((240, 240, 4, 32, 32), {1: 2, 4: None}),
    ((240, 320, 4, 32, 43), {1: 1}),
    ((240, 472, 4, 32, 64), {1: None}),
]


@pytest.mark.parametrize("geom,bands", LADDER, ids=[f"{g[0]}x{g[1]}x{g[2]}_to_{g[3]}x{g[4]}" for g, _ in LADDER])
def test_band_ladder_through_the_plan_query(lib, geom, bands):
    from vit_torch_amd import VitmiError, ops
    H, W, C, Hr, Wr = geom
    yt, xt = _taps(H, Hr), _taps(W, Wr)
    for unit, want in bands.items():
        first = unit if unit >= 32 else 32 // unit * unit
        if want is None:
            with pytest.raises(VitmiError, match=rf"rc={E_SHAPE}\).*needs {_lds(H, W, C, Hr, Wr, yt, xt, unit)} B of LDS"):
                ops.resize_ingest_plan(H, W, C, Hr, Wr, yt, xt, 32, 4, 128, unit)
            continue
        br, lds = ops.resize_ingest_plan(H, W, C, Hr, Wr, yt, xt, 32, 4, 128, unit)
        assert (br, lds) == (want, _lds(H, W, C, Hr, Wr, yt, xt, want)) and lds <= 64 * 1024
        assert want == first or _lds(H, W, C, Hr, Wr, yt, xt, 2 * want) > 64 * 1024      # halved because it had to be
    if geom == (240, 472, 4, 32, 64):
        assert _lds(H, W, C, Hr, Wr, yt, xt, 1) == 81296


def test_every_resize_case_runs_at_the_band_the_table_names(lib):
    from vit_torch_amd import ops
    seen = set()
    for c in U.RESIZE_CASES:
        yt, xt = _taps(c.H, c.Hr), _taps(c.W, c.Wr)
        br, _ = ops.resize_ingest_plan(c.H, c.W, c.C, c.Hr, c.Wr, yt, xt, c.S, c.pad, c.fill, 1)
        assert br == c.band, (c.name, br)
        seen.add(br)
        for p, *_ in c.patch:
            assert ops.resize_ingest_plan(c.H, c.W, c.C, c.Hr, c.Wr, yt, xt, c.S, c.pad, c.fill, p)[0] == max(c.band, p), c.name
    assert seen == {32, 16, 8, 4, 2, 1}
    assert ops.resize_ingest_plan(256, 256, 3, 224, 224, 7, 7, 224, 18)[0] < 32            # the 256 -> 224 path halves too
    pads = {c.name: (c.pad, c.band) for c in U.RESIZE_CASES if c.pad >= c.band}             # whole bands in the padding
    assert {"240x240_c3_to_32x32_pad8", "40x40_c3_to_32x32_pad32"} <= set(pads)


# ---------------------------------------------------------------------------------------------- host-side refusals ---
P = 0x10000          # a dummy 16-byte aligned pointer: every call below returns before it could be read


def _image_ingest(lib, dst=P, B=4, H=32, W=32, C=3, S=32, pad=4, fill=128):
    return lib.vitmi_image_ingest(P, dst, None, None, None, None, None, B, H, W, C, S, pad, fill, None)


def _ingest_patchify(lib, out=P, dtype=1, out_ld=0, B=4, H=32, W=32, C=3, S=32, pad=4, fill=128, p=8, cls_rows=1):
    return lib.vitmi_ingest_patchify(P, out, dtype, out_ld, None, None, None, None, None, B, H, W, C, S, pad, fill, p,
                                     cls_rows, None)


def _resize_ingest(lib, dst=P, ytaps=7, Hr=224, xtaps=7, Wr=224, B=4, H=96, W=96, C=3, S=224, pad=18, fill=128):
    return lib.vitmi_resize_ingest(P, dst, P, ytaps, Hr, P, xtaps, Wr, None, None, None, None, None, B, H, W, C, S, pad,
                                   fill, None)


def _resize_ingest_patchify(lib, out=P, dtype=1, out_ld=0, ytaps=7, Hr=224, xtaps=7, Wr=224, B=4, H=96, W=96, C=3, S=224,
                            pad=18, fill=128, p=16, cls_rows=1):
    return lib.vitmi_resize_ingest_patchify(P, out, dtype, out_ld, P, ytaps, Hr, P, xtaps, Wr, None, None, None, None,
                                            None, B, H, W, C, S, pad, fill, p, cls_rows, None)


def _plan(lib, ytaps=7, Hr=224, xtaps=7, Wr=224, H=96, W=96, C=3, S=224, pad=18, fill=128, band_unit=1):
    import ctypes
    br, lds = ctypes.c_int(-7), ctypes.c_int64(-7)
    rc = lib.vitmi_resize_ingest_plan(H, W, C, Hr, Wr, ytaps, xtaps, S, pad, fill, band_unit, ctypes.byref(br),
                                      ctypes.byref(lds))
    assert rc == 0 or (br.value, lds.value) == (-7, -7)          # a refusal writes nothing
    return rc


_BIG = dict(H=240, W=240, Hr=32, Wr=32, ytaps=31, xtaps=31, S=32, pad=4)       # 7.5x down: the LDS-bound geometry
_PLAIN = [_image_ingest, _ingest_patchify]
_RESIZE = [_resize_ingest, _resize_ingest_patchify]
_PATCH = [_ingest_patchify, _resize_ingest_patchify]
_ALL = _PLAIN + _RESIZE

# (what, entry points, the one argument that is wrong, code, fragment of the message)
REFUSALS = [
    ("lds_plain", [_resize_ingest, _plan], dict(H=240, W=472, C=4, Hr=32, Wr=64, ytaps=31, xtaps=31, S=32, pad=4),
     E_SHAPE, b"needs 81296 B of LDS per workgroup (limit 65536)"),
    ("lds_176_p16", [_resize_ingest_patchify], dict(H=176, W=176, Hr=32, Wr=32, ytaps=23, xtaps=23, S=32, pad=4, p=16),
     E_SHAPE, b"B of LDS per workgroup"),
    ("lds_240_p8", [_resize_ingest_patchify], dict(_BIG, p=8), E_SHAPE, b"B of LDS per workgroup"),
    ("lds_240_c4_p4", [_resize_ingest_patchify], dict(_BIG, C=4, p=4), E_SHAPE, b"B of LDS per workgroup"),
    ("c5", _RESIZE + [_plan], dict(C=5), E_SHAPE, b"C <= 4"),
    ("b65536", _RESIZE, dict(B=65536), E_SHAPE, b"B <= 65535"),
    ("ytaps33", _RESIZE + [_plan], dict(ytaps=33), E_SHAPE, b"tables need 1..32 taps (got 33, 7)"),
    ("xtaps33", _RESIZE + [_plan], dict(xtaps=33), E_SHAPE, b"tables need 1..32 taps (got 7, 33)"),
    ("s_mod_4_plain", [_image_ingest], dict(S=30), E_ALIGN, b"multiple of 4"),
    ("s_mod_4_resize", [_resize_ingest], dict(S=222), E_ALIGN, b"multiple of 4"),
    ("s_mod_p_plain", [_ingest_patchify], dict(S=32, p=12), E_SHAPE, b"S % p and p % 4 must be 0"),
    ("s_mod_p_resize", [_resize_ingest_patchify], dict(S=224, p=12), E_SHAPE, b"S % p and p % 4 must be 0"),
    ("p_mod_4_plain", [_ingest_patchify], dict(S=30, p=6), E_SHAPE, b"S % p and p % 4 must be 0"),
    ("p_mod_4_resize", [_resize_ingest_patchify], dict(S=222, p=6), E_SHAPE, b"S % p and p % 4 must be 0"),
    ("p68", [_resize_ingest_patchify], dict(S=204, p=68), E_SHAPE, b"p <= 64 (S=204 p=68)"),
    ("ld_short_plain", [_ingest_patchify], dict(out_ld=3 * 64 - 4), E_ALIGN, b"out_ld / alignment"),
    ("ld_short_resize", [_resize_ingest_patchify], dict(out_ld=3 * 256 - 4), E_ALIGN, b"out_ld / alignment"),
    ("ld_mod_4_plain", [_ingest_patchify], dict(out_ld=3 * 64 + 2), E_ALIGN, b"out_ld / alignment"),
    ("ld_mod_4_resize", [_resize_ingest_patchify], dict(out_ld=3 * 256 + 2), E_ALIGN, b"out_ld / alignment"),
    ("fill256", _ALL + [_plan], dict(fill=256), E_SHAPE, b"crop"),
    ("fill_negative", _ALL + [_plan], dict(fill=-1), E_SHAPE, b"crop"),
    ("rows_do_not_fit_plain", _PLAIN, dict(H=23, W=32), E_SHAPE, b"does not fit the padded image"),
    ("cols_do_not_fit_plain", _PLAIN, dict(H=32, W=23), E_SHAPE, b"does not fit the padded image"),
    ("rows_do_not_fit_resize", _RESIZE + [_plan], dict(Hr=187, Wr=224), E_SHAPE,
     b"crop 224 does not fit the padded resized image (187x224+2*18)"),
    ("cols_do_not_fit_resize", _RESIZE + [_plan], dict(Hr=224, Wr=187), E_SHAPE,
     b"crop 224 does not fit the padded resized image (224x187+2*18)"),
    ("dst_4_bytes_off", [_image_ingest, _resize_ingest], dict(dst=P + 4), E_ALIGN, b"dst 16-B aligned"),
    ("out_4_bytes_off", _PATCH, dict(out=P + 4), E_ALIGN, b"out_ld / alignment"),
    ("bad_out_dtype", _PATCH, dict(dtype=7), E_DTYPE, b"bad out dtype"),
    ("b0", _ALL, dict(B=0), E_BADARG, b"bad argument"),
    ("plan_unit_0", [_plan], dict(band_unit=0), E_BADARG, b"resize_ingest_plan: bad argument"),
]


@pytest.mark.parametrize("what,entries,wrong,code,fragment", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_bad_geometry_is_refused_on_the_host_before_any_launch(lib, what, entries, wrong, code, fragment):
    for fn in entries:
        rc = fn(lib, **wrong)
        msg = lib.vitmi_last_error_string()
        assert rc == code, (fn.__name__, rc, msg)
        assert fragment in msg, (fn.__name__, msg)
        # the text names the entry point; the geometry checks the three resize entries share say "resize_ingest:"
        own = b"resize_ingest" if fn in _RESIZE + [_plan] else fn.__name__.lstrip("_").encode()
        assert msg.startswith(own), (fn.__name__, msg)


def test_the_plan_accepts_what_the_launches_accept(lib):
    assert _plan(lib) == 0 and _plan(lib, band_unit=16) == 0 and _plan(lib, **_BIG) == 0 and _plan(lib, **_BIG, band_unit=4) == 0
