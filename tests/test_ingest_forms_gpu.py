"""The four uint8 ingest kernels (image_ingest_kernel, ingest_patchify_kernel, resize_ingest_kernel,
resize_ingest_patchify_kernel) against the plain-torch reference of tests/ingest_util.py, bit for bit, on every form
their entry points accept: non-square sources and distinct tables per axis, every band height of the resize kernels
(tests/test_ingest_ref_cpu.py asserts the band of each case through vitmi_resize_ingest_plan), ragged last bands, bands
wholly in the crop padding, both staging branches, C = 1..4, fill 0 / 128 / 255, mean / std given or not, the
evaluation form, every patch-row layout, and a second pass of the plain kernels' grid-stride loops.

Calls are at the ops level.  Every destination is a view into a larger buffer filled with NaN (fp32) or 1e30 (bf16): the
elements before and after it must come back untouched, the destination itself equal to the reference (so without a NaN).
Offsets are pinned to the corners of each axis (tests/ingest_util.draws)."""
import math

import pytest
import torch

from tests import ingest_util as U

pytestmark = pytest.mark.gpu

# elements on either side of a destination (16-byte alignment is kept): wider than one whole band of any case below, as
# rows (at most 28 x 36 elements) or as patch rows (at most 63 x 48), so an extra band lands in the guard and is seen
GUARD = 4096


def _guarded(shape, dtype):
    n = math.prod(shape)
    buf = torch.full((n + 2 * GUARD,), float("nan") if dtype == torch.float32 else 1e30, dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + n].view(shape)


def _assert_guards_untouched(buf):
    g = torch.cat([buf[:GUARD], buf[-GUARD:]]).cpu()
    if buf.dtype == torch.float32:
        assert bool(g.isnan().all()), "a store outside the destination"
    else:
        assert bool((g == torch.tensor(1e30, dtype=buf.dtype)).all()), "a store outside the destination"


def _assert_equal(buf, out, want):
    got = out.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype
    assert not bool(got.float().isnan().any()) and not bool((got.float() > 1e29).any())      # every element written
    assert torch.equal(got, want), f"{int((got != want).sum())} of {want.numel()} elements differ"
    _assert_guards_untouched(buf)


def _device_args(c):
    """(src, oy, ox, flip, mean, std) of a case on the device."""
    oy, ox, fl = U.draws(c)

    def dev(v, dt):
        return None if v is None else torch.as_tensor(v, dtype=dt).cuda()
    mean, std = U.norm(c)
    return (U.source(c).cuda(), dev(oy, torch.int32), dev(ox, torch.int32), dev(fl, torch.uint8), dev(mean, torch.float32),
            dev(std, torch.float32))


def _device_tables(c):
    return tuple(t.cuda() for t in U.tables(c))


def _assert_patch_rows(buf, out, x_ref, c, p, cls_rows, ld, dt):
    _assert_equal(buf, out, U.patch_rows_ref(x_ref, p, cls_rows, ld, dt))
    ntok, kp = cls_rows + (c.S // p) ** 2, c.C * p * p
    if cls_rows:
        assert out.view(-1, ntok, ld)[:, :cls_rows].float().abs().max().item() == 0
    if ld > kp:
        assert out[:, kp:].float().abs().max().item() == 0


# --------------------------------------------------------------------------- image_ingest, ingest_patchify ---
@pytest.mark.parametrize("name", [c.name for c in U.PLAIN_CASES])
def test_image_ingest_equals_the_reference(lib, name):
    from vit_torch_amd import ops
    c = U.CASES[name]
    src, oy, ox, fl, mean, std = _device_args(c)
    buf, dst = _guarded((src.shape[0], c.C, c.S, c.S), torch.float32)
    ops.image_ingest(src, dst, oy, ox, fl, mean, std, c.pad, fill=c.fill)
    _assert_equal(buf, dst, U.reference(c))


@pytest.mark.parametrize("name", [c.name for c in U.PLAIN_CASES])
def test_ingest_patchify_equals_the_reference_in_every_row_layout(lib, name):
    from vit_torch_amd import ops
    c = U.CASES[name]
    src, oy, ox, fl, mean, std = _device_args(c)
    assert c.patch
    for p, cls_rows, extra, dt in c.patch:
        ld = c.C * p * p + extra
        buf, out = _guarded((src.shape[0] * (cls_rows + (c.S // p) ** 2), ld), dt)
        ops.ingest_patchify(src, out, oy, ox, fl, mean, std, c.S, c.pad, p, cls_rows, fill=c.fill)
        _assert_patch_rows(buf, out, U.reference(c), c, p, cls_rows, ld, dt)


_CAP = {}


def _grid_cap_case():
    """B=64, C=3, 224x224, pad 18: 2.41 M threads in either plain kernel against the 8192 x 256 = 2.10 M in flight."""
    if not _CAP:
        B, S, pad = 64, 224, 18
        g = torch.Generator("cpu").manual_seed(64)
        src = torch.randint(0, 256, (B, S, S, 3), generator=g, dtype=torch.uint8)
        oy = [0, 0, 2 * pad, 2 * pad] + [(7 * b) % (2 * pad + 1) for b in range(4, B)]
        ox = [0, 2 * pad, 0, 2 * pad] + [(11 * b) % (2 * pad + 1) for b in range(4, B)]
        fl = [b % 2 for b in range(B)]
        mean, std = torch.tensor(U.MEAN[:3]), torch.tensor(U.STD[:3])
        _CAP.update(src=src, oy=oy, ox=ox, fl=fl, mean=mean, std=std, S=S, pad=pad,
                    ref=U.ingest_ref(src, oy, ox, fl, mean, std, S, pad, 128))
    return _CAP


def _cap_device(k):
    return (k["src"].cuda(), torch.tensor(k["oy"], dtype=torch.int32).cuda(), torch.tensor(k["ox"], dtype=torch.int32).cuda(),
            torch.tensor(k["fl"], dtype=torch.uint8).cuda(), k["mean"].cuda(), k["std"].cuda())


def test_image_ingest_past_the_grid_cap(lib):
    from vit_torch_amd import ops
    k = _grid_cap_case()
    B, S = k["src"].shape[0], k["S"]
    assert B * 3 * S * (S // 4) > 8192 * 256                          # the loop takes a second pass
    src, oy, ox, fl, mean, std = _cap_device(k)
    buf, dst = _guarded((B, 3, S, S), torch.float32)
    ops.image_ingest(src, dst, oy, ox, fl, mean, std, k["pad"])
    _assert_equal(buf, dst, k["ref"])


def test_ingest_patchify_past_the_grid_cap(lib):
    from vit_torch_amd import ops
    k = _grid_cap_case()
    B, S, p, cls_rows, ld = k["src"].shape[0], k["S"], 16, 1, 768
    rows = B * (cls_rows + (S // p) ** 2)
    assert rows * (ld // 4) > 8192 * 256
    src, oy, ox, fl, mean, std = _cap_device(k)
    buf, out = _guarded((rows, ld), torch.bfloat16)
    ops.ingest_patchify(src, out, oy, ox, fl, mean, std, S, k["pad"], p, cls_rows)
    _assert_equal(buf, out, U.patch_rows_ref(k["ref"], p, cls_rows, ld, torch.bfloat16))


# ------------------------------------------------------------------- resize_ingest, resize_ingest_patchify ---
@pytest.mark.parametrize("name", [c.name for c in U.RESIZE_CASES])
def test_resize_ingest_equals_the_reference(lib, name):
    from vit_torch_amd import ops
    c = U.CASES[name]
    src, oy, ox, fl, mean, std = _device_args(c)
    ytab, xtab = _device_tables(c)
    buf, dst = _guarded((src.shape[0], c.C, c.S, c.S), torch.float32)
    ops.resize_ingest(src, dst, ytab, xtab, oy, ox, fl, mean, std, c.pad, fill=c.fill)
    _assert_equal(buf, dst, U.reference(c))


@pytest.mark.parametrize("name", [c.name for c in U.RESIZE_CASES if c.patch])
def test_resize_ingest_patchify_equals_the_reference(lib, name):
    from vit_torch_amd import ops
    c = U.CASES[name]
    src, oy, ox, fl, mean, std = _device_args(c)
    ytab, xtab = _device_tables(c)
    for p, cls_rows, extra, dt in c.patch:
        ld = c.C * p * p + extra
        buf, out = _guarded((src.shape[0] * (cls_rows + (c.S // p) ** 2), ld), dt)
        ops.resize_ingest_patchify(src, out, ytab, xtab, oy, ox, fl, mean, std, c.S, c.pad, p, cls_rows, fill=c.fill)
        _assert_patch_rows(buf, out, U.reference(c), c, p, cls_rows, ld, dt)


def test_same_size_tables_equal_the_plain_kernels(lib):
    """resize.table(n, n) is the identity: the resize kernels on it equal image_ingest / ingest_patchify on the same draws."""
    from vit_torch_amd import ops, resize
    c = U.IDENTITY_CASE
    src, oy, ox, fl, mean, std = _device_args(c)
    t = resize.table(40, 40).cuda()
    B = src.shape[0]
    ref = U.reference(c)
    outs = []
    for call in (lambda d: ops.image_ingest(src, d, oy, ox, fl, mean, std, c.pad),
                 lambda d: ops.resize_ingest(src, d, t, t, oy, ox, fl, mean, std, c.pad)):
        buf, dst = _guarded((B, 3, 32, 32), torch.float32)
        call(dst)
        _assert_equal(buf, dst, ref)
        outs.append(dst)
    assert torch.equal(outs[0], outs[1])
    p, cls_rows, ld = 8, 1, 3 * 64 + 8
    rows = []
    for call in (lambda o: ops.ingest_patchify(src, o, oy, ox, fl, mean, std, 32, c.pad, p, cls_rows),
                 lambda o: ops.resize_ingest_patchify(src, o, t, t, oy, ox, fl, mean, std, 32, c.pad, p, cls_rows)):
        buf, out = _guarded((B * (cls_rows + 16), ld), torch.bfloat16)
        call(out)
        _assert_patch_rows(buf, out, ref, c, p, cls_rows, ld, torch.bfloat16)
        rows.append(out)
    assert torch.equal(rows[0], rows[1])


def test_a_halved_band_is_repeatable_and_batch_invariant(lib):
    """240x240x3 -> 32x32 (bands of 4 rows): two runs and one launch per image give the same bits."""
    from vit_torch_amd import ops
    c = U.CASES["240x240_c3_to_32x32"]
    src, oy, ox, fl, mean, std = _device_args(c)
    ytab, xtab = _device_tables(c)
    B = src.shape[0]

    def run(sl):
        dst = torch.full((sl.stop - sl.start, c.C, c.S, c.S), float("nan"), device="cuda")
        ops.resize_ingest(src[sl].contiguous(), dst, ytab, xtab, oy[sl], ox[sl], fl[sl], mean, std, c.pad, fill=c.fill)
        p, cls_rows, extra, dt = c.patch[0]
        rows = torch.full((dst.shape[0] * (cls_rows + (c.S // p) ** 2), c.C * p * p + extra), float("nan"), device="cuda").to(dt)
        ops.resize_ingest_patchify(src[sl].contiguous(), rows, ytab, xtab, oy[sl], ox[sl], fl[sl], mean, std, c.S, c.pad, p,
                                   cls_rows, fill=c.fill)
        return dst, rows
    first, again = run(slice(0, B)), run(slice(0, B))
    ones = [run(slice(b, b + 1)) for b in range(B)]
    for i in range(2):
        assert torch.equal(first[i], again[i])
        assert torch.equal(first[i], torch.cat([o[i] for o in ones]))
    assert torch.equal(first[0].cpu(), U.reference(c))


# ----------------------------------------------------------------------------------------------- DeviceAugment ---
def test_device_augment_on_a_non_square_batch(lib):
    from vit_torch_amd.data import NORM, DeviceAugment
    H, W, S, B = 40, 56, 32, 8
    aug = DeviceAugment(S, **NORM["stl10"], train=True, generator=torch.Generator("cpu").manual_seed(5))
    my, mx = H + 2 * aug.pad - S, W + 2 * aug.pad - S
    assert (aug.pad, my, mx) == (2, 12, 28)
    draw = DeviceAugment(S, train=True, device="cpu", generator=torch.Generator("cpu").manual_seed(0)).draw(4096, H, W)
    assert (int(draw[0].min()), int(draw[0].max()), int(draw[1].min()), int(draw[1].max())) == (0, my, 0, mx)
    src = torch.randint(0, 256, (B, H, W, 3), generator=torch.Generator("cpu").manual_seed(40), dtype=torch.uint8)
    oy, ox, fl = [0, 0, my, my, 5, 5, 0, my], [0, mx, 0, mx, 17, 17, mx, 0], [0, 1, 0, 1, 0, 1, 0, 1]
    dev = [torch.tensor(v, dtype=dt).cuda() for v, dt in ((oy, torch.int32), (ox, torch.int32), (fl, torch.uint8))]
    ref = U.ingest_ref(src, oy, ox, fl, NORM["stl10"]["mean"], NORM["stl10"]["std"], S, aug.pad, 128)
    got = aug(src.cuda(), *dev)
    assert got.shape == (B, 3, S, S) and torch.equal(got.cpu(), ref)
    for cls_rows in (0, 2):
        pr = aug.patch_rows(src.cuda(), 8, dtype=torch.bfloat16, cls_rows=cls_rows, off_y=dev[0], off_x=dev[1], flip=dev[2])
        assert (pr.B, pr.C, pr.H, pr.W, pr.p, pr.cls_rows) == (B, 3, S, S, 8, cls_rows)
        assert torch.equal(pr.rows.cpu(), U.patch_rows_ref(ref, 8, cls_rows, 3 * 64, torch.bfloat16))
