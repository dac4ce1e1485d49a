"""Device input pipeline with the reference's resize (utils_datasets.py:553-582 when the stored size differs from the
training size): vitmi_resize_ingest / vitmi_resize_ingest_patchify against Pillow's bicubic resize (the committed
fixture, or the int64 restatement of its passes in tests/resize_util.py) followed by the torch crop / flip / normalize
chain, bit for bit."""
import math
import os

import numpy as np
import pytest
import torch

from tests.resize_util import crop_flip_normalize, resize_u8

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resize_bicubic.npz")


def _norm(name, C):
    from vit_torch_amd.data import NORM
    return NORM[name]["mean"][:C], NORM[name]["std"][:C]


def _restated(resized_u8_nhwc, aug, oy, ox, fl):
    B = resized_u8_nhwc.shape[0]
    if oy is None:
        oy = ox = [aug.pad] * B
        fl = [0] * B
    else:
        oy, ox, fl = oy.cpu().tolist(), ox.cpu().tolist(), fl.cpu().tolist()
    return crop_flip_normalize(resized_u8_nhwc, oy, ox, fl, aug.mean.cpu(), aug.std.cpu(), aug.S, aug.pad)


@pytest.mark.parametrize("case", ["96_224_c3", "96_384_c3", "32_224_c3", "40_32_c3", "96_224_c1"])
@pytest.mark.parametrize("norm", ["stl10", "cifar10"])
@pytest.mark.parametrize("train", [True, False])
def test_transform_equals_pillow_then_crop_flip_normalize(lib, case, norm, train):
    from vit_torch_amd.data import DeviceAugment
    z = np.load(GOLDEN)
    src, resized = torch.from_numpy(z[f"src_{case}"]), torch.from_numpy(z[f"out_{case}"])
    n, S, C = src.shape[0], resized.shape[0], src.shape[2]
    B = 16
    aug = DeviceAugment(S, *_norm(norm, C), train=train, generator=torch.Generator("cpu").manual_seed(3), resize=True)
    img = src[None].expand(B, n, n, C).contiguous()
    oy, ox, fl = aug.draw(B, n, n)
    got = aug(img.cuda(), oy, ox, fl)
    if train:
        assert int(oy.max()) <= 2 * aug.pad and int(fl.sum()) not in (0, B)
    want = _restated(resized[None].expand(B, S, S, C), aug, oy, ox, fl)
    assert got.shape == (B, C, S, S)
    assert torch.equal(got.cpu(), want), (got.cpu() - want).abs().max()


@pytest.mark.parametrize("S,p,dt", [(224, 16, torch.bfloat16), (224, 8, torch.float32), (384, 16, torch.float32),
                                    (384, 8, torch.bfloat16)])
def test_patch_rows_equal_resize_ingest_then_patchify(lib, S, p, dt):
    from vit_torch_amd import ops
    from vit_torch_amd.data import DeviceAugment
    g = torch.Generator("cpu").manual_seed(11)
    B, C, cls_rows = 5, 3, 1
    img = torch.randint(0, 256, (B, 96, 96, C), generator=g, dtype=torch.uint8).cuda()
    aug = DeviceAugment(S, *_norm("stl10", C), train=True, generator=torch.Generator("cpu").manual_seed(6), resize=True)
    oy, ox, fl = aug.draw(B, 96, 96)
    x = aug(img, oy, ox, fl)
    gq = S // p
    rows_n, ld = B * (cls_rows + gq * gq), C * p * p + 8                 # 8 zero K-padding columns
    want = torch.full((rows_n, ld), float("nan"), device="cuda").to(dt)
    ops.patchify(x, want, p, cls_rows=cls_rows)
    buf = torch.full((rows_n * ld + 64,), 7.0, device="cuda").to(dt)    # a sentinel past the last row
    out = buf[:rows_n * ld].view(rows_n, ld)
    t = aug._tables[96]
    ops.resize_ingest_patchify(img, out, t, t, oy, ox, fl, aug.mean, aug.std, S, aug.pad, p, cls_rows)
    assert torch.equal(out.float().cpu(), want.float().cpu())
    assert out.view(B, cls_rows + gq * gq, ld)[:, :cls_rows].abs().max().item() == 0
    assert out[:, C * p * p:].abs().max().item() == 0
    assert (buf[rows_n * ld:].float() == 7.0).all()
    pr = aug.patch_rows(img, p, dtype=dt, off_y=oy, off_x=ox, flip=fl)
    assert torch.equal(pr.rows.float().cpu(), want[:, :C * p * p].float().cpu())


@pytest.mark.parametrize("S,train", [(224, True), (96, True), (96, False)])
def test_source_already_at_size_is_not_resized(lib, S, train):
    from vit_torch_amd.data import DeviceAugment
    g = torch.Generator("cpu").manual_seed(4)
    B = 7
    img = torch.randint(0, 256, (B, S, S, 3), generator=g, dtype=torch.uint8).cuda()
    outs, rows = [], []
    for resize in (False, True):
        aug = DeviceAugment(S, *_norm("stl10", 3), train=train, generator=torch.Generator("cpu").manual_seed(9),
                            resize=resize)
        oy, ox, fl = aug.draw(B, S, S)
        outs.append(aug(img, oy, ox, fl).cpu())
        rows.append(aug.patch_rows(img, 16, off_y=oy, off_x=ox, flip=fl).rows.float().cpu())
        assert not aug._tables
    assert torch.equal(outs[0], outs[1]) and torch.equal(rows[0], rows[1])


@pytest.mark.parametrize("S", [224, 384])
def test_full_batch(lib, S):
    """B = 256 (the training batch): sampled images against the restatement, the batch against B = 1 launches, and a
    second run bit-identical (deterministic: no atomics)."""
    from vit_torch_amd import resize
    from vit_torch_amd.data import DeviceAugment
    g = torch.Generator("cpu").manual_seed(21)
    B = 256
    img = torch.randint(0, 256, (B, 96, 96, 3), generator=g, dtype=torch.uint8)
    aug = DeviceAugment(S, *_norm("stl10", 3), train=True, generator=torch.Generator("cpu").manual_seed(22), resize=True)
    oy, ox, fl = aug.draw(B, 96, 96)
    img_d = img.cuda()
    got = aug(img_d, oy, ox, fl)
    again = aug(img_d, oy, ox, fl)
    assert torch.equal(got, again)
    idx = [0, 1, 127, 254, 255]
    t = resize.table(96, S)
    want = crop_flip_normalize(resize_u8(img[idx], t, t), oy.cpu()[idx].tolist(), ox.cpu()[idx].tolist(),
                               fl.cpu()[idx].tolist(), aug.mean.cpu(), aug.std.cpu(), S, aug.pad)
    assert torch.equal(got[idx].cpu(), want), (got[idx].cpu() - want).abs().max()
    ones = torch.cat([aug(img_d[b:b + 1], oy[b:b + 1], ox[b:b + 1], fl[b:b + 1]) for b in range(B)])
    assert torch.equal(got, ones)


def test_graph_replay_with_new_images_and_draws(lib):
    from vit_torch_amd.data import DeviceAugment
    g = torch.Generator("cpu").manual_seed(31)
    B, S = 16, 224
    aug = DeviceAugment(S, *_norm("stl10", 3), train=True, generator=torch.Generator("cpu").manual_seed(32), resize=True)
    aug.prepare(96, 96)
    img = torch.randint(0, 256, (B, 96, 96, 3), generator=g, dtype=torch.uint8).cuda()
    oy, ox, fl = aug.draw(B, 96, 96)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        aug(img, oy, ox, fl)                                             # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = aug(img, oy, ox, fl)
        rows = aug.patch_rows(img, 16, off_y=oy, off_x=ox, flip=fl)
    for _ in range(2):
        img.copy_(torch.randint(0, 256, (B, 96, 96, 3), generator=g, dtype=torch.uint8).cuda())
        for dst, src in zip((oy, ox, fl), aug.draw(B, 96, 96)):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, aug(img, oy, ox, fl))
        assert torch.equal(rows.rows, aug.patch_rows(img, 16, off_y=oy, off_x=ox, flip=fl).rows)


def test_capture_without_prepare_names_prepare(lib):
    from vit_torch_amd import VitmiError
    from vit_torch_amd.data import DeviceAugment
    aug = DeviceAugment(224, *_norm("stl10", 3), train=False, resize=True)
    img = torch.zeros(2, 96, 96, 3, dtype=torch.uint8, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(VitmiError, match="prepare"):
        with torch.cuda.graph(graph):
            aug(img)
    torch.cuda.synchronize()


def test_training_step_on_patch_rows_matches_the_image_tensor(lib):
    from vit_torch_amd import CrossEntropyLoss, VisionTransformer
    from vit_torch_amd.data import DeviceAugment
    g = torch.Generator("cpu").manual_seed(12)
    B = 4
    img = torch.randint(0, 256, (B, 96, 96, 3), generator=g, dtype=torch.uint8).cuda()
    y = torch.randint(0, 10, (B,), generator=g).cuda()
    aug = DeviceAugment(224, *_norm("stl10", 3), train=True, generator=torch.Generator("cpu").manual_seed(7), resize=True)
    oy, ox, fl = aug.draw(B, 96, 96)
    torch.manual_seed(2)
    m = VisionTransformer(img_size=224, patch_size=16, embed_dim=64, depth=2, num_heads=2, num_classes=10,
                          apply_head=True, compute_dtype="bf16", residual_dtype="auto").cuda()
    outs, grads = [], []
    for inp in (aug(img, oy, ox, fl), aug.patch_rows(img, 16, off_y=oy, off_x=ox, flip=fl)):
        m.zero_grad()
        out = m(inp)
        CrossEntropyLoss()(out, y).backward()
        outs.append(out.detach().clone())
        grads.append([p.grad.clone() for p in m.parameters() if p.grad is not None])
    assert torch.equal(outs[0], outs[1])
    assert len(grads[0]) == len(grads[1]) > 0 and all(torch.equal(a, b) for a, b in zip(*grads))


def test_linear_evaluation_epoch_on_resized_stl10_batches(lib):
    """One Network.fit epoch in linear-evaluation form (frozen backbone, trained head) on 96x96 uint8 batches resized to
    224 on the device: the loader hands over raw bytes, the device pipeline does the rest."""
    from vit_torch_amd import VisionModelZoo, VisionTransformer
    from vit_torch_amd.data import DeviceAugment
    from vit_torch_amd.network import Network
    g = torch.Generator("cpu").manual_seed(13)
    batches = [(torch.randint(0, 256, (8, 96, 96, 3), generator=g, dtype=torch.uint8),
                torch.randint(0, 10, (8,), generator=g)) for _ in range(3)]
    train_aug = DeviceAugment(224, *_norm("stl10", 3), train=True, generator=torch.Generator("cpu").manual_seed(14),
                              resize=True)
    test_aug = DeviceAugment(224, *_norm("stl10", 3), train=False, resize=True)
    bb = VisionTransformer(img_size=224, patch_size=16, embed_dim=64, depth=1, num_heads=2, apply_head=False,
                           compute_dtype="fp32")
    head = VisionModelZoo.get_classifier_head(64, [32, 10])
    net = Network(head, opt="sgd", lr=5e-2, lr_type="step", lr_step=100, frozen_model_bottom=[bb])
    before = [p.detach().clone() for p in head.parameters()]
    hist = net.fit(((train_aug(x.cuda()), y) for x, y in batches), ((test_aug(x.cuda()), y) for x, y in batches),
                   epochs=1)
    assert len(hist) == 1 and len(hist[0]["train"]["loss"]) == 3 and math.isfinite(hist[0]["train"]["loss_avg"])
    assert 0.0 <= hist[0]["val"]["acc"] <= 1.0 and hist[0]["val"]["correct"].size == 24
    assert any(not torch.equal(a, b.detach()) for a, b in zip(before, head.parameters()))
    assert set(train_aug._tables) == set(test_aug._tables) == {96}
