"""The reference's Swin arch names (models/vision_all.py:50-69, models/swin.py:768-820) resolve through
VisionModelZoo, and window-12 models carry the reference's parameter and buffer layout."""
import pytest
import torch

# (img_size, embed_dim, depths, num_heads, window_size), written out from models/swin.py:768-820
EXPECTED = {
    "swin_tiny_patch4_window7_224": (224, 96, [2, 2, 6, 2], [3, 6, 12, 24], 7),
    "swin_small_patch4_window7_224": (224, 96, [2, 2, 18, 2], [3, 6, 12, 24], 7),
    "swin_base_patch4_window7_224": (224, 128, [2, 2, 18, 2], [4, 8, 16, 32], 7),
    "swin_base_patch4_window12_384": (384, 128, [2, 2, 18, 2], [4, 8, 16, 32], 12),
    "swin_base_patch4_window7_224_22k": (224, 128, [2, 2, 18, 2], [4, 8, 16, 32], 7),
    "swin_base_patch4_window7_224_22kto1k": (224, 128, [2, 2, 18, 2], [4, 8, 16, 32], 7),
    "swin_base_patch4_window12_384_22k": (384, 128, [2, 2, 18, 2], [4, 8, 16, 32], 12),
    "swin_base_patch4_window12_384_22kto1k": (384, 128, [2, 2, 18, 2], [4, 8, 16, 32], 12),
    "swin_large_patch4_window7_224_22k": (224, 192, [2, 2, 18, 2], [6, 12, 24, 48], 7),
    "swin_large_patch4_window7_224_22kto1k": (224, 192, [2, 2, 18, 2], [6, 12, 24, 48], 7),
    "swin_large_patch4_window12_384_22k": (384, 192, [2, 2, 18, 2], [6, 12, 24, 48], 12),
    "swin_large_patch4_window12_384_22kto1k": (384, 192, [2, 2, 18, 2], [6, 12, 24, 48], 12),
}


def _shape(m):
    stages = m.layers
    return (m.patch_embed.img_size[0] if isinstance(m.patch_embed.img_size, (tuple, list)) else m.patch_embed.img_size,
            m.embed_dim, [len(s.blocks) for s in stages], [s.blocks[0].attn.num_heads for s in stages],
            stages[0].blocks[0].window_size)


@pytest.mark.parametrize("arch", sorted(EXPECTED))
def test_every_reference_swin_name_builds(arch):
    from vit_torch_amd import VisionModelZoo
    m = VisionModelZoo.get_model(arch, pretrained=False)
    assert _shape(m) == EXPECTED[arch]


def test_unknown_swin_name_still_raises():
    from vit_torch_amd import VisionModelZoo
    with pytest.raises(ValueError, match=r"arch \[swin_huge_patch4_window12_384\] not found!"):
        VisionModelZoo.get_model("swin_huge_patch4_window12_384", pretrained=False)


def test_window12_configs_inherit_the_default_drop_path_rate():
    from vit_torch_amd.swin import configs
    assert "drop_path_rate" not in configs["swin_base_patch4_window12_384"]
    assert "drop_path_rate" not in configs["swin_large_patch4_window12_384"]
    assert "crop" not in configs["swin_base_patch4_window12_384"]


def test_tiny_c24_window8_resolves():
    from vit_torch_amd.swin import get_swin_model
    m = get_swin_model("swin_tiny_c24_patch4_window8_256")
    assert _shape(m) == (256, 96, [2, 2, 6, 2], [4, 8, 16, 32], 8)
    assert m.embed_dim // m.layers[0].blocks[0].attn.num_heads == 24


def test_window12_state_dict_matches_the_oracle_layout():
    from oracle.swin_ref import SwinTransformer as Ref
    from vit_torch_amd import load_reference_checkpoint
    from vit_torch_amd.swin import get_swin_model
    m = get_swin_model("swin_base_patch4_window12_384", num_classes=10)
    ref = Ref(img_size=384, patch_size=4, embed_dim=128, depths=[2, 2, 18, 2], num_heads=[4, 8, 16, 32],
              window_size=12, num_classes=10)
    ours, theirs = m.state_dict(), ref.state_dict()
    assert sorted(ours) == sorted(theirs)
    for k, v in theirs.items():
        assert tuple(ours[k].shape) == tuple(v.shape), k
    assert tuple(ours["layers.0.blocks.0.attn.relative_position_bias_table"].shape) == (529, 4)
    assert tuple(ours["layers.0.blocks.0.attn.relative_position_index"].shape) == (144, 144)
    assert torch.equal(ours["layers.0.blocks.0.attn.relative_position_index"],
                       theirs["layers.0.blocks.0.attn.relative_position_index"])
    assert tuple(ours["layers.0.blocks.1.attn_mask"].shape) == (64, 144, 144)
    assert torch.equal(ours["layers.0.blocks.1.attn_mask"], theirs["layers.0.blocks.1.attn_mask"])
    load_reference_checkpoint(m, {"model": theirs}, family="swin")


def _fixture(name):
    import os
    from fixture_codec import load
    return load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz"))


def test_oracle_window_attention_ws12_matches_reference():
    from fixture_codec import check, group
    from oracle.swin_ref import WindowAttention
    f = _fixture("window_attention_ws12")
    wa = WindowAttention(64, (12, 12), 2)
    res = wa.load_state_dict(group(f, "state"), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for masked in (False, True):
        sfx = "_masked" if masked else ""
        wa.zero_grad()
        x = f["x"].clone().requires_grad_(True)
        y = wa(x, f["mask"]) if masked else wa(x)
        check("y" + sfx, y, f["y" + sfx], 2e-6)
        y.backward(f["dy"])
        check("dx" + sfx, x.grad, f["dx" + sfx], 1e-5)
        for n, p in wa.named_parameters():
            check(f"grad{sfx}[{n}]", p.grad, f[f"grad{sfx}/{n}"], 1e-5)


def test_oracle_swin_tiny_ws12_matches_reference():
    import torch.nn.functional as F
    from fixture_codec import check, group
    from oracle.swin_ref import SwinTransformer
    f = _fixture("swin_tiny_ws12")
    m = SwinTransformer(img_size=96, patch_size=4, in_chans=3, num_classes=10, embed_dim=32, depths=[2, 2],
                        num_heads=[1, 2], window_size=12, drop_path_rate=0.0)
    # the buffers are the oracle's own, pinned to the reference's index and shift mask
    for li, layer in enumerate(m.layers):
        for bi, blk in enumerate(layer.blocks):
            assert torch.equal(blk.attn.relative_position_index, f["relative_position_index"])
    assert torch.equal(m.layers[0].blocks[1].attn_mask, f["attn_mask"])
    assert m.layers[0].blocks[0].attn_mask is None and m.layers[1].blocks[1].attn_mask is None
    res = m.load_state_dict(group(f, "state"), strict=False)
    assert not res.unexpected_keys and all(k.endswith(("relative_position_index", "attn_mask")) for k in res.missing_keys)
    logits = m(f["x"])
    check("logits", logits, f["logits"], 2e-6)
    loss = F.cross_entropy(logits, f["labels"])
    assert abs(loss.item() - f["loss"].item()) < 1e-6
    loss.backward()
    for n, p in m.named_parameters():
        check(f"grad[{n}]", p.grad, f["grad/" + n], 2e-5)
