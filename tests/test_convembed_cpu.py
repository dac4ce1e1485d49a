"""ConvPatchEmbed (XCiT's conv stem) without a GPU: the test reference against the reference's own class
(tests/golden/conv_patch_embed.npz, written by tests/golden/gen_golden_convembed.py), the closed form against autograd, the
premise of the exact gather tests, the ABI entries, and the module's construction-time contract."""
import os
import re

import pytest
import torch

import convembed_util as U
import fixture_codec as FC
from vit_torch_amd import ConvPatchEmbed, VitmiError, _lib

HERE = os.path.dirname(os.path.abspath(__file__))
FP32_GRADE = 4e-6      # the fixture is the reference class in float32; the restatement runs in float64 (measured: <= 1.72e-6)
ENTRIES = ("vitmi_conv3s2_supported", "vitmi_conv3s2_im2col", "vitmi_conv3s2_col2im", "vitmi_conv3s2_wcopy",
           "vitmi_bn_act_supported", "vitmi_bn_act_workspace", "vitmi_bn_act_fwd", "vitmi_bn_act_bwd")


@pytest.fixture(scope="module")
def fx():
    return FC.load(os.path.join(HERE, "golden", "conv_patch_embed.npz"))


@pytest.mark.parametrize("name", ["p16", "p8"])
def test_reference_restatement_reproduces_the_reference_class(fx, name):
    x, dy, st, patch, want = U.fixture_case(fx, name)
    ref = U.torch_stem(x, dy, st, patch, True)
    st2 = dict(st)
    st2.update({k[4:]: v for k, v in ref.items() if k.startswith("buf/")})
    ref["y_eval"] = U.torch_stem(x, None, st2, patch, False)["y"]
    for k, e in U.module_errors(ref, want).items():
        print(f"\n  {name} {k}: {e:.2e} (bound {FP32_GRADE:.0e})", end="")
        assert e <= FP32_GRADE, f"{k}: {e:.3e}"
    d = FC.group(fx, name)
    assert tuple(d["grid"].tolist()) == {"p16": (2, 2), "p8": (3, 5)}[name]
    for k in U.buffer_keys(patch):
        if k.endswith("tracked"):
            assert int(d["after/" + k]) == int(st[k]) + 1
    cf = U.closed_stem(x, dy, st, patch, True)          # the closed form the GPU test's bounds come from
    for k in want:
        if k != "y_eval":
            assert U.rel(cf[k], ref[k]) < 1e-12, k


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("gelu", [True, False], ids=["gelu", "plain"])
def test_bn_act_closed_form_equals_autograd(gelu, training):
    """1e-11: at M = 2 the training dy is a cancellation (yh = +-1 exactly), so float64 itself carries ~6e-13 there"""
    worst = 0.0
    for M, C, seed in U.bn_cases():
        p = U.bn_params(C, seed)
        y, d = U.bn_inputs(M, C, seed + 50)
        e = U.bn_errors(U.closed_bn_act(y, d, p, gelu, training), U.torch_bn_act(y, d, p, gelu, training), training)
        worst = max(worst, max(e.values()))
        assert max(e.values()) <= 1e-11, f"M {M} C {C}: {e}"
    print(f"\n  worst closed form vs autograd {worst:.2e}", end="")


def test_fold_of_grid_values_is_exact_in_every_dtype():
    """the premise of the exact col2im test: float64 F.fold of multiples of 1/8 in [-2, 2] equals its float32 and its
    bf16-rounded value, and unfold / fold are transposes of each other"""
    for H, W in U.GATHER_GRIDS:
        Ho, Wo = U.out_grid(H, W)
        dc = U.grid_values((3 * Ho * Wo, 72), 31 * H + W)
        f64 = U.fold_cols(dc.double(), 3, H, W)
        assert torch.equal(f64, U.fold_cols(dc, 3, H, W).double()), (H, W)
        assert torch.equal(U.bf16(f64.float()).double(), f64) and f64.abs().max() <= 8, (H, W)
        x = U.grid_values((3, 8, H, W), 7 * H + W).double()
        assert torch.equal((U.unfold_cols(x) * dc.double()).sum(), (x * f64).sum()), (H, W)


def test_header_declares_and_lib_binds_the_entries():
    hdr = open(os.path.join(HERE, "..", "include", "vitmi.h")).read()
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} is not declared in include/vitmi.h"
        assert name in _lib.SIGNATURES, f"{name} is not bound in _lib.py"
    assert len(_lib.SIGNATURES["vitmi_bn_act_fwd"][1]) == 18 and len(_lib.SIGNATURES["vitmi_bn_act_bwd"][1]) == 16
    assert len(_lib.SIGNATURES["vitmi_conv3s2_im2col"][1]) == 14


def test_version_stays_109(lib):
    assert lib.vitmi_version() == 109
    for name in ENTRIES:
        assert hasattr(lib, name)
    assert lib.vitmi_bn_act_supported(_lib.BF16, 50, 96) == 1 and lib.vitmi_bn_act_supported(_lib.BF16, 50, 100) == 0
    assert lib.vitmi_bn_act_supported(_lib.F32, 1, 8) == 1 and lib.vitmi_bn_act_supported(5, 50, 96) == 0
    assert lib.vitmi_bn_act_workspace(_lib.BF16, 4100, 96) >= 2 * 96 * 8
    assert lib.vitmi_conv3s2_supported(_lib.BF16, 0, 2, 7, 9, 24, 216) == 1
    assert lib.vitmi_conv3s2_supported(_lib.BF16, 0, 2, 7, 9, 24, 220) == 0        # ld not a multiple of 8
    assert lib.vitmi_conv3s2_supported(_lib.BF16, 0, 2, 7, 9, 12, 112) == 0        # C not a multiple of 8
    assert lib.vitmi_conv3s2_supported(_lib.F32, 1, 2, 7, 9, 3, 32) == 1 and lib.vitmi_conv3s2_supported(_lib.F32, 1, 2, 7, 9, 4, 40) == 0


@pytest.mark.parametrize("name", ["p16", "p8"])
def test_state_dict_keys_shapes_and_dtypes(fx, name):
    d = FC.group(fx, name)
    listed = [ln.split(" ", 1) for ln in bytes(d["keys"].numpy()).decode().split("\n")]
    patch = 16 if name == "p16" else 8
    m = ConvPatchEmbed(img_size=32, patch_size=patch, embed_dim=64)
    sd = m.state_dict()
    assert [(k, f"{tuple(v.shape)} {str(v.dtype).replace('torch.', '')}") for k, v in sd.items()] == [(k, v) for k, v in listed]
    st = FC.group(d, "state")
    assert set(sd) == set(st)
    m.load_state_dict(st)
    assert int(m.proj[2][1].num_batches_tracked) == 8 and m.proj[2][1].num_batches_tracked.dtype == torch.int64
    assert [n for n, _ in m.named_parameters()] == U.param_keys(patch)


def test_cpu_tensor_raises():
    with pytest.raises(VitmiError, match="no CPU fallback"):
        ConvPatchEmbed(32, 16, embed_dim=64)(torch.zeros(1, 3, 32, 32))


def test_constructor_refusals():
    with pytest.raises(VitmiError, match="in_chans"):
        ConvPatchEmbed(in_chans=1)
    with pytest.raises(VitmiError, match="8 or 16"):
        ConvPatchEmbed(patch_size=4)
    with pytest.raises(VitmiError, match="multiple of 64"):
        ConvPatchEmbed(patch_size=16, embed_dim=96)
    with pytest.raises(VitmiError, match="multiple of 32"):
        ConvPatchEmbed(patch_size=8, embed_dim=48)
    with pytest.raises(VitmiError, match="compute_dtype"):
        ConvPatchEmbed(compute_dtype="fp16")
    m = ConvPatchEmbed(224, 16, 3, 384)
    assert m.num_patches == 196 and [c[0].weight.shape[0] for c in m.proj if not isinstance(c, torch.nn.GELU)] == [48, 96, 192, 384]
    assert ConvPatchEmbed(224, 8, 3, 96).num_patches == 784
