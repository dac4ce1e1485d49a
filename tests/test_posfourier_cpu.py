"""PositionalEncodingFourier (XCiT's Fourier positional encoding) without a GPU: the float64 restatement against the
reference's own class (tests/golden/pos_fourier.npz, written by tests/golden/gen_golden_posfourier.py), the closed-form
backward against autograd, the bounds that tests/test_posfourier_gpu.py freezes, the ABI entries and the module's
construction-time contract."""
import os
import re

import pytest
import torch

import fixture_codec as FC
import posfourier_util as U
import test_posfourier_gpu as GT
from vit_torch_amd import PositionalEncodingFourier, VitmiError, _lib

HERE = os.path.dirname(os.path.abspath(__file__))
FP32_GRADE = 1e-6      # the fixture is the reference class in float32; the restatement runs in float64 (measured: <= 2.3e-7)
ENTRIES = ("vitmi_posfourier_supported", "vitmi_posfourier_features", "vitmi_add_rows_bcast_supported", "vitmi_add_rows_bcast")


@pytest.fixture(scope="module")
def fx():
    return FC.load(os.path.join(HERE, "golden", "pos_fourier.npz"))


@pytest.mark.parametrize("name", list(U.FIXTURE_GRIDS))
def test_restatement_reproduces_the_reference_class(fx, name):
    x, dy, w, b, (H, W), want = U.fixture_case(fx, name)
    assert (H, W) == U.FIXTURE_GRIDS[name] and tuple(x.shape) == (2, H * W, 64)
    ref = U.torch_posenc(x, dy, w, b, H, W)
    for k, e in U.errors(ref, want).items():
        print(f"\n  {name} {k}: {e:.2e} (bound {FP32_GRADE:.0e})", end="")
        assert e <= FP32_GRADE, f"{k}: {e:.3e}"
    cf = U.closed_posenc(x, dy, w, b, H, W)          # the closed-form backward the module runs
    for k in U.KEYS + ("dx",):
        assert U.rel(cf[k], ref[k]) < 1e-12, k
    assert torch.equal(cf["dx"], dy.double())


def test_feature_table_layout():
    """y-features first, then x-features; sin at even and cos at odd indices; the first pixel's coordinate is 1, not 0"""
    H, W = 3, 5
    f = U.features(H, W).view(H, W, 64)
    t = 2 * torch.pi / (H + 1e-6)
    assert abs(f[0, 0, 0].item() - torch.sin(torch.tensor(t, dtype=torch.float64)).item()) < 1e-15
    assert abs(f[0, 0, 1].item() - torch.cos(torch.tensor(t, dtype=torch.float64)).item()) < 1e-15
    assert torch.equal(f[:, 0, :32], f[:, 4, :32]) and torch.equal(f[0, :, 32:], f[2, :, 32:])     # y-features ignore x, and back
    assert not torch.equal(f[0, 0, :32], f[1, 0, :32]) and not torch.equal(f[0, 0, 32:], f[0, 1, 32:])
    assert U.rel(U.features_np32(H, W), U.features(H, W)) < 1e-6


def test_measured_bounds_match_the_frozen_tables(fx):
    """the figures test_posfourier_gpu.py freezes: the float32 table's error, and per fixture grid the float32 closed form's
    and the bf16 emulation's errors against float64; each measured error stays within half of the bound built from the table"""
    e32 = U.table_f32_error()
    print(f"\n  table: numpy float32 vs float64 {e32:.3e} (frozen {GT.F32_TABLE:.2e})", end="")
    assert e32 <= 2 * GT.F32_TABLE
    emu = max(U.rel(U.bf16(U.features(H, W)), U.features(H, W)) for H, W in U.TABLE_GRIDS)
    assert emu <= (2 * GT.EMU_TABLE + 4 * GT.F32_TABLE) / 2
    for name in U.FIXTURE_GRIDS:
        x, dy, w, b, (H, W), _ = U.fixture_case(fx, name)
        f32, em = U.measure(x, dy, w, b, H, W)
        print(f"\n  {name}: f32 {f32}  emu {em}", end="")
        for k in U.KEYS:
            assert f32[k] <= GT.module_bound("fp32", name)[k] / 2, (name, k, f32[k])
            assert em[k] <= GT.module_bound("bf16", name)[k] / 2, (name, k, em[k])


def test_header_declares_and_lib_binds_the_entries(lib):
    hdr = open(os.path.join(HERE, "..", "include", "vitmi.h")).read()
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} is not declared in include/vitmi.h"
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.vitmi_version() == 109
    assert lib.vitmi_posfourier_supported(_lib.BF16, 14, 14, 32) == 1 and lib.vitmi_posfourier_supported(_lib.F32, 1, 1, 32) == 1
    assert lib.vitmi_posfourier_supported(_lib.F32, 14, 14, 64) == 0 and lib.vitmi_posfourier_supported(5, 14, 14, 32) == 0
    assert lib.vitmi_posfourier_supported(_lib.F32, 0, 14, 32) == 0
    assert lib.vitmi_add_rows_bcast_supported(_lib.BF16, 3, 5, 7) == 1 and lib.vitmi_add_rows_bcast_supported(_lib.F32, 0, 5, 7) == 0
    assert lib.vitmi_posfourier_features(None, _lib.F32, 3, 5, 16, 10000.0, None) == -4          # refused before any launch
    assert b"hidden_dim" in lib.vitmi_last_error_string()


def test_state_dict_keys_shapes_and_dtypes(fx):
    d = FC.group(fx, "g3x5")
    listed = [tuple(ln.split(" ", 1)) for ln in bytes(d["keys"].numpy()).decode().split("\n")]
    m = PositionalEncodingFourier(dim=64)
    sd = m.state_dict()
    assert [(k, f"{tuple(v.shape)} {str(v.dtype).replace('torch.', '')}") for k, v in sd.items()] == listed
    assert listed[0] == ("token_projection.weight", "(64, 64, 1, 1) float32")
    m.load_state_dict(FC.group(d, "state"))
    assert tuple(PositionalEncodingFourier().token_projection.weight.shape) == (768, 64, 1, 1)


def test_cpu_tensor_raises():
    m = PositionalEncodingFourier(dim=64)
    with pytest.raises(VitmiError, match="no CPU fallback"):
        m(torch.zeros(1, 15, 64), 3, 5)


def test_constructor_refusals():
    with pytest.raises(VitmiError, match="hidden_dim"):
        PositionalEncodingFourier(hidden_dim=16)
    with pytest.raises(VitmiError, match="compute_dtype"):
        PositionalEncodingFourier(compute_dtype="fp16")
    with pytest.raises(VitmiError, match="multiple of 8"):
        PositionalEncodingFourier(dim=60)
    with pytest.raises(VitmiError, match="temperature"):
        PositionalEncodingFourier(temperature=0)
