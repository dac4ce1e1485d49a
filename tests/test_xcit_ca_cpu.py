"""ClassAttentionBlock (XCiT's class-attention block) without a GPU: the float64 restatement against the reference's own
class (tests/golden/xcit_ca.npz, written by tests/golden/gen_golden_xcit_ca.py), the closed-form backward the module runs
against autograd, the bounds that tests/test_xcit_ca_gpu.py freezes, the ABI entries and the module's construction-time
contract."""
import os
import re
from functools import partial

import pytest
import torch
import torch.nn as nn

import fixture_codec as FC
import test_xcit_ca_gpu as GT
import xcit_ca_util as U
from vit_torch_amd import ClassAttentionBlock, VitmiError, _lib

HERE = os.path.dirname(os.path.abspath(__file__))
FP32_GRADE = 2e-6      # the fixture is the reference class in float32; the restatement runs in float64 (measured: <= 7.9e-7)
ENTRIES = ("vitmi_ca_glue_supported", "vitmi_ca_merge_fwd", "vitmi_ca_merge_bwd_workspace", "vitmi_ca_merge_bwd",
           "vitmi_ca_out_fwd", "vitmi_ca_out_bwd")


@pytest.fixture(scope="module")
def fx():
    return FC.load(os.path.join(HERE, "golden", "xcit_ca.npz"))


@pytest.mark.parametrize("name", ["tn", "cls"])
def test_restatement_reproduces_the_reference_class(fx, name):
    x, dy, st, H, tokens_norm, want = U.fixture_case(fx, name)
    assert tuple(x.shape) == (2, 7, 64) and H == 2 and tokens_norm == (name == "tn")
    assert len(set(st["gamma1"].tolist())) > 8 and not (st["gamma1"] == 1).any() and not (st["gamma2"] == 1).any()
    ref = U.torch_block(x, dy, st, H, tokens_norm)
    for k, e in U.fixture_errors(ref, want).items():
        print(f"\n  {name} {k}: {e:.2e} (bound {FP32_GRADE:.0e})", end="")
        assert e <= FP32_GRADE, f"{k}: {e:.3e}"


@pytest.mark.parametrize("tokens_norm", [True, False], ids=["tn", "cls"])
def test_closed_form_backward_equals_autograd(tokens_norm):
    worst = 0.0
    for case in ("single-patch", "n197-hd48", "n785-hd32"):
        x, dy, st, H = U.module_case(case)
        e = U.errors(U.closed_block(x, dy, st, H, tokens_norm), U.module_reference(case, tokens_norm))
        worst = max(worst, max(e.values()))
        assert max(e.values()) <= 1e-12, f"{case}: {e}"
    print(f"\n  worst closed form vs autograd {worst:.2e}", end="")


@pytest.mark.parametrize("case", ["fixture-tn", "fixture-cls"] + [f"{c[0]}-{t}" for c in U.MODULE_CASES for t in ("tn", "cls")])
def test_measured_errors_stay_within_half_of_the_frozen_bounds(fx, case):
    if case.startswith("fixture-"):
        x, dy, st, H, tokens_norm, _ = U.fixture_case(fx, case[8:])
        ref = None
    else:
        name, tokens_norm = case.rsplit("-", 1)[0], case.endswith("-tn")
        x, dy, st, H = U.module_case(name)
        ref = U.module_reference(name, tokens_norm)
    f32, emu = U.measure(x, dy, st, H, tokens_norm, ref)
    print(f"\n  {case}: f32 max {max(f32.values()):.2e}  emu max {max(emu.values()):.2e}", end="")
    for k in U.KEYS:
        assert f32[k] <= GT.module_bound("fp32", case)[k] / 2, (k, f32[k])
        assert emu[k] <= GT.module_bound("bf16", case)[k] / 2, (k, emu[k])


def test_glue_errors_stay_within_half_of_the_frozen_bounds():
    f32, emu = U.glue_measure()
    print(f"\n  f32 {f32}\n  emu {emu}", end="")
    for k in U.GLUE_KEYS:
        assert f32[k] <= GT.glue_bound(torch.float32)[k] / 2 and emu[k] <= GT.glue_bound(torch.bfloat16)[k] / 2, k


def test_header_declares_and_lib_binds_the_entries(lib):
    hdr = open(os.path.join(HERE, "..", "include", "vitmi.h")).read()
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} is not declared in include/vitmi.h"
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.vitmi_version() == 109
    assert lib.vitmi_ca_glue_supported(_lib.BF16, 256, 197, 384) == 1 and lib.vitmi_ca_glue_supported(_lib.F32, 1, 2, 8) == 1
    assert lib.vitmi_ca_glue_supported(_lib.BF16, 2, 1, 64) == 0 and lib.vitmi_ca_glue_supported(_lib.BF16, 2, 7, 60) == 0
    assert lib.vitmi_ca_glue_supported(7, 2, 7, 64) == 0
    assert lib.vitmi_ca_merge_bwd_workspace(256, 197, 384) == 512 * 384 * 4 and lib.vitmi_ca_merge_bwd_workspace(1, 2, 64) == 64 * 4
    assert lib.vitmi_ca_merge_fwd(None, None, None, None, None, _lib.BF16, 2, 7, 60, None) == -4      # refused before any launch
    assert b"multiple of 8" in lib.vitmi_last_error_string()


def test_state_dict_keys_shapes_and_dtypes(fx):
    d = FC.group(fx, "tn")
    listed = [tuple(ln.split(" ", 1)) for ln in bytes(d["keys"].numpy()).decode().split("\n")]
    m = ClassAttentionBlock(64, 2, mlp_ratio=2.0, qkv_bias=True, eta=0.5, tokens_norm=True, norm_layer=partial(nn.LayerNorm, eps=1e-6))
    sd = m.state_dict()
    assert [(k, f"{tuple(v.shape)} {str(v.dtype).replace('torch.', '')}") for k, v in sd.items()] == listed
    assert sorted(sd) == sorted(U.PARAM_KEYS) and m.norm1.eps == 1e-6 and m.norm2.eps == 1e-6
    m.load_state_dict(FC.group(d, "state"))
    assert "attn.qkv.bias" not in ClassAttentionBlock(64, 2, eta=1.0).state_dict()
    assert ClassAttentionBlock(64, 2, eta=1.0).norm1.eps == 1e-5 and ClassAttentionBlock(64, 2, eta=1.0, qk_scale=0.3).scale == 0.3


def test_cpu_tensor_raises():
    m = ClassAttentionBlock(64, 2, eta=1.0)
    with pytest.raises(VitmiError, match="no CPU fallback"):
        m(torch.zeros(1, 7, 64), 2, 3)
    with pytest.raises(VitmiError, match="only holds parameters"):
        m.attn(torch.zeros(1, 7, 64))


def test_constructor_refusals():
    for kw in ({"drop": 0.1}, {"attn_drop": 0.1}, {"drop_path": 0.1}):
        with pytest.raises(VitmiError, match="dropout and drop_path"):
            ClassAttentionBlock(64, 2, eta=1.0, **kw)
    with pytest.raises(VitmiError, match="nn.GELU"):
        ClassAttentionBlock(64, 2, eta=1.0, act_layer=nn.ReLU)
    with pytest.raises(VitmiError, match="eta=None"):
        ClassAttentionBlock(64, 2)
    with pytest.raises(VitmiError, match="head dim"):
        ClassAttentionBlock(256, 2, eta=1.0)            # hd 128
    with pytest.raises(VitmiError, match="head dim"):
        ClassAttentionBlock(72, 6, eta=1.0)             # hd 12
    with pytest.raises(VitmiError, match="head dim"):
        ClassAttentionBlock(64, 3, eta=1.0)
    with pytest.raises(VitmiError, match="compute_dtype"):
        ClassAttentionBlock(64, 2, eta=1.0, compute_dtype="fp16")
    with pytest.raises(VitmiError, match="nn.LayerNorm"):
        ClassAttentionBlock(64, 2, eta=1.0, norm_layer=nn.BatchNorm1d)
