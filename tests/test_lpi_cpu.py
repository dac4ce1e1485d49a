"""LPI (XCiT's local patch interaction) without a GPU: the test reference against the reference's own class
(tests/golden/lpi.npz, written by tests/golden/gen_golden_lpi.py), the closed form against autograd, the ABI entries, and
the module's construction-time contract."""
import os
import re

import pytest
import torch
import torch.nn as nn

import fixture_codec as FC
import lpi_util as U
from vit_torch_amd import LPI, VitmiError, _lib

HERE = os.path.dirname(os.path.abspath(__file__))
FP32_GRADE = 2e-6      # the fixture is the reference class in float32; the restatement runs in float64 (measured: <= 8.4e-7)
ENTRIES = ("vitmi_lpi_supported", "vitmi_lpi_workspace", "vitmi_lpi_fwd", "vitmi_lpi_bwd")
FH, FW = 3, 5


@pytest.fixture(scope="module")
def fx():
    return FC.load(os.path.join(HERE, "golden", "lpi.npz"))


def test_reference_restatement_reproduces_the_reference_class(fx):
    """torch_lpi (autograd over the reference's lines, token-major) gives the fixture's y, gradients, buffers and y_eval."""
    st = FC.group(fx, "state")
    B = fx["x"].shape[0]
    ref = U.torch_lpi(fx["x"], fx["dy"], st, B, FH, FW, training=True)
    got = {"y": ref.out, "dx": ref.dx, **{"grad/" + k: v for k, v in ref.grads.items()},
           "after/bn.running_mean": ref.running_mean, "after/bn.running_var": ref.running_var}
    st2 = dict(st)
    st2["bn.running_mean"], st2["bn.running_var"] = ref.running_mean, ref.running_var
    got["y_eval"] = U.torch_lpi(fx["x"], fx["dy"], st2, B, FH, FW, training=False).out
    for k, v in got.items():
        e = U.rel(fx[k], v)
        print(f"\n  {k}: {e:.2e} (bound {FP32_GRADE:.0e})", end="")
        assert e <= FP32_GRADE, f"{k}: {e:.3e}"
    assert int(fx["after/bn.num_batches_tracked"].item()) == int(st["bn.num_batches_tracked"].item()) + 1
    # and the closed-form module restatement the GPU test's bounds come from
    mod = U.module_ref(fx["x"], fx["dy"], st, FH, FW)
    for k in mod:
        assert U.rel(mod[k], got[k.replace("buf/", "after/")]) < 1e-12, k


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_closed_form_equals_autograd(training):
    worst = 0.0
    for B, H, W, C, seed in U.sweep_cases():
        p = U.make_params(C, seed)
        x, dy = U.make_inputs(B, H, W, C, seed + 50)
        e = U.lpi_errors(U.emulated_lpi(x, dy, p, B, H, W, training=training, rounding=False),
                         U.torch_lpi(x, dy, p, B, H, W, training=training), training)
        worst = max(worst, max(e.values()))
        assert max(e.values()) <= 1e-12, f"C {C} {B}x{H}x{W}: {e}"
    print(f"\n  worst closed form vs autograd {worst:.2e}", end="")


def test_header_declares_and_lib_binds_the_entries():
    hdr = open(os.path.join(HERE, "..", "include", "vitmi.h")).read()
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} is not declared in include/vitmi.h"
        assert name in _lib.SIGNATURES, f"{name} is not bound in _lib.py"
    assert len(_lib.SIGNATURES["vitmi_lpi_fwd"][1]) == 24 and len(_lib.SIGNATURES["vitmi_lpi_bwd"][1]) == 25


def test_version_stays_109(lib):
    assert lib.vitmi_version() == 109
    for name in ENTRIES:
        assert hasattr(lib, name)
    assert lib.vitmi_lpi_supported(_lib.BF16, 2, 3, 5, 96) == 1 and lib.vitmi_lpi_supported(_lib.BF16, 2, 3, 5, 100) == 0
    assert lib.vitmi_lpi_supported(_lib.F32, 1, 1, 1, 8) == 1 and lib.vitmi_lpi_supported(_lib.BF16, 2, 0, 5, 96) == 0
    assert lib.vitmi_lpi_workspace(_lib.BF16, 2, 3, 5, 96) >= 2 * 15 * 96 * 2


def test_state_dict_keys_and_shapes(fx):
    st = FC.group(fx, "state")
    m = LPI(96)
    sd = m.state_dict()
    assert list(sd) == list(U.STATE_KEYS) and set(sd) == set(st)
    for k in sd:
        assert tuple(sd[k].shape) == tuple(st[k].shape), k
    m.load_state_dict(st)
    assert int(m.bn.num_batches_tracked) == 7 and m.bn.num_batches_tracked.dtype == torch.int64
    assert [n for n, _ in m.named_parameters()] == list(U.GRAD_KEYS)


def test_cpu_tensor_raises():
    with pytest.raises(VitmiError, match="no CPU fallback"):
        LPI(96)(torch.zeros(1, 4, 96), 2, 2)


def test_constructor_refusals():
    with pytest.raises(VitmiError, match="kernel_size"):
        LPI(96, kernel_size=5)
    with pytest.raises(VitmiError, match="GELU"):
        LPI(96, act_layer=nn.ReLU)
    with pytest.raises(VitmiError, match="dropout"):
        LPI(96, drop=0.1)
    with pytest.raises(VitmiError, match="out_features"):
        LPI(96, out_features=48)
    with pytest.raises(VitmiError, match="multiple of 8"):
        LPI(100)
    with pytest.raises(VitmiError, match="compute_dtype"):
        LPI(96, compute_dtype="fp16")
    LPI(96, hidden_features=384, out_features=96)        # the reference's call: hidden_features is unused there too
