"""XCA (XCiT's cross-covariance attention) without a GPU: the test reference against the reference's own class
(tests/golden/xca.npz, written by tests/golden/gen_golden_xca.py), the closed-form backward against autograd, the ABI
entries, and the module's construction-time contract."""
import os
import re

import pytest
import torch

import fixture_codec as FC
import xca_util as U
from vit_torch_amd import XCA, VitmiError, _lib

HERE = os.path.dirname(os.path.abspath(__file__))
FP32_GRADE = 2e-6      # the fixture is the reference class in float32; the restatement runs in float64
ENTRIES = ("vitmi_xca_supported", "vitmi_xca_workspace", "vitmi_xca_fwd", "vitmi_xca_bwd")


@pytest.fixture(scope="module")
def fx():
    return FC.load(os.path.join(HERE, "golden", "xca.npz"))


def test_reference_restatement_reproduces_the_reference_class(fx):
    """torch_xca (autograd over the reference's lines) between float64 Linears gives the fixture's y and gradients."""
    st = FC.group(fx, "state")
    x = fx["x"].double().requires_grad_(True)
    B, N, C = x.shape
    H = st["temperature"].shape[0]
    p = {k: v.double().requires_grad_(True) for k, v in st.items()}
    qkv = x @ p["qkv.weight"].T + p["qkv.bias"]
    q, k, v = qkv.reshape(B, N, 3, H, C // H).permute(2, 0, 3, 1, 4)
    q, k, v = q.transpose(-2, -1), k.transpose(-2, -1), v.transpose(-2, -1)
    q, k = torch.nn.functional.normalize(q, dim=-1), torch.nn.functional.normalize(k, dim=-1)
    a = ((q @ k.transpose(-2, -1)) * p["temperature"]).softmax(-1)
    y = (a @ v).permute(0, 3, 1, 2).reshape(B, N, C) @ p["proj.weight"].T + p["proj.bias"]
    y.backward(fx["dy"].double())
    got = {"y": y, "dx": x.grad, **{"grad/" + k: t.grad for k, t in p.items()}}
    # the op alone, through torch_xca, on the same qkv: the attention output that feeds proj
    op = U.torch_xca(qkv.detach().reshape(B, N, 3 * C), torch.zeros(B, N, C), st["temperature"].reshape(H), B, N, H, C // H)
    got_y = op.out @ p["proj.weight"].detach().T + p["proj.bias"].detach()
    assert U.rel(got_y, y.detach()) < 1e-12
    for k in ("y", "dx") + tuple("grad/" + n for n in U.MODULE_KEYS):
        e = U.rel_fixture(got[k], fx[k])
        print(f"\n  {k}: {e:.2e} (bound {FP32_GRADE:.0e})", end="")
        assert e <= FP32_GRADE, f"{k}: {e:.3e}"
    # and the closed-form module restatement the GPU test's bounds come from
    ref = U.module_ref(fx["x"], fx["dy"], st, H)
    for k in ref:
        assert U.rel(ref[k], got[k].detach()) < 1e-12, k


@pytest.mark.parametrize("hd", U.SWEEP_HD)
def test_closed_form_equals_autograd(hd):
    worst = 0.0
    for B, N, H, hd_, seed, temp in U.sweep_cases():
        if hd_ != hd:
            continue
        qkv, dO = U.normal_inputs(B, N, H, hd, seed)
        t = torch.tensor(temp)
        e = U.xca_errors(U.emulated_xca(qkv, dO, t, B, N, H, hd, rounding=False), U.torch_xca(qkv, dO, t, B, N, H, hd),
                         grads=N > 1)
        worst = max(worst, max(e.values()))
        assert max(e.values()) <= 1e-12, f"hd {hd} N {N}: {e}"
    print(f"\n  hd {hd}: worst closed form vs autograd {worst:.2e}", end="")


def test_header_declares_and_lib_binds_the_entries():
    hdr = open(os.path.join(HERE, "..", "include", "vitmi.h")).read()
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} is not declared in include/vitmi.h"
        assert name in _lib.SIGNATURES, f"{name} is not bound in _lib.py"
    assert len(_lib.SIGNATURES["vitmi_xca_fwd"][1]) == 12 and len(_lib.SIGNATURES["vitmi_xca_bwd"][1]) == 14


def test_version_stays_109(lib):
    assert lib.vitmi_version() == 109
    for name in ENTRIES:
        assert hasattr(lib, name)
    assert lib.vitmi_xca_supported(_lib.BF16, 8, 196, 48) == 1 and lib.vitmi_xca_supported(_lib.BF16, 8, 196, 40) == 0
    assert lib.vitmi_xca_supported(_lib.F32, 1, 1, 64) == 1 and lib.vitmi_xca_supported(_lib.BF16, 8, 0, 48) == 0


def test_state_dict_keys_and_shapes(fx):
    st = FC.group(fx, "state")
    m = XCA(96, 3, qkv_bias=True)
    sd = m.state_dict()
    assert set(sd) == set(st) == set(U.MODULE_KEYS)
    for k in sd:
        assert tuple(sd[k].shape) == tuple(st[k].shape), k
    m.load_state_dict(st)
    assert "qkv.bias" not in XCA(96, 3).state_dict()


def test_cpu_tensor_raises():
    with pytest.raises(VitmiError, match="no CPU fallback"):
        XCA(96, 3)(torch.zeros(1, 4, 96))


def test_dropout_raises():
    with pytest.raises(VitmiError, match="dropout"):
        XCA(96, 3, attn_drop=0.1)
    with pytest.raises(VitmiError, match="dropout"):
        XCA(96, 3, proj_drop=0.1)
