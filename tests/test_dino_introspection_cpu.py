"""DINO's get_last_selfattention / get_intermediate_layers without a GPU: present on every DINO arch of VisionModelZoo,
refusing CPU input with VitmiError (there is no CPU fallback), and bound in the C ABI table.  The numerics are in
tests/test_dino_introspection_gpu.py and tests/test_attn_probs_gpu.py."""
import pytest
import torch

from vit_torch_amd import VisionModelZoo, _lib, ops
from vit_torch_amd._lib import VitmiError


@pytest.mark.parametrize("arch", VisionModelZoo.archs_types["dino"])
def test_every_dino_arch_has_both_methods_and_refuses_cpu_input(arch):
    m = VisionModelZoo.get_model(arch, pretrained=False, classifier=10)
    assert callable(m.get_last_selfattention) and callable(m.get_intermediate_layers)
    x = torch.zeros(1, 3, 32, 32)
    with torch.no_grad():
        with pytest.raises(VitmiError, match="CPU"):
            m.get_last_selfattention(x)
        with pytest.raises(VitmiError, match="CPU"):
            m.get_intermediate_layers(x, 2)


def test_attn_probs_is_bound_and_refuses_cpu_tensors():
    assert "vitmi_attn_probs" in _lib.SIGNATURES
    qkv = torch.zeros(2 * 5, 3 * 2 * 64, dtype=torch.bfloat16)
    P = torch.empty(2, 2, 5, 5)
    with pytest.raises(VitmiError, match="GPU only"):
        ops.attn_probs(qkv, P, 2, 5, 2, 64, 0.125)
