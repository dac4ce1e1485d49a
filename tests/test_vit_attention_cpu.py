"""The references of tests/test_vit_attention_gpu.py checked on the CPU: the float64 attention against PyTorch's own
scaled_dot_product_attention, the bf16-rounding emulation against the float64 attention (the frozen bounds of the GPU
module are twice its error: this is what keeps them honest if the emulation is edited), and the inputs of the
padding-leak section."""
import pytest
import torch
import torch.nn.functional as F

import vit_attn_util as U
from test_vit_attention_gpu import DEEP_DK, DEEP_DQ, LEAK_DQ, S1, WALK_BOUNDS
from vit_attn_util import emulated_attention, rel, torch_attention

F64 = torch.float64


@pytest.mark.parametrize("B,N,H,hd", [(2, 197, 3, 64), (3, 5, 2, 32), (1, 300, 2, 64)])
def test_reference_equals_scaled_dot_product_attention(B, N, H, hd):
    scale = hd ** -0.5
    qkv, do = U.normal_inputs(B, N, H, hd, 7)
    r = torch_attention(qkv, do, B, N, H, hd, scale, F64, images_per_chunk=2)
    x = qkv.double().view(B, N, 3, H, hd).clone().requires_grad_(True)
    q, k, v = x.permute(2, 0, 3, 1, 4)
    o = F.scaled_dot_product_attention(q, k, v, scale=scale).transpose(1, 2).reshape(B, N, H * hd)
    o.backward(do.double())
    assert rel(r.out, o.detach()) <= 1e-12 and rel(r.dqkv, x.grad) <= 1e-12
    lse = ((q @ k.transpose(-2, -1)) * scale).detach().logsumexp(-1)
    assert rel(r.lse, lse) <= 1e-12
    # the emulation without its roundings is the closed form of the same gradient
    e = emulated_attention(qkv, do, B, N, H, hd, scale, F64, rounding=False)
    assert rel(e.out, r.out) <= 1e-12 and rel(e.lse, r.lse) <= 1e-12 and rel(e.dqkv, r.dqkv) <= 1e-12


def test_emulation_stays_within_half_the_frozen_bounds():
    """Every section-1 N at hd 64 (B = 2, H = 3, the GPU test's seeds): out, dq, dk, dv and the bias sums."""
    B, H, hd = 2, 3, 64
    worst = {}
    for N in U.sweep_ns(True):
        qkv, do = U.normal_inputs(B, N, H, hd, 1000 + N)
        w = torch_attention(qkv, do, B, N, H, hd, hd ** -0.5)
        e = U.errors(emulated_attention(qkv, do, B, N, H, hd, hd ** -0.5), w)
        assert e.pop("lse") <= 1e-12
        for k, v in e.items():
            assert v <= S1[k] / 2, f"N {N}: emulated {k} differs from float64 by {v:.3e} > {S1[k] / 2:.2e}"
            worst[k] = max(worst.get(k, 0.0), v)
    print("\n  emulation, hd 64: " + ", ".join(f"{k} {v:.2e} (bound / 2 = {S1[k] / 2:.2e})" for k, v in worst.items()))


def test_emulation_stays_within_half_the_walk_bounds_at_the_one_wave_shape():
    """C1 (128 images of 5 tokens, 6 heads) with the per-pair scales, per pair."""
    B, N, H, hd = 128, 5, 6, 64
    qkv, do = U.pair_scaled_inputs(B, N, H, hd, 3000 + N)
    w = torch_attention(qkv, do, B, N, H, hd, hd ** -0.5)
    g = emulated_attention(qkv, do, B, N, H, hd, hd ** -0.5)
    b = WALK_BOUNDS["C1"]
    assert U.per_pair_rel(g.out.view(B, N, H, hd), w.out.view(B, N, H, hd)).max().item() <= b["out"] / 2
    for i, nm in enumerate("qkv"):
        assert U.per_pair_rel(g.dqkv[:, :, i], w.dqkv[:, :, i]).max().item() <= b["d" + nm] / 2


@pytest.mark.parametrize("N", U.LEAK_NS + U.LEAK_NS_STREAM)
def test_a_leaked_key_is_gross_on_the_leak_inputs(N):
    """Every scaled score lies well below zero, one zero-padded key moves the float64 O by more than 100x the bound
    on O, and the emulation stays within half the bounds the GPU test applies to these inputs."""
    B, H, hd = 2, 3, 64
    scale = hd ** -0.5
    qkv, do = U.leak_inputs(B, N, H, hd, scale, 2000 + N)
    x = qkv.double().view(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)
    s = (x[0] @ x[1].transpose(-2, -1)) * scale
    assert -14.5 <= s.min().item() and s.max().item() <= -4.0
    assert U.leaked_key_effect(qkv, B, N, H, hd, scale) > 100 * S1["out"]
    e = U.errors(emulated_attention(qkv, do, B, N, H, hd, scale), torch_attention(qkv, do, B, N, H, hd, scale))
    assert e["out"] <= S1["out"] / 2 and e["dk"] <= S1["dk"] / 2 and e["dv"] <= S1["dv"] / 2
    assert e["dq"] <= LEAK_DQ / 2


@pytest.mark.parametrize("N", [5, 197])
def test_emulation_on_the_inputs_far_below_zero(N):
    """Scores about -120: every lse below -100 (exp(-lse) overflows fp32), the emulation within half the bounds."""
    B, H, hd = 2, 3, 64
    scale = hd ** -0.5
    qkv, do = U.leak_inputs(B, N, H, hd, scale, 6000 + N, depth=120.0)
    w = torch_attention(qkv, do, B, N, H, hd, scale)
    assert w.lse.max().item() < -100
    e = U.errors(emulated_attention(qkv, do, B, N, H, hd, scale), w)
    assert e["out"] <= S1["out"] / 2 and e["dv"] <= S1["dv"] / 2
    assert e["dq"] <= DEEP_DQ / 2 and e["dk"] <= DEEP_DK / 2
