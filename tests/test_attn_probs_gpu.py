"""ops.attn_probs (vitmi_attn_probs, csrc/attn_probs.hip): the materialised attention probabilities
P[b,h,i,j] = softmax_j((q_i . k_j) * scale), fp32 [B, H, N, N], that DINO's get_last_selfattention returns.

Every case is compared with a float64 softmax of the SAME q and k (bf16-rounded for the bf16 form), at the token counts
the ViT runs at (145, 197, 785, 1297, 2305 = vitb8 at 384 px) and at ragged ones (1, 50).  The output is pre-filled with
NaN, so an element the kernel never writes fails the finiteness check.  One case writes more than 2^31 elements and is
checked at the (image, head) slices around the 2^31 and 2^32 element offsets and at both ends.

Error metric: max |P - P64| over the tensor (P lies in [0, 1]), and max |sum_j P - 1| over the rows.  Bounds, each
2-3x the largest value measured on an MI355X (in brackets; every check prints its error beside its bound with -s):
  * P: the scores are fp32 sums of exact products (bf16 operands are exact in the fp32 accumulator; fp32 operands go
    through the fp32 matrix pipe), the exponential is the hardware exp2 [bf16 1.2e-7, fp32 3.0e-7]: P_TOL = 8e-7.
  * row sums: N fp32 probabilities of one row [3.0e-7, peaked rows included]: SUM_TOL = 8e-7.
  * peaked rows (qkv scaled 3.5x, median row maximum of P 0.9): scores of a few tens carry a proportionally larger fp32
    rounding into the exponential [bf16 2.0e-6, fp32 7.2e-6]: PEAK_TOL = 2e-5.
"""
import pytest
import torch

from vit_torch_amd import ops
from vit_torch_amd._lib import VitmiError

pytestmark = pytest.mark.gpu

P_TOL = 8e-7
SUM_TOL = 8e-7
PEAK_TOL = 2e-5

CASES = [(2, 6, 197, 64), (1, 12, 785, 64), (3, 12, 145, 64), (2, 4, 1297, 64), (1, 2, 2305, 64), (2, 3, 50, 32),
         (2, 2, 1, 64)]


def make_qkv(B, H, N, hd, dtype, scale=1.0, seed=0):
    g = torch.Generator("cuda").manual_seed(seed)
    qkv = torch.randn(B * N, 3 * H * hd, generator=g, device="cuda") * scale
    return qkv.to(dtype)


def probs64(qkv, B, H, N, hd, scale, bh=None):
    """float64 softmax((q k^T) * scale) of the operands as stored (all (image, head) pairs, or the listed flat ones)."""
    t = qkv.view(B, N, 3, H, hd)
    q, k = t[:, :, 0].permute(0, 2, 1, 3).reshape(B * H, N, hd), t[:, :, 1].permute(0, 2, 1, 3).reshape(B * H, N, hd)
    if bh is not None:
        q, k = q[bh], k[bh]
    q, k = q.double(), k.double()
    return ((q @ k.transpose(-2, -1)) * scale).softmax(dim=-1)


def run(qkv, B, H, N, hd):
    P = torch.full((B, H, N, N), float("nan"), dtype=torch.float32, device="cuda")
    ops.attn_probs(qkv, P, B, N, H, hd, hd ** -0.5)
    torch.cuda.synchronize()
    return P


def check(name, P, want, B, H, N, P_TOL=P_TOL):
    assert torch.isfinite(P).all(), f"{name}: unwritten (NaN) or non-finite elements"
    err = (P.double() - want.view(B, H, N, N)).abs().max().item()
    serr = (P.double().sum(-1) - 1.0).abs().max().item()
    print(f"\n  {name}: max|P - P64| {err:.2e} (bound {P_TOL:.0e}), max|rowsum - 1| {serr:.2e} (bound {SUM_TOL:.0e})",
          end="")
    assert err <= P_TOL, f"{name}: max|P - P64| = {err:.3e} > {P_TOL:.1e}"
    assert serr <= SUM_TOL, f"{name}: max|rowsum - 1| = {serr:.3e} > {SUM_TOL:.1e}"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("B,H,N,hd", CASES, ids=[f"B{c[0]}H{c[1]}N{c[2]}hd{c[3]}" for c in CASES])
def test_probs_against_float64(B, H, N, hd, dtype):
    qkv = make_qkv(B, H, N, hd, dtype)
    P = run(qkv, B, H, N, hd)
    check(f"{dtype} B{B} H{H} N{N} hd{hd}", P, probs64(qkv, B, H, N, hd, hd ** -0.5), B, H, N)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("N", [197, 785])
def test_probs_peaked_rows(N, dtype):
    B, H, hd = 2, 6, 64
    qkv = make_qkv(B, H, N, hd, dtype, scale=3.5, seed=11)
    P = run(qkv, B, H, N, hd)
    print(f"\n  peaked: median row max of P {P.amax(-1).median().item():.3f}", end="")
    check(f"peaked {dtype} N{N}", P, probs64(qkv, B, H, N, hd, hd ** -0.5), B, H, N, P_TOL=PEAK_TOL)


def test_probs_beyond_2_31_elements():
    """B = 256, H = 12, N = 1297: 5.17e9 elements (20.7 GB) of P; 64-bit offsets throughout."""
    B, H, N, hd = 256, 12, 1297, 64
    if torch.cuda.get_device_properties(0).total_memory < 40 * 2**30:
        pytest.fail("this test needs a device with at least 40 GiB (the MI355X has 288 GB)")
    qkv = make_qkv(B, H, N, hd, torch.bfloat16, seed=5)
    P = run(qkv, B, H, N, hd)
    assert P.numel() > 2**32
    P = P.view(B * H, N, N)
    bhs = sorted({0, 2**31 // (N * N), 2**31 // (N * N) + 1, 2**32 // (N * N), 2**32 // (N * N) + 1, B * H - 1})
    got = P[bhs]
    assert torch.isfinite(got).all(), "unwritten (NaN) elements in the checked slices"
    assert torch.isfinite(P[-1, -1]).all() and torch.isfinite(P[-1]).all()
    want = probs64(qkv, B, H, N, hd, hd ** -0.5, bh=torch.tensor(bhs, device="cuda"))
    check(f"2^31+ slices {bhs}", got, want, 1, len(bhs), N)


def test_refusals():
    B, H, N = 1, 2, 10
    P = torch.empty((B, H, N, N), dtype=torch.float32, device="cuda")
    with pytest.raises(VitmiError, match="head dim"):
        ops.attn_probs(make_qkv(B, H, N, 48, torch.bfloat16), P, B, N, H, 48, 48 ** -0.5)
    with pytest.raises(VitmiError, match="bf16 or fp32"):
        ops.attn_probs(make_qkv(B, H, N, 64, torch.float16), P, B, N, H, 64, 0.125)
    with pytest.raises(VitmiError, match="GPU only"):
        ops.attn_probs(make_qkv(B, H, N, 64, torch.bfloat16).cpu(), P.cpu(), B, N, H, 64, 0.125)
