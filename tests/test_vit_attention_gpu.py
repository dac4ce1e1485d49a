"""Plain multi-head attention (attention.hip, attention_f32.hip) on every dispatch path against a float64 PyTorch
reference (tests/vit_attn_util.py), at the shapes where the kernels go wrong: every sequence length around the 32-row
blocks and the 256-row switch to the streaming kernels, inputs on which a leaked padded key is a gross error, the
persistent walk of the fused backward at the shapes training runs, determinism of the backward, stores outside the
output tensors, and the refusals.

Paths (each case forces its own with the vitmi_debug_* switches, starting from vitmi_debug_reset):
  bf16.whole   N <= 256   attn_fwd_whole_kernel            attn_bwd_fused_kernel
  bf16.stream  any N      attn_fwd_kernel (4 waves)        attn_delta + attn_bwd_dkdv + attn_bwd_dq kernels
  fp32.matrix  N <= 256   attn_fwd_f32m_kernel             attn_bwd_dq_f32m + attn_bwd_dkdv_f32m kernels
  fp32.valu    any N      attn_fwd_f32_kernel              attn_delta_f32 + attn_bwd_dq_f32 + attn_bwd_dkdv_f32 kernels

Error metric: max |got - want| / max |want| (vit_attn_util.rel), per tensor in sections 1-2, per (image, head) pair in
section 3.  dq and dk at N = 1 are exact zeros in the reference and are measured against max |dv|.  Both sides see the
same bf16-rounded operands in both dtypes.  Bounds (largest value measured on an MI355X in brackets; every test prints
its errors beside their bounds with -s):
  * fp32 paths, and lse on every path: FP32_GRADE = 2e-6 (fp32 sums of exact bf16 products)
    [fp32.matrix out 8.8e-7, lse 1.6e-7, dq 9.2e-7, dk 1.0e-6, dv 8.6e-7; fp32.valu 1.3e-6 / 1.5e-7 / 1.7e-6 / 8.8e-7 /
    6.7e-7, its largest at N = 1025; bf16 lse 1.5e-7].  fp32.valu's dk measured 2.9e-6 at N = 1025 while
    attn_bwd_dkdv_f32_kernel summed all N queries in one fp32 chain; it now sums each 64-query tile from zero.
  * bf16 O, dq, dk, dv: 2x the largest error that vit_attn_util.emulated_attention (float64 with only the kernels'
    declared roundings: P, dS, O, dq/dk/dv to bf16, delta from the rounded O) shows against float64 over the section's
    own inputs, measured on the CPU and frozen below.  The factor 2 covers fp32 instead of float64 accumulation, the
    hardware exp2 and a rounding placed one operation earlier or later than the emulation's.
      section 1 (emulation: out 4.01e-3 at N 100, dq 7.18e-3 at N 2, dk 9.63e-3 at hd 32 N 2, dv 5.30e-3 at N 38):
        S1 = out 8.1e-3, dq 1.44e-2, dk 1.93e-2, dv 1.07e-2
        [bf16.whole out 4.0e-3, dq 7.2e-3, dk 9.6e-3, dv 5.3e-3; bf16.stream the same: the emulation's own figures]
      section 2 uses S1 except for dq, which is ill-conditioned on those inputs (sum_k dS K with sum_k dS = 0 and K
        carrying the common -u; emulation 4.31e-2 at N 577): LEAK_DQ = 8.7e-2 [whole 2.2e-2 at N 255, stream 4.3e-2 at N 577;
        fp32: see the test].
      section 3, per pair and per shape (emulation C2: out 4.49e-3, dq 7.18e-3, dk 6.32e-3, dv 7.13e-3; C3: 4.80e-3,
        6.37e-3, 6.62e-3, 5.96e-3; C1: 4.27e-3, 1.08e-2, 1.17e-2, 5.90e-3; S8: 3.69e-3, 5.36e-3, 5.36e-3, 5.32e-3):
        WALK_BOUNDS below [C2 4.8e-3 / 7.5e-3 / 6.3e-3 / 7.1e-3, C3 4.8e-3 / 6.4e-3 / 6.6e-3 / 6.0e-3 on both paths,
        C1 4.3e-3 / 1.1e-2 / 1.2e-2 / 5.9e-3, S8 3.7e-3 / 5.4e-3 / 5.4e-3 / 5.3e-3; batch-summed bias q third 1.7e-3 ...
        3.9e-3, fused v third 1.3e-8].
  * dbias_part (bf16 only; per-image sums in section 1, batch sums in section 3): the q third, and on the streaming
    path the k and v thirds, 2x the emulation's column-sum error (the k third, whose reference is rounding noise around
    zero, relative to max |q third|): section 1 BQ 1.25e-2, BK 1.55e-2, BV 5.9e-3 (emulation 6.23e-3, 7.70e-3,
    2.93e-3, all at N 2-3) [whole bq 6.2e-3; stream 6.4e-3 / 7.5e-3 / 1.7e-3].  On the fused path the k third is
    exact zeros and the v third an fp32 column sum of exact bf16 dO against a float64 one, bound 1e-5 [6.0e-8].  On every path
    the reference itself must satisfy |sum_k dK| <= 1e-4 max |sum dQ| first [1e-15].
"""
import functools

import pytest
import torch

import vit_attn_util as U
from vit_attn_util import AttentionRef, emulated_attention, rel, torch_attention

pytestmark = pytest.mark.gpu

F64 = torch.float64
FP32_GRADE = 2e-6
S1 = {"out": 8.1e-3, "dq": 1.44e-2, "dk": 1.93e-2, "dv": 1.07e-2, "bq": 1.25e-2, "bk": 1.55e-2, "bv": 5.9e-3}
FUSED_BV = 1e-5                        # v third of the fused path against float64 column sums of dO
LEAK_DQ = 8.7e-2
DEEP_DQ, DEEP_DK = 6.5e-2, 3.6e-2       # scores about -120 (test_padded_keys_stay_harmless_far_below_zero)
# per pair: out, dq, dk, dv; batch-summed bias thirds bq, bk (relative to max |bq|), bv
WALK_BOUNDS = {
    "C2": {"out": 9.0e-3, "dq": 1.44e-2, "dk": 1.27e-2, "dv": 1.43e-2, "bq": 5.2e-3, "bk": 7.8e-3, "bv": 5.5e-4},
    "C3": {"out": 9.7e-3, "dq": 1.28e-2, "dk": 1.33e-2, "dv": 1.20e-2, "bq": 4.2e-3, "bk": 6.3e-3, "bv": 7.3e-4},
    "C1": {"out": 8.6e-3, "dq": 2.17e-2, "dk": 2.35e-2, "dv": 1.19e-2, "bq": 7.9e-3, "bk": 8.8e-3, "bv": 2.81e-3},
    "S8": {"out": 7.4e-3, "dq": 1.08e-2, "dk": 1.08e-2, "dv": 1.07e-2, "bq": 4.5e-3, "bk": 5.6e-3, "bv": 2.71e-4},
}

PATHS = ["bf16.whole", "bf16.stream", "fp32.matrix", "fp32.valu"]
ANY_N = ("bf16.stream", "fp32.valu")


@pytest.fixture(scope="module")
def ops(lib):
    from vit_torch_amd import ops as _o
    return _o


def force(lib, path):
    """Every switch to its default, then this path's own; returns the path's dtype."""
    lib.vitmi_debug_reset()
    if path == "bf16.whole":
        lib.vitmi_debug_attn_bwd(1)
    elif path == "bf16.stream":
        lib.vitmi_debug_attn_fwd_waves(4)
        lib.vitmi_debug_attn_bwd(0)
    elif path == "fp32.valu":
        lib.vitmi_debug_attn_f32_valu(1)
    else:
        assert path == "fp32.matrix"
    return torch.bfloat16 if path.startswith("bf16") else torch.float32


def nan(shape, dt):
    return torch.full(shape, float("nan"), device="cuda", dtype=dt)


def bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def forward(ops, Q, B, N, H, hd, scale):
    O, lse = nan((B, N, H * hd), Q.dtype), nan((B * H * N,), torch.float32)
    ops.attn_fwd(Q, O, lse, B, N, H, hd, scale)
    return O, lse


def backward(ops, Q, O, DO, lse, B, N, H, hd, scale, dbias=False, flags=0):
    dqkv = nan((B, N, 3 * H * hd), Q.dtype)
    part = nan((ops.attn_bwd_dbias_rows(B, N), 3 * H * hd), torch.float32) if dbias else None
    ops.attn_bwd(Q, O, DO, lse, dqkv, B, N, H, hd, scale, dbias_part=part, launch_flags=flags)
    return dqkv, part


def run(ops, qkv, do, B, N, H, hd, dt, dbias=False, flags=0):
    """forward + backward (fed the kernel's own O, as the engine does) on the device, every output NaN-filled first;
    returns (AttentionRef on the CPU, dbias_part or None)."""
    scale = hd ** -0.5
    Q, DO = qkv.to("cuda", dt).contiguous(), do.to("cuda", dt).contiguous()
    O, lse = forward(ops, Q, B, N, H, hd, scale)
    dqkv, part = backward(ops, Q, O, DO, lse, B, N, H, hd, scale, dbias, flags)
    torch.cuda.synchronize()
    return AttentionRef(O.cpu(), lse.view(B, H, N).cpu(), dqkv.view(B, N, 3, H, hd).cpu()), part


def check(name, e, bound, failures=None):
    """An error printed beside its bound, then asserted (or collected, when a case loops over N)."""
    print(f"\n  {name}: {e:.2e} (bound {bound:.2e})", end="")
    ok = e <= bound            # False for NaN too
    if failures is None:
        assert ok, f"{name}: rel-to-max error {e:.3e} > {bound:.2e}"
    elif not ok:
        failures.append(f"{name}: {e:.3e} > {bound:.2e}")
    return e


def finite(name, got, part=None):
    for k, t in (("out", got.out), ("lse", got.lse), ("dqkv", got.dqkv), ("dbias_part", part)):
        if t is not None:
            assert torch.isfinite(t).all(), f"{name}.{k}: non-finite values (an output element was not written?)"


def image_sums(part, B, H, hd):
    """dbias_part [rows, 3*H*hd] -> float64 per-image sums [B,3,H,hd] on the CPU."""
    return part.double().view(B, -1, 3, H, hd).sum(1).cpu()


@functools.lru_cache(maxsize=4)
def reference(kind, B, N, H, hd, seed, chunk=None):
    scale = hd ** -0.5
    qkv, do = {"normal": lambda: U.normal_inputs(B, N, H, hd, seed),
               "leak": lambda: U.leak_inputs(B, N, H, hd, scale, seed),
               "pairs": lambda: U.pair_scaled_inputs(B, N, H, hd, seed)}[kind]()
    return qkv, do, torch_attention(qkv, do, B, N, H, hd, scale, F64, chunk)


def compare(name, path, got, want, bounds, failures=None):
    """out, lse, dq, dk, dv of one launch against float64; returns the errors."""
    f32 = path.startswith("fp32")
    den = U.grad_denoms(want.dqkv)
    e = {"out": check(f"{name}.out", rel(got.out, want.out), FP32_GRADE if f32 else bounds["out"], failures),
         "lse": check(f"{name}.lse", rel(got.lse, want.lse), FP32_GRADE, failures)}
    for i, nm in enumerate("qkv"):
        e["d" + nm] = check(f"{name}.d{nm}", rel(got.dqkv[:, :, i], want.dqkv[:, :, i], den[i]),
                            FP32_GRADE if f32 else bounds["d" + nm], failures)
    return e


def compare_bias(name, path, ops, qkv, do, got, part, want, B, N, H, hd, dt, bounds, failures):
    """dbias_part of a bf16 path: same dqkv bits without it, then the q, k, v thirds."""
    got2, _ = run(ops, qkv, do, B, N, H, hd, dt)
    if not torch.equal(bits(got2.dqkv), bits(got.dqkv)):
        failures.append(f"{name}: dqkv differs with and without dbias_part")
    bw = U.bias_sums(want.dqkv)
    qden = bw[:, 0].abs().max().item() or bw[:, 2].abs().max().item()
    assert bw[:, 1].abs().max().item() <= 1e-4 * bw[:, 0].abs().max().item(), f"{name}: reference sum_k dK is not ~0"
    bg = image_sums(part, B, H, hd)
    e = {"bq": check(f"{name}.bias_q", rel(bg[:, 0], bw[:, 0], qden), bounds["bq"], failures)}
    if path == "bf16.whole":
        nz = int(torch.count_nonzero(bg[:, 1]))
        if nz:
            failures.append(f"{name}.bias_k: {nz} non-zero entries on the fused path")
        e["bv"] = check(f"{name}.bias_v", rel(bg[:, 2], do.double().view(B, N, H, hd).sum(1)), FUSED_BV, failures)
    else:
        e["bk"] = check(f"{name}.bias_k", rel(bg[:, 1], bw[:, 1], qden), bounds["bk"], failures)
        e["bv"] = check(f"{name}.bias_v", rel(bg[:, 2], bw[:, 2]), bounds["bv"], failures)
    return e


# ------------------------------------------------------------------------------ 1. N sweep against float64 ---
@pytest.mark.parametrize("hd", [64, 32])
@pytest.mark.parametrize("path", PATHS)
def test_n_sweep_against_float64(ops, lib, path, hd):
    """B = 2, H = 3 (image, head and q/k/v strides all differ), every N of vit_attn_util.sweep_ns the path takes."""
    B, H = 2, 3
    dt = force(lib, path)
    failures, worst = [], {}
    for N in U.sweep_ns(path in ANY_N):
        qkv, do, want = reference("normal", B, N, H, hd, 1000 + N)
        name = f"{path}.hd{hd}.N{N}"
        got, part = run(ops, qkv, do, B, N, H, hd, dt, dbias=dt == torch.bfloat16)
        finite(name, got, part)
        e = compare(name, path, got, want, S1, failures)
        if dt == torch.bfloat16:
            e.update(compare_bias(name, path, ops, qkv, do, got, part, want, B, N, H, hd, dt, S1, failures))
        for k, v in e.items():
            if v >= worst.get(k, (-1.0, 0))[0]:
                worst[k] = (v, N)
    print(f"\n  {path}.hd{hd} worst: " + ", ".join(f"{k} {v:.2e} at N {n}" for k, (v, n) in worst.items()), end="")
    assert not failures, "; ".join(failures)


# ---------------------------------------------------------------------------------- 2. padding must not leak ---
LEAK_CASES = [(p, n) for p in PATHS for n in U.LEAK_NS + (U.LEAK_NS_STREAM if p in ANY_N else [])]


@pytest.mark.parametrize("path,N", LEAK_CASES)
def test_padding_does_not_leak(ops, lib, path, N):
    """Inputs (vit_attn_util.leak_inputs) on which every real score is about -9, so a zero-padded key (score 0) would
    take 93-100 % of every softmax row: O moves by 0.9-1.0 rel-to-max, which the test first asserts on the float64
    reference alone (more than 100x the bound on O).  Then forward and backward at the section-1 bounds, dq at
    LEAK_DQ.  In fp32 dq's cancellation amplifies the fp32 roundings as it does the bf16 ones: its bound is
    FP32_GRADE times the ratio LEAK_DQ / S1['dq'] = 6.0 of the two emulation floors, 1.2e-5 [fp32.matrix 4.2e-6 at N 255,
    fp32.valu 1.14e-5 at N 577; every other fp32 output on these inputs <= 1.4e-6]."""
    B, H, hd = 2, 3, 64
    scale = hd ** -0.5
    qkv, do, want = reference("leak", B, N, H, hd, 2000 + N)
    effect = U.leaked_key_effect(qkv, B, N, H, hd, scale)
    print(f"\n  leak.N{N}: one zero key moves float64 O by {effect:.3f}", end="")
    assert effect > 100 * S1["out"]
    dt = force(lib, path)
    name = f"leak.{path}.N{N}"
    got, _ = run(ops, qkv, do, B, N, H, hd, dt)
    finite(name, got)
    f32 = dt == torch.float32
    den = U.grad_denoms(want.dqkv)
    check(f"{name}.out", rel(got.out, want.out), FP32_GRADE if f32 else S1["out"])
    check(f"{name}.lse", rel(got.lse, want.lse), FP32_GRADE)
    check(f"{name}.dq", rel(got.dqkv[:, :, 0], want.dqkv[:, :, 0], den[0]),
          FP32_GRADE * LEAK_DQ / S1["dq"] if f32 else LEAK_DQ)
    check(f"{name}.dk", rel(got.dqkv[:, :, 1], want.dqkv[:, :, 1], den[1]), FP32_GRADE if f32 else S1["dk"])
    check(f"{name}.dv", rel(got.dqkv[:, :, 2], want.dqkv[:, :, 2], den[2]), FP32_GRADE if f32 else S1["dv"])


@pytest.mark.parametrize("N", [5, 197])
@pytest.mark.parametrize("path", ["bf16.whole", "bf16.stream"])
def test_padded_keys_stay_harmless_far_below_zero(ops, lib, path, N):
    """The same inputs with every real score about -120, so lse < -100: for a zero-padded key the backward's
    p = exp(0 - lse) overflows fp32.  The fused backward zeroes p for its padded keys; unzeroed, the infinite dS would
    meet the zero K rows in the dQ product as inf * 0 = NaN.  (At scores about -9 that p is finite and multiplies
    zeros: dropping the select changes no output there.)  K carries the common -u more heavily here, so dq and dk get
    their own constants by the same rule (emulation 3.24e-2 and 1.79e-2 at N 197): DEEP_DQ, DEEP_DK [both paths 3.2e-2,
    1.9e-2].  attn_bwd_dq_kernel did not zero its padded keys' dS and returned NaN rows of dq on these inputs at both N;
    it now zeroes them in the ragged key block."""
    B, H, hd = 2, 3, 64
    scale = hd ** -0.5
    qkv, do = U.leak_inputs(B, N, H, hd, scale, 6000 + N, depth=120.0)
    want = torch_attention(qkv, do, B, N, H, hd, scale)
    assert want.lse.max().item() < -100
    dt = force(lib, path)
    name = f"deep.{path}.N{N}"
    got, part = run(ops, qkv, do, B, N, H, hd, dt, dbias=True)
    finite(name, got, part)
    compare(name, path, got, want, dict(S1, dq=DEEP_DQ, dk=DEEP_DK))


# ------------------------------------------------------------- 3. the walk at training shapes, against float64 ---
# (B, N, H) at hd 64: ViT-B/16 batch 256 (C2), 145 tokens batch 128 (C3), 5 tokens 6 heads batch 128 (C1: one-wave
# workgroups), ViT-S/8 at 224 px (S8: the streaming kernels with real image and head strides)
WALK_SHAPES = {"C2": (256, 197, 12), "C3": (128, 145, 12), "C1": (128, 5, 6), "S8": (8, 785, 6)}
WALK_CASES = [("C2", "bf16.whole"), ("C3", "bf16.whole"), ("C1", "bf16.whole"), ("S8", "bf16.stream"),
              ("C3", "bf16.stream")]


@pytest.mark.parametrize("case,path", WALK_CASES)
def test_walk_at_training_shapes(ops, lib, case, path):
    """Full batch, v and dO of pair (b, h) scaled by 2^k, k = (b * H + h) mod 7 - 3, and the error taken per pair: a
    value staged for the wrong pair (lse, delta, V fragments, the dO column sums) is wrong by a factor, not by a
    rounding.  The persistent launch (workgroups walk pairs bh, bh + grid, ...: 12 / 6 / 3 per workgroup at C2 / C3 /
    C1 on 256 CUs) and the one-pair-per-workgroup launch agree bit for bit, dbias_part included; the batch-summed
    qkv-bias gradient against float64."""
    from vit_torch_amd._lib import LAUNCH_SHARED_DEVICE
    B, N, H = WALK_SHAPES[case]
    hd = 64
    bounds = WALK_BOUNDS[case]
    qkv, do, want = reference("pairs", B, N, H, hd, 3000 + N, 16)
    dt = force(lib, path)
    if path == "bf16.whole":
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        print(f"\n  walk.{case}: {B * H} pairs on {cus} CUs", end="")
        assert B * H > 2 * cus, "the walk no longer reaches its steady state (three pairs per workgroup) on this part"
    name = f"walk.{case}.{path}"
    got, part = run(ops, qkv, do, B, N, H, hd, dt, dbias=True)
    got1, part1 = run(ops, qkv, do, B, N, H, hd, dt, dbias=True, flags=LAUNCH_SHARED_DEVICE)
    finite(name, got, part)
    assert torch.equal(bits(got.dqkv), bits(got1.dqkv)), f"{name}: dqkv differs between the two launch forms"
    assert torch.equal(part, part1), f"{name}: dbias_part differs between the two launch forms"
    del got1, part1
    failures = []

    def per_pair(tag, g, w, bound):
        e = U.per_pair_rel(g, w)
        i = int(e.argmax())
        check(f"{name}.{tag} (worst pair b {i // H}, h {i % H})", e.max().item(), bound, failures)

    per_pair("out", got.out.view(B, N, H, hd), want.out.view(B, N, H, hd), bounds["out"])
    check(f"{name}.lse", rel(got.lse, want.lse), FP32_GRADE, failures)
    for i, nm in enumerate("qkv"):
        per_pair("d" + nm, got.dqkv[:, :, i], want.dqkv[:, :, i], bounds["d" + nm])
    bw = want.dqkv.sum((0, 1))
    bg = part.double().sum(0).view(3, H, hd).cpu()
    qden = bw[0].abs().max().item()
    assert bw[1].abs().max().item() <= 1e-4 * qden
    check(f"{name}.bias_q", rel(bg[0], bw[0]), bounds["bq"], failures)
    if path == "bf16.whole":
        assert torch.count_nonzero(part.view(-1, 3, H * hd)[:, 1]).item() == 0
        check(f"{name}.bias_v", rel(bg[2], do.double().view(B, N, H, hd).sum((0, 1))), FUSED_BV, failures)
    else:
        check(f"{name}.bias_k", rel(bg[1], bw[1], qden), bounds["bk"], failures)
        check(f"{name}.bias_v", rel(bg[2], bw[2]), bounds["bv"], failures)
    assert not failures, "; ".join(failures)


# ------------------------------------------------------------------------- 4. determinism of the backward ---
@pytest.mark.parametrize("path,B,N,H", [("bf16.whole", 44, 197, 12), ("bf16.stream", 44, 197, 12),
                                         ("bf16.stream", 4, 785, 6)])
def test_backward_is_deterministic(ops, lib, path, B, N, H):
    """Three launches on the same inputs (528 pairs: two or three per workgroup of the persistent walk): the same
    bits in dqkv and dbias_part."""
    hd = 64
    scale = hd ** -0.5
    dt = force(lib, path)
    qkv, do = U.normal_inputs(B, N, H, hd, 4000 + N)
    Q, DO = qkv.to("cuda", dt), do.to("cuda", dt)
    O, lse = forward(ops, Q, B, N, H, hd, scale)
    runs = [backward(ops, Q, O, DO, lse, B, N, H, hd, scale, dbias=True) for _ in range(3)]
    torch.cuda.synchronize()
    assert torch.isfinite(runs[0][0].float()).all() and torch.isfinite(runs[0][1]).all()
    for i, (dqkv, part) in enumerate(runs[1:], 1):
        assert torch.equal(bits(dqkv), bits(runs[0][0])), f"launch {i}: dqkv differs from launch 0"
        assert torch.equal(bits(part), bits(runs[0][1])), f"launch {i}: dbias_part differs from launch 0"


# ------------------------------------------------------------------------------------- 5. no stray stores ---
GUARD = 4096               # elements on either side: more than a token row of dqkv (3 * H * hd = 576), 16-byte multiple
STRAY_CASES = [(p, n) for p in ("bf16.whole", "bf16.stream") for n in (1, 197, 255, 257) if n <= 256 or p in ANY_N]


def guarded(shape, dt, sentinel):
    """A NaN-filled contiguous interior view of a larger sentinel-filled buffer, 16-byte aligned."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * GUARD,), sentinel, device="cuda", dtype=dt)
    view = buf[GUARD:GUARD + n].view(shape)
    view.fill_(float("nan"))
    assert view.data_ptr() % 16 == 0 and view.is_contiguous()
    return buf, view


@pytest.mark.parametrize("path,N", STRAY_CASES)
def test_no_stores_outside_the_outputs(ops, lib, path, N):
    """O, lse, dqkv and dbias_part are interior views of larger buffers: after forward and backward every output
    element is written and every guard element still holds its sentinel."""
    B, H, hd = 2, 3, 64
    scale = hd ** -0.5
    dt = force(lib, path)
    qkv, do = U.normal_inputs(B, N, H, hd, 5000 + N)
    Q, DO = qkv.to("cuda", dt), do.to("cuda", dt)
    bufs = {"out": guarded((B, N, H * hd), dt, -7.0), "lse": guarded((B * H * N,), torch.float32, -7.0),
            "dqkv": guarded((B, N, 3 * H * hd), dt, -7.0),
            "dbias_part": guarded((ops.attn_bwd_dbias_rows(B, N), 3 * H * hd), torch.float32, -7.0)}
    ops.attn_fwd(Q, bufs["out"][1], bufs["lse"][1], B, N, H, hd, scale)
    ops.attn_bwd(Q, bufs["out"][1], DO, bufs["lse"][1], bufs["dqkv"][1], B, N, H, hd, scale,
                 dbias_part=bufs["dbias_part"][1])
    torch.cuda.synchronize()
    for k, (buf, view) in bufs.items():
        assert torch.isfinite(view.float()).all(), f"{k}: an output element was not written"
        lo, hi = buf[:GUARD].float(), buf[GUARD + view.numel():].float()
        assert (lo == -7.0).all() and (hi == -7.0).all(), \
            f"{k}: {int((lo != -7.0).sum())} guard elements before and {int((hi != -7.0).sum())} after the tensor were overwritten"


# ------------------------------------------------------------------------------------------ 6. refusals ---
def refused(ops, match, Q, B, N, H, hd, fwd=True, bwd=True, dbias=False, DO=None):
    """attn_fwd / attn_bwd raise VitmiError naming the argument, and their NaN-filled outputs stay untouched."""
    from vit_torch_amd._lib import VitmiError
    dt = Q.dtype
    O, lse = nan((B, N, H * hd), dt), nan((B * H * N,), torch.float32)
    if fwd:
        with pytest.raises(VitmiError, match=match):
            ops.attn_fwd(Q, O, lse, B, N, H, hd, hd ** -0.5)
    if bwd:
        dqkv = nan((B, N, 3 * H * hd), dt)
        part = nan((ops.attn_bwd_dbias_rows(B, N), 3 * H * hd), torch.float32) if dbias else None
        Oin, lin = torch.zeros_like(O), torch.zeros_like(lse)
        with pytest.raises(VitmiError, match=match):
            ops.attn_bwd(Q, Oin, torch.zeros_like(O) if DO is None else DO, lin, dqkv, B, N, H, hd, hd ** -0.5,
                         dbias_part=part)
        torch.cuda.synchronize()
        assert dqkv.isnan().all() and (part is None or part.isnan().all())
    torch.cuda.synchronize()
    assert O.isnan().all() and lse.isnan().all()


@pytest.mark.parametrize("hd", [16, 48, 128])
def test_refuses_bf16_head_dims_other_than_32_and_64(ops, lib, hd):
    B, N, H = 2, 33, 2
    refused(ops, "head dim", torch.zeros((B, N, 3 * H * hd), device="cuda", dtype=torch.bfloat16), B, N, H, hd)


@pytest.mark.parametrize("path", ["fp32.matrix", "fp32.valu"])
def test_refuses_fp32_head_dims_above_64(ops, lib, path):
    B, N, H, hd = 2, 33, 2, 80
    force(lib, path)
    refused(ops, "head dim", torch.zeros((B, N, 3 * H * hd), device="cuda"), B, N, H, hd)


@pytest.mark.parametrize("path", ["bf16.whole", "bf16.stream", "fp32.valu"])
def test_refuses_more_pairs_than_the_grid_holds(ops, lib, path):
    """B * H = 65536 pairs on the paths whose grid carries the pair index in y (fp32.matrix carries it in x)."""
    B, N, H, hd = 16384, 1, 4, 32
    dt = force(lib, path)
    refused(ops, r"B\*H", torch.zeros((B, N, 3 * H * hd), device="cuda", dtype=dt), B, N, H, hd)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
def test_refuses_a_workspace_that_is_too_small(ops, lib, dt):
    from vit_torch_amd._lib import VitmiError, check
    B, N, H, hd = 2, 33, 3, 64
    Q = torch.zeros((B, N, 3 * H * hd), device="cuda", dtype=dt)
    O, lse, dqkv = torch.zeros((B, N, H * hd), device="cuda", dtype=dt), torch.zeros(B * H * N, device="cuda"), \
        nan((B, N, 3 * H * hd), dt)
    need = lib.vitmi_attn_bwd_workspace(B, N, H)
    assert need == B * N * H * 4
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    with pytest.raises(VitmiError, match="workspace"):
        check(lib.vitmi_attn_bwd(Q.data_ptr(), O.data_ptr(), O.data_ptr(), lse.data_ptr(), dqkv.data_ptr(),
                                 ops.dtype_code(Q), B, N, H, hd, hd ** -0.5, None, 0, ws.data_ptr(), need - 4,
                                 torch.cuda.current_stream().cuda_stream), "vitmi_attn_bwd")
    torch.cuda.synchronize()
    assert dqkv.isnan().all()


def test_refuses_dbias_part_in_fp32(ops, lib):
    B, N, H, hd = 2, 33, 3, 64
    refused(ops, "dbias_part", torch.zeros((B, N, 3 * H * hd), device="cuda"), B, N, H, hd, fwd=False, dbias=True)


def test_refuses_a_qkv_view_two_bytes_off(ops, lib):
    B, N, H, hd = 2, 33, 3, 64
    Q = torch.zeros((B * N * 3 * H * hd + 1,), device="cuda", dtype=torch.bfloat16)[1:].view(B, N, 3 * H * hd)
    assert Q.data_ptr() % 16 == 2 and Q.is_contiguous()
    refused(ops, "qkv", Q, B, N, H, hd)
