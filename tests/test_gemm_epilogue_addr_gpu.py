"""The 256x256 tile kernel's epilogue addressing (gemm_fast.hip; uniform_ptr / lane_off / lane_ptr in gemm_tile.h): one
wave-uniform 64-bit base per array and tile in scalar registers plus one 32-bit byte offset per lane.

Every case gives C, C2 and R / AUX a leading dimension of their own (row + 8 / + 24 / + 40, all different from N and from
each other; C of the plain store is a column slice of an [M, 3N] buffer, as qkv is used) and a base address inside a
larger NaN-filled allocation; colsum_part (indexed with N by the kernel) is a row range inside a NaN-filled [G + 4, N].
Each bf16-output case runs under both store policies, because the policy selects the epilogue the plan takes: with the
`nt` policy the plain store, the fc1 GELU pair and the gelu'-multiply take their straight-line form (DEEP 2) and the
residual the general row function behind deep side loads (DEEP 1); with the default policy the residual without a second
output takes DEEP 2 and the gelu'-multiply DEEP 1.  The case asserts the plan's `deep` through vitmi_debug_gemm_plan.  The outputs are compared to the float64 reference with the helpers and bounds of
tests/gemm_util.py (FP32_GRADE for fp32 outputs, rounding_check with delta = FP32_GRADE * max |want| for bf16 ones, the
colsum bound of tests/test_gemm_gpu.py); everything outside the addressed sub-matrices must still be NaN and nothing
inside may be.  On top of that each case runs as the persistent walk and as one tile per workgroup
(VITMI_LAUNCH_SHARED_DEVICE), each with the counted prefetch wait and with vitmi_debug_gemm_strict_wait(1): the four
results must be bit-equal.

A split-K weight gradient and a paired weight gradient (k-minor operands, fp32 C, NaN-filled workspace) run in the same
four launch forms with the same checks.

M = 300 has a ragged last row tile; M = 384 puts the second half of the last tile wholly into the padding rows
(VITMI_LAUNCH_ROWS_PADDED), where colsum_part has no row.
"""
import ctypes

import pytest
import torch

import gemm_util as U
from gemm_util import EPI_BIAS_GELU, EPI_DGELU, EPI_RESIDUAL, EPI_STORE, FP32_GRADE, F64

BF, F32 = torch.bfloat16, torch.float32
NAN = float("nan")
SHARED_DEVICE, ROWS_PADDED = 1, 2
COLSUM_CAP = 2e-3

SHAPES = [(256, 256, 64), (512, 512, 128), (300, 256, 128), (384, 512, 64)]
# name: (epilogue, C is bf16, options)
EPIS = {
    "store-bf16": (EPI_STORE, True, ("bias", "slice")),
    "store-fp32": (EPI_STORE, False, ("bias",)),
    "res-bf16": (EPI_RESIDUAL, True, ("bias",)),
    "res-bf16-gamma": (EPI_RESIDUAL, True, ("bias", "gamma")),
    "res-fp32": (EPI_RESIDUAL, False, ("bias",)),
    "res-fp32-gamma-c2": (EPI_RESIDUAL, False, ("bias", "gamma", "C2")),
    "gelu-c2": (EPI_BIAS_GELU, True, ("bias", "C2", "deriv")),
    "dgelu-colsum": (EPI_DGELU, True, ("deriv", "colsum")),
}
# every epilogue in the layout(s) the tile kernel is built for (the gelu'-multiply exists as nn only); the plain stores
# in all three
CASES = [(s, "nt", e) for s in SHAPES for e in EPIS if e != "dgelu-colsum"]
CASES += [(s, "nn", e) for s in SHAPES for e in ("store-bf16", "dgelu-colsum")]          # the data gradients of a step
CASES += [(s, "tn", e) for s in SHAPES[:2] for e in ("store-bf16", "store-fp32")]         # (ragged M needs a k-major A)
assert all(U.tile_combo_built(l, EPIS[e][0], EPIS[e][1]) for _, l, e in CASES)


def test_lane_offset_overflow_refuses_the_tile_kernel_cpu():
    """Host only: a leading dimension at which (RPI * ld + 64) * esz reaches 2^31 (RPI = 8 rows per wave instruction for a
    bf16 C, 4 for an fp32 one) is refused by the plan — gemm_uses_fast reports False, as for any other unsupported
    argument — and the largest one below is accepted."""
    from vit_torch_amd import ops
    from vit_torch_amd._lib import BF16, F32 as F32_CODE
    for c_dtype, rpi, esz in ((BF16, 8, 2), (F32_CODE, 4, 4)):
        first_bad = ((1 << 31) // esz - 64 + rpi - 1) // rpi
        first_bad = (first_bad + 7) // 8 * 8                       # leading dimensions of the tile kernel are multiples of 8
        assert (rpi * first_bad + 64) * esz >= 1 << 31 and (rpi * (first_bad - 8) + 64) * esz < 1 << 31
        assert ops.gemm_uses_fast(256, 256, 64, c_dtype=c_dtype, ldc=264)
        assert ops.gemm_uses_fast(256, 256, 64, c_dtype=c_dtype, ldc=first_bad - 8)
        assert not ops.gemm_uses_fast(256, 256, 64, c_dtype=c_dtype, ldc=first_bad)
        assert not ops.gemm_uses_fast(256, 256, 64, c_dtype=c_dtype, ldc=1 << 30)


@pytest.fixture(scope="module")
def ops(lib):
    from vit_torch_amd import ops as _o
    return _o


@pytest.fixture(scope="module")
def problems():
    """Inputs and float64 products, computed once per (shape, layout-independent) problem and left unchanged."""
    out = {}
    for M, N, K in SHAPES:
        x = U.make_inputs("normal", M, N, K, None, 1000 + M + N + K, side_bf16=False)
        x["acc"] = x["a"] @ x["b"].t()
        x["R16"] = U.bf16(x["R"])
        out[(M, N, K)] = x
    return out


def colsum_bound(v, colsum):
    G, N = colsum.shape
    pad = torch.zeros((G * 128, N), dtype=F64)
    pad[:v.shape[0]] = v.abs()
    s = pad.view(G, 128, N).sum(1).max().item()
    return min(COLSUM_CAP, 128 * (2.0 ** -24 * s + FP32_GRADE * v.abs().max().item()) / colsum.abs().max().item())


def outside_is_nan(buf, r0, r1, c0, c1):
    """Everything of `buf` outside rows r0..r1, columns c0..c1 is still NaN."""
    m = torch.isnan(buf.float())
    m[r0:r1, c0:c1] = True
    return bool(m.all())


def expected_deep(name, policy):
    """The DEEP of the main kernel's epilogue plan_fast chooses (gemm_fast.hip) for a case under a store policy."""
    epi, c_bf16, opts = EPIS[name]
    if not c_bf16:
        return 0
    if epi == EPI_RESIDUAL:
        return 2 if (policy == 0 and "C2" not in opts) else 1
    if epi == EPI_DGELU:
        return 2 if policy == 2 else 1
    return 2 if policy == 2 else 0


def launch(ops, lib, x, M, N, K, layout, name, flags, strict, policy):
    epi, c_bf16, opts = EPIS[name]
    akm, bkm = U.LAYOUTS[layout]
    Mp = (M + 255) // 256 * 256
    cdt = BF if c_bf16 else F32
    lib.vitmi_debug_reset()
    lib.vitmi_debug_gemm_tile(1)
    lib.vitmi_debug_gemm_strict_wait(int(strict))
    lib.vitmi_debug_gemm_store_policy(policy)
    _, A = U.place(x["a"] if akm else x["a"].t(), 8, BF, "cuda")
    _, B = U.place(x["b"] if bkm else x["b"].t(), 24, BF, "cuda")
    r = {}
    if "slice" in opts:                                 # C = the middle third of an [Mp, 3N] matrix, itself inside NaN
        r["Cbuf"] = torch.full((Mp + 4, 3 * N + 8), NAN, dtype=cdt, device="cuda")
        r["Cbox"] = (2, 2 + Mp, N, 2 * N)
        C = r["Cbuf"][2:2 + M, N:2 * N]
    else:
        r["Cbuf"], C = U.place(torch.full((M, N), NAN, dtype=F64), 24, cdt, "cuda", rows_alloc=Mp)
        r["Cbox"] = (2, 2 + Mp, 0, N)
    kw = dict(a_kmajor=akm, b_kmajor=bkm, epilogue=epi, launch_flags=flags | (ROWS_PADDED if M % 256 else 0))
    if "bias" in opts:
        kw["bias"] = x["bias"].to(F32).cuda()
    if "gamma" in opts:
        kw["gamma"] = x["gamma"].to(F32).cuda()
    if "deriv" in opts:
        kw["aux_deriv"] = True
    if "C2" in opts:
        r["C2buf"], kw["C2"] = U.place(torch.full((M, N), NAN, dtype=F64), 40, BF if epi == EPI_RESIDUAL else cdt, "cuda", rows_alloc=Mp)
    if epi == EPI_RESIDUAL:
        _, kw["R"] = U.place(x["R16"] if c_bf16 else x["R"], 8, cdt, "cuda", rows_alloc=Mp, surplus=0.5)
    if epi == EPI_DGELU:
        _, kw["aux"] = U.place(x["aux"], 8, BF, "cuda", rows_alloc=Mp, surplus=0.5)
    if "colsum" in opts:
        G = (M + 127) // 128
        r["partbuf"] = torch.full((G + 4, N), NAN, device="cuda")
        kw["colsum_part"] = r["partbuf"][2:2 + G]
    d = ops._gemm_desc(A, B, C, **kw)
    assert lib.vitmi_gemm_uses_fast(ctypes.byref(d)), "the case does not take the tile kernel"
    plan = [ctypes.c_int(-7) for _ in range(4)]
    assert lib.vitmi_debug_gemm_plan(ctypes.byref(d), *map(ctypes.byref, plan)) == 0
    assert plan[0].value == U.PLAN_KINDS["WHOLE"] and plan[2].value == expected_deep(name, policy), \
        f"plan (kind, pipe, deep, splits) = {[v.value for v in plan]}: not the epilogue this case is about"
    ops.gemm(A, B, C, **kw)
    torch.cuda.synchronize()
    lib.vitmi_debug_reset()
    r["C"], r["C2"], r["part"] = C, kw.get("C2"), kw.get("colsum_part")
    return r


# store policy 0 (write-back) and 2 (`nt`); an fp32 output has one epilogue whatever the policy
POLICY_CASES = [(s, l, e, p) for s, l, e in CASES for p in ((0, 2) if EPIS[e][1] else (0,))]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,layout,name,policy", POLICY_CASES,
                         ids=[f"{s[0]}x{s[1]}x{s[2]}-{l}-{e}-{'nt' if p else 'wb'}" for s, l, e, p in POLICY_CASES])
def test_epilogue_addressing(ops, lib, problems, shape, layout, name, policy):
    M, N, K = shape
    Mp = (M + 255) // 256 * 256
    x = problems[shape]
    epi, c_bf16, opts = EPIS[name]
    runs = [launch(ops, lib, x, M, N, K, layout, name, flags, strict, policy) for flags in (0, SHARED_DEVICE) for strict in (0, 1)]
    first = runs[0]
    # ---- stray writes and unwritten elements
    for r in runs:
        assert outside_is_nan(r["Cbuf"], *r["Cbox"]), "C: a store outside the matrix"
        assert torch.isfinite(r["C"].float()).all(), "C: an element not written"
        if r["C2"] is not None:
            assert U.canaries_intact(r["C2buf"], M, N, rows_alloc=Mp), "C2: a store outside the matrix"
            assert torch.isfinite(r["C2"].float()).all(), "C2: an element not written"
        if r["part"] is not None:
            G = r["part"].shape[0]
            assert torch.isnan(r["partbuf"][:2]).all() and torch.isnan(r["partbuf"][2 + G:]).all(), "colsum_part: a row outside written"
            assert torch.isfinite(r["part"]).all(), "colsum_part: an element not written"
    # ---- the launch forms and the two waits agree bit for bit
    for r in runs[1:]:
        for k in ("C", "C2", "part"):
            if first[k] is not None:
                assert torch.equal(first[k], r[k]), f"{k}: launch forms / waits differ"
    # ---- against float64
    R = (x["R16"] if c_bf16 else x["R"]) if epi == EPI_RESIDUAL else None
    want = U.reference(None, None, epilogue=epi, acc=x["acc"], bias=x["bias"] if "bias" in opts else None, R=R,
                       gamma=x["gamma"] if "gamma" in opts else None, aux=x["aux"] if epi == EPI_DGELU else None,
                       aux_deriv="deriv" in opts, want_c2="C2" in opts, want_colsum="colsum" in opts)
    outs = [("C", first["C"], want.C, c_bf16)]
    if first["C2"] is not None:
        outs.append(("C2", first["C2"], want.C2, first["C2"].dtype == BF))
    for nm, got, w, is16 in outs:
        g = got.cpu()
        if is16:
            bad, share, worst = U.rounding_check(g, w, FP32_GRADE * w.abs().max().item())
            print(f"\n  {nm}: {bad} elements off the rounding of float64 (band share {share:.2%}, worst |err| {worst:.2e})", end="")
            assert bad == 0, f"{nm}: {bad} of {g.numel()} elements are not the bf16 rounding of the float64 result"
        else:
            e = U.rel(g, w)
            print(f"\n  {nm}: rel {e:.2e} (bound {FP32_GRADE:.0e})", end="")
            assert e <= FP32_GRADE, f"{nm}: rel {e:.2e} > {FP32_GRADE:.0e}"
    if first["part"] is not None:
        v = U.reference(None, None, epilogue=epi, acc=x["acc"], aux=x["aux"], aux_deriv=True).C
        e, bound = U.rel(first["part"].cpu(), want.colsum), colsum_bound(v, want.colsum)
        print(f"\n  colsum_part: rel {e:.2e} (bound {bound:.2e})", end="")
        assert e <= bound, f"colsum_part: rel {e:.2e} > {bound:.2e}"


# ------------------------------------------------------------------------------------- weight gradients ---
def wgrad_operands(x, ea, eb):
    """k-minor operands [K, M] / [K, N] of a weight gradient, each at its own leading dimension inside NaN."""
    _, A = U.place(x["a"].t(), ea, BF, "cuda")
    _, B = U.place(x["b"].t(), eb, BF, "cuda")
    return A, B


def check_wgrad(runs, wants, shapes):
    """runs: per launch form a list of (Cbuf, C) per product."""
    for r in runs:
        for (Cbuf, C), (M, N) in zip(r, shapes):
            assert U.canaries_intact(Cbuf, M, N), "C: a store outside the matrix"
            assert torch.isfinite(C).all(), "C: an element not written"
    for r in runs[1:]:
        for (_, C0), (_, C) in zip(runs[0], r):
            assert torch.equal(C0, C), "launch forms / waits differ"
    for (_, C), w in zip(runs[0], wants):
        e = U.rel(C.cpu(), w)
        print(f"\n  C: rel {e:.2e} (bound {FP32_GRADE:.0e})", end="")
        assert e <= FP32_GRADE, f"C: rel {e:.2e} > {FP32_GRADE:.0e}"


@pytest.mark.gpu
def test_split_k_weight_gradient(ops, lib):
    """[256, 256] = A^T B over K = 1088 (17 k-steps: the last slice is short), fp32 C: the contraction is split over
    workgroups, each stores its raw slab, the reduce writes C."""
    M, N, K = 256, 256, 1088
    x = U.make_inputs("normal", M, N, K, None, 4321)
    want = x["a"] @ x["b"].t()
    runs = []
    for flags in (0, SHARED_DEVICE):
        for strict in (0, 1):
            lib.vitmi_debug_reset()
            lib.vitmi_debug_gemm_tile(1)
            lib.vitmi_debug_gemm_strict_wait(strict)
            A, B = wgrad_operands(x, 8, 24)
            Cbuf, C = U.place(torch.full((M, N), NAN, dtype=F64), 40, F32, "cuda")
            kw = dict(a_kmajor=False, b_kmajor=False, launch_flags=flags)
            d = ops._gemm_desc(A, B, C, **kw)
            need = lib.vitmi_gemm_workspace(ctypes.byref(d))
            assert need > 0, "no workspace asked for: the contraction is not split"
            ws = ops.workspace(need, A.device)
            ws[:ws.numel() // 4 * 4].view(F32).fill_(NAN)
            d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
            plan = [ctypes.c_int(-7) for _ in range(4)]
            assert lib.vitmi_debug_gemm_plan(ctypes.byref(d), *map(ctypes.byref, plan)) == 0
            assert plan[0].value == U.PLAN_KINDS["SPLITK"] and plan[3].value > 1, f"plan = {[v.value for v in plan]}"
            ops.gemm(A, B, C, **kw)
            torch.cuda.synchronize()
            lib.vitmi_debug_reset()
            runs.append([(Cbuf, C)])
    check_wgrad(runs, [want], [(M, N)])


@pytest.mark.gpu
def test_paired_weight_gradients(ops, lib):
    """(256, 256) and (768, 256) over K = 1024 in one split-K launch (vitmi_gemm_pair), each C at its own leading
    dimension inside NaN."""
    K, shapes = 1024, [(256, 256), (768, 256)]
    xs = [U.make_inputs("normal", M, N, K, None, 99 + M) for M, N in shapes]
    wants = [x["a"] @ x["b"].t() for x in xs]
    assert ops.gemm_pair_shares_a_launch(256, 256, 768, 256, K)
    runs = []
    for flags in (0, SHARED_DEVICE):
        for strict in (0, 1):
            lib.vitmi_debug_reset()
            lib.vitmi_debug_gemm_strict_wait(strict)
            t, outs = [], []
            for x, (M, N), (ea, eb, ec) in zip(xs, shapes, ((8, 24, 40), (16, 8, 24))):
                A, B = wgrad_operands(x, ea, eb)
                Cbuf, C = U.place(torch.full((M, N), NAN, dtype=F64), ec, F32, "cuda")
                t += [A, B, C]
                outs.append((Cbuf, C))
            ops.workspace(1 << 20, "cuda").fill_(0xFF)
            ops.gemm_pair(*t, launch_flags=flags)
            torch.cuda.synchronize()
            lib.vitmi_debug_reset()
            runs.append(outs)
    check_wgrad(runs, wants, shapes)


# ------------------------------------------------------------------------------------ registers, host only ---
def test_step_kernels_use_no_scratch_cpu():
    """The tile-GEMM instantiations a bf16 ViT step launches report no scratch and at most 256 VGPRs in hipcc's
    resource-usage remarks (vit_torch_amd.build.kernel_resources): <A_KM, B_KM, MODE, bf16, SPLITK, PIPE, FIX, DEEP>."""
    from vit_torch_amd import build
    if not (build.OBJ / "gemm_fast.hip.resources.json").exists():
        build.build()
    res = build.kernel_resources("gemm_fast.hip")
    step = [(1, 0, 3, 0, 1, 0, 2), (1, 1, 2, 0, 2, 0, 2), (1, 1, 2, 0, 1, 0, 2), (1, 1, 0, 0, 2, 0, 2), (1, 0, 0, 0, 1, 0, 2),
            (1, 1, 1, 0, 2, 0, 2), (1, 0, 3, 0, 2, 0, 2)]
    for a, b, mode, sk, pipe, fix, deep in step:
        tag = f"gemm_fast_kernelILb{a}ELb{b}ELi{mode}EDF16bLb{sk}ELi{pipe}ELb{fix}ELi{deep}EE"
        hit = [v for k, v in res.items() if tag in k]
        assert len(hit) == 1, f"{tag}: {len(hit)} kernels of that name"
        assert int(hit[0]["ScratchSize [bytes/lane]"]) == 0, f"{tag}: scratch {hit[0]['ScratchSize [bytes/lane]']} B"
        assert int(hit[0]["VGPRs"]) <= 256
    for k, v in res.items():
        assert int(v["VGPRs"]) <= 256, k
