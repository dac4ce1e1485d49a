"""The references of tests/test_gemm_gpu.py checked on the CPU: gemm_util.reference against independent float64
formulations through torch.autograd, the rounding emulation against the reference, the conditions the `integer` family
and the rounding-band metric must meet on every case the GPU module runs, the float32 emulation of the tile kernels'
GELU, and the figures frozen in the GPU module (recomputed here: they cannot rot)."""
import functools

import pytest
import torch
import torch.nn.functional as F

import gemm_util as U
import test_gemm_gpu as G
from gemm_util import EPI_BIAS_GELU, EPI_DGELU, EPI_PATCH_POS, EPI_RESIDUAL, EPI_STORE, F64


def rn(shape, seed):
    return torch.randn(shape, generator=torch.Generator("cpu").manual_seed(seed), dtype=F64)


# ------------------------------------------------------------------------------------ independence ---
def test_reference_is_the_mlp_block_with_layerscale_and_droppath():
    """Linear -> GELU -> Linear + residual with LayerScale and a per-sample DropPath mask, forward and backward, against
    torch.nn.functional in float64 with autograd: EPI_BIAS_GELU (both C2 forms), EPI_RESIDUAL (C, C2), EPI_DGELU (both
    forms, colsum_part = the fc1 bias gradient), the two weight-gradient layouts."""
    Bn, T, D, Hd = 3, 50, 24, 40
    M = Bn * T
    x0 = rn((M, D), 1).requires_grad_(True)
    W1, b1, W2, b2 = (rn(s, i).requires_grad_(True) for i, s in enumerate([(Hd, D), (Hd,), (D, Hd), (D,)], 2))
    gamma = rn((D,), 6).requires_grad_(True)
    keep = torch.tensor([0.0, 1.0 / 0.75, 1.0 / 0.75], dtype=F64)
    pre = F.linear(x0, W1, b1)
    h = F.gelu(pre)
    f = F.linear(h, W2, b2)
    y = x0 + keep.repeat_interleave(T)[:, None] * (gamma * f)
    dy = rn((M, D), 7)
    y.backward(dy)

    r1 = U.reference(x0.detach(), W1.detach(), epilogue=EPI_BIAS_GELU, bias=b1.detach(), want_c2=True)
    assert U.rel(r1.C, h.detach()) <= 1e-14 and U.rel(r1.C2, pre.detach()) <= 1e-14
    r1d = U.reference(x0.detach(), W1.detach(), epilogue=EPI_BIAS_GELU, bias=b1.detach(), want_c2=True, aux_deriv=True)
    r2 = U.reference(r1.C, W2.detach(), epilogue=EPI_RESIDUAL, bias=b2.detach(), R=x0.detach(), gamma=gamma.detach(),
                     rowscale=keep, rows_per_group=T, want_c2=True)
    assert U.rel(r2.C, y.detach()) <= 1e-14 and U.rel(r2.C2, f.detach()) <= 1e-14
    # backward: df = dy * keep * gamma; dh = df W2 (nn layout); dpre = dh * gelu'(pre); db1 = column sums of dpre
    df = dy * keep.repeat_interleave(T)[:, None] * gamma.detach()
    for kw in (dict(aux=r1.C2), dict(aux=r1d.C2, aux_deriv=True)):
        r3 = U.reference(df, W2.detach(), b_kmajor=False, epilogue=EPI_DGELU, want_colsum=True, **kw)
        gW1 = U.reference(r3.C, x0.detach(), a_kmajor=False, b_kmajor=False).C                          # dpre^T x: tn layout
        assert U.rel(gW1, W1.grad) <= 1e-13
        assert U.rel(r3.colsum.sum(0), b1.grad) <= 1e-13
        assert r3.colsum.shape == ((M + 127) // 128, Hd)
        assert U.rel(r3.colsum[1], r3.C[128:].sum(0)) <= 1e-14
    # dx through fc1 accumulated onto the residual gradient: EPI_STORE with accumulate (nn layout), alpha
    dx = U.reference(r3.C, W1.detach(), b_kmajor=False, C_in=dy).C
    assert U.rel(dx, x0.grad) <= 1e-13
    half = U.reference(r3.C, W1.detach(), b_kmajor=False, alpha=0.5, bias=b1.detach()[:D]).C
    assert U.rel(half, 0.5 * (r3.C @ W1.detach()) + b1.detach()[:D]) <= 1e-14
    # tt layout: both operands stored k-minor / k-major swapped
    tt = U.reference(x0.detach().t().contiguous(), W1.detach(), a_kmajor=False, b_kmajor=True).C
    assert U.rel(tt, x0.detach() @ W1.detach().t()) <= 1e-14


def test_reference_is_the_patch_embedding_with_cls_and_pos():
    """cat(cls, x W^T + b) + pos per image against EPI_PATCH_POS on rows with a zero placeholder where the CLS token goes."""
    Bn, T, Kp, D = 3, 7, 12, 10
    patches = rn((Bn, T - 1, Kp), 1)
    W, b, cls, pos = rn((D, Kp), 2), rn((D,), 3), rn((D,), 4), rn((T, D), 5)
    want = torch.cat((cls.expand(Bn, 1, D), F.linear(patches, W, b)), 1) + pos
    rows = torch.cat((torch.full((Bn, 1, Kp), 123.0, dtype=F64), patches), 1).reshape(Bn * T, Kp)
    r = U.reference(rows, W, epilogue=EPI_PATCH_POS, bias=b, pos=pos.reshape(-1), n_tok=T, cls=cls)
    assert U.rel(r.C, want.reshape(Bn * T, D)) <= 1e-14
    # without cls row 0 is an ordinary token
    r0 = U.reference(rows, W, epilogue=EPI_PATCH_POS, bias=b, pos=pos.reshape(-1), n_tok=T)
    assert U.rel(r0.C, (F.linear(rows, W, b).view(Bn, T, D) + pos).reshape(Bn * T, D)) <= 1e-14


def test_reference_dgelu_is_autograd_through_gelu():
    x = torch.cat((rn((300,), 1) * 3, torch.tensor([0.0, -0.75179, 0.75179, -8.0, 8.0, -30.0, 30.0], dtype=F64))).requires_grad_(True)
    F.gelu(x).sum().backward()
    assert (U.dgelu64(x.detach()) - x.grad).abs().max().item() <= 1e-15
    assert (U.gelu64(x.detach()) - F.gelu(x.detach())).abs().max().item() <= 1e-14


# --------------------------------------------------------------------------------------- emulation ---
@pytest.mark.parametrize("epi", U.ALL_EPIS, ids=[U.EPI_NAMES[e] for e in U.ALL_EPIS])
def test_emulation_without_rounding_is_the_reference(epi):
    M, N, K = 130, 40, 24
    x = U.make_inputs("normal", M, N, K, epi, 5, n_tok=U.NTOK, rows_per_group=U.rpg(M))
    for opts in U.option_sets(epi, False, True) + [("deriv", "C2")]:
        kw = U.ref_kwargs(x, epi, opts)
        r = U.reference(x["a"], x["b"], epilogue=epi, **kw)
        e = U.emulated(x["a"], x["b"], c_bf16=True, rounding=False, epilogue=epi, **kw)
        for a, b in zip(r, e):
            assert (a is None) == (b is None)
            assert a is None or torch.equal(a, b)
        er = U.emulated(x["a"], x["b"], c_bf16=True, epilogue=epi, **kw)
        assert torch.equal(er.C, U.bf16(er.C)) and U.rel(er.C, r.C) <= 2.0 ** -8      # rounded, and by no more than bf16's half ulp + GELU's slope
        if epi == EPI_BIAS_GELU and "deriv" not in opts and er.C2 is not None:
            assert torch.equal(er.C2, U.bf16(r.C2)) and torch.equal(er.C, U.bf16(U.gelu64(er.C2)))
        if er.colsum is not None:
            assert torch.equal(er.colsum, r.colsum)            # the sums are taken of the unrounded values


def test_rne_bf16_is_torchs_rounding_and_the_check_is_strict():
    v = torch.cat((rn((20000,), 3).float() * 7, U.finite_bf16_line()[::7], torch.tensor([1e-40, -3e-39, 0.0]))).to(F64)
    v = v[v.abs() < 3e38]
    assert torch.equal(U.rne_bf16(v), v.float().to(torch.bfloat16).to(F64))
    want = torch.tensor([1.0 + 2.0 ** -8 + 1e-6, 1.0 + 2.0 ** -8 + 1e-3, 1.0, 1.0, 0.0], dtype=F64)
    ulp = 2.0 ** -7
    for got, bad in (([1 + ulp, 1 + ulp, 1, 1, 0], 0), ([1.0, 1 + ulp, 1, 1, 0], 0), ([1 + ulp, 1.0, 1, 1, 0], 1),
                     ([1 + 2 * ulp, 1 + ulp, 1, 1, 0], 1), ([1 + ulp, 1 + ulp, 1 + ulp, 1, 0], 1),
                     ([1 + ulp, 1 + ulp, 1, float("nan"), 0], 1)):
        n, share, _ = U.rounding_check(torch.tensor(got, dtype=torch.bfloat16), want, 1e-5)
        assert n == bad, (got, n)
        assert share == pytest.approx(2 / 5)                  # element 0 (near a boundary) and the zero (delta > its ulp)


# ------------------------------------------------------------------------- conditions on the cases ---
base = G.base


@pytest.mark.parametrize("path", list(U.PATHS))
def test_integer_family_meets_its_conditions_on_every_case(path):
    """Section 3.1's cases: max |want| <= 256 where the output is bf16, < 2^24 otherwise, and every value exact in the
    output dtype — for C, C2 and (fp32) colsum_part.  Rows whose rowscale is 0 exist in every rowscale case."""
    P = U.PATHS[path]
    n = 0
    for M, N, K, layout, epi, c_bf16, opts in U.cases(path, "3.1"):
        x = base("integer", M, N, K, P["in_bf16"], c_bf16, U.big_factor(opts, K))
        assert set(x["a"].unique().tolist()) <= {-64.0, -1.0, 0.0, 1.0, 64.0}
        want = U.reference(None, None, epilogue=epi, acc=x["acc"], **U.ref_kwargs(x, epi, opts))
        name = G.opt_name(M, N, K, layout, epi, c_bf16, opts, {})
        if epi != EPI_BIAS_GELU:
            assert U.integer_conditions(want.C, c_bf16) is None, f"{name}: {U.integer_conditions(want.C, c_bf16)}"
        if want.C2 is not None:
            b = c_bf16 if epi == EPI_BIAS_GELU else P["in_bf16"]
            assert U.integer_conditions(want.C2, b) is None, f"{name} C2: {U.integer_conditions(want.C2, b)}"
        if want.colsum is not None:
            assert U.integer_conditions(want.colsum, False) is None
        if "rowscale" in opts:
            assert (x["rowscale"] == 0).any() and (x["rowscale"] != 0).any(), f"{name}: dropped and kept groups are both needed"
        n += 1
    assert n > 0


def test_integer_accumulators_stay_small():
    """max |acc| of the family's operands at the contraction lengths the cases use (the issue's CPU run: 12, 34, 65, 135 at
    K = 64, 768, 3072, 12608, from other draws): far below 2^24, and below 256 up to K = 3072."""
    for K, cap in ((64, 32), (768, 64), (3072, 128), (12608, 256)):
        x = U.make_inputs("integer", 256, 256, K, None, K)
        m = (x["a"].float() @ x["b"].float().t()).abs().max().item()
        assert m <= cap, (K, m)


@pytest.mark.parametrize("path", [p for p in U.PATHS if U.PATHS[p]["in_bf16"] and any(True for _ in U.cases(p, "3.2"))])
def test_rounding_band_holds_at_most_3_percent_of_a_bf16_output(path):
    """Section 3.2's bf16 cases: the share of elements for which rounding_check accepts more than one bf16 value, from the
    reference alone, with delta = FP32_GRADE * max |want| (normalised for `scaled`).  A condition of the metric: were the
    band wide, the check would say little."""
    P = U.PATHS[path]
    worst = 0.0
    for M, N, K, layout, epi, c_bf16, opts in U.cases(path, "3.2"):
        if not c_bf16:
            continue
        for family in ("normal", "scaled"):
            x = base(family, M, N, K, True, c_bf16, 1.0)
            want = U.reference(None, None, epilogue=epi, acc=x["acc"], **U.ref_kwargs(x, epi, opts))
            wn = want.C / x["norm"]
            share = U.band_share(want.C, U.FP32_GRADE * wn.abs().max().item(), x["norm"])
            worst = max(worst, share)
            assert share <= 0.03, f"{family} {G.opt_name(M, N, K, layout, epi, c_bf16, opts, {})}: band share {share:.3%}"
    print(f"\n  {path}: worst band share {worst:.2%}", end="")


def test_cpu_fp32_matmul_mismatches_lie_inside_the_band():
    """CPU fp32 a @ b^T rounded to bf16 against the RNE of float64: every mismatch inside the band (what the band is for)."""
    for K in (64, 768):
        x = U.make_inputs("normal", 256, 512, K, None, K)
        w = x["a"] @ x["b"].t()
        got = (x["a"].float() @ x["b"].float().t()).to(torch.bfloat16)
        bad, share, _ = U.rounding_check(got, w, U.FP32_GRADE * w.abs().max().item())
        assert bad == 0 and share <= 0.03


# --------------------------------------------------------------------------- GELU and frozen figures ---
def sig3(v):
    return float(f"{v:.2e}")


def test_frozen_figures_of_the_gpu_module_are_what_this_recomputes():
    eg, ed, er = U.tile_gelu_errors()
    assert (sig3(eg), sig3(ed), sig3(er)) == (G.GELU_EMU, G.DGELU_EMU, G.GELU_EMU_REL), (eg, ed, er)
    assert G.DELTA_GELU == 4 * G.GELU_EMU and G.DELTA_DGELU == 4 * G.DGELU_EMU
    fg, fd = U.torch_gelu_f32_errors()
    assert (sig3(fg), sig3(fd)) == (G.GELU_F32, G.DGELU_F32), (fg, fd)
    assert eg >= 1.5e-7 / 2                                     # not below the published floor of the erfc fit (halved: h = erfc / 2)
    assert G.FP32_GRADE == U.FP32_GRADE == 2e-6 and G.LONG_K_GRADE == 2e-5 and G.COLSUM_CAP == 2e-3
    for v in (G.GELU_EMU, G.DGELU_EMU, G.GELU_EMU_REL, G.GELU_F32, G.DGELU_F32):
        assert f"{v:.2e}" in G.__doc__.replace("e-07", "e-7").replace("e-7", "e-07") or f"{v:.2e}".replace("e-07", "e-7") in G.__doc__


def test_tile_gelu_emulation_is_exact_at_the_ends_and_covers_the_line():
    x = U.finite_bf16_line()
    assert x.numel() == 65280 and torch.isfinite(x).all() and x.unique().numel() == 65279      # +0 and -0 compare equal
    g = U.gelu_grid()
    assert g.shape == (256, 256) and torch.equal(g.view(-1)[:65280], x)
    gl, dg = U.tile_gelu_f32(x)
    assert torch.isfinite(gl).all() and torch.isfinite(dg).all()
    big, small = x >= G.HUGE, x <= -G.HUGE
    assert torch.equal(gl[big], x[big]) and (gl[small] == 0).all()
    assert (dg[big] == 1).all() and (dg[small] == 0).all()
    x64 = x.to(F64)
    assert torch.equal(U.gelu64(x64)[big], x64[big]) and (U.gelu64(x64)[small] == 0).all()
    assert (U.dgelu64(x64)[big] == 1).all() and (U.dgelu64(x64)[small] == 0).all()
    # the band of the GELU check is narrow as well
    for fn, d in ((U.gelu64, G.DELTA_GELU), (U.dgelu64, G.DELTA_DGELU)):
        w = fn(x64)
        share = U.band_share(w, d)
        print(f"\n  band share of {fn.__name__} at delta {d:.2e}: {share:.2%}", end="")
